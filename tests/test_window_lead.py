"""The K loops of csrc/conv_mfma.hip and csrc/conv_plane.hip prefetch the next chunk's LDS window behind a ring of weight loads on the
same vmcnt counter; conv_mfma's ring waits by hand (mfma_tile.hpp: weight_fetch / ring_wait / weight_landed) so that the window stays in
flight.  What can go wrong in such a loop is a window read before it has landed, a buffer overwritten while it is still read, or a
weight used before its load returned: wrong bits, at the smallest shapes that take the loop through 1, 2 and >= 3 chunks (buffer 0
reused).  Every tile variant of both families against the CPU twins, bit for bit.

Two limits of the small-map family shape its cases: conv_plane takes Cout % 64 == 0 only (so Cout = 64, the smallest, not 32) and its
convolutions take Cin % 8 == 0 only (so the ragged Cin = 13 runs through the deconvolution, which takes any Cin); both are asserted."""
import numpy as np
import pytest
import torch

import flownet2_amd

import oracle

pytestmark = pytest.mark.gpu


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dv(a):
    return torch.from_numpy(a).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# (Cin, forced ksplit): with one part and 2 channel quads per chunk Cin = 8, 16, 24, 40 are 1, 2, 3, 5 chunks (twice that in the
# variants with one quad per chunk); two parts at Cin = 24 run 1 and 2 chunks
PLANE_CIN = [(8, 1), (16, 1), (24, 1), (40, 1), (24, 2)]


def _every_plane_variant(run, want, what):
    """run() under every forced conv_plane variant; returns how many took the geometry."""
    from flownet2_amd import ops
    ran = 0
    try:
        for v in range(ops.plane_num_variants()):
            ops.set_plane_variant(v)
            try:
                got = run()
            except flownet2_amd.Fn2Error:
                continue                                  # the other mode / stride / tap class / DMA width
            ran += 1
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), f"{what}: variant {v}"
    finally:
        ops.set_plane_variant(-1)
    return ran


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin_ksplit", PLANE_CIN)
def test_plane_conv_chunk_counts_bitwise_in_every_variant(cin_ksplit, stride):
    from flownet2_amd import ops
    (Cin, ksplit), N, H, W, Cout = cin_ksplit, 2, 5, 7, 64
    assert not ops.conv_plane_supported(N, Cin, H, W, 32, stride, 1) and not ops.conv_plane_supported(N, 13, H, W, Cout, stride, 1)
    x, w, b = rnd((N, Cin, H, W), 1), rnd((Cout, Cin, 3, 3), 2, 0.2), rnd((Cout,), 3)
    pw = ops.conv_mfma_pack_weights(dv(w))
    try:
        ops.set_plane_ksplit(ksplit)
        assert ops.conv_plane_ksplit(N, Cin, H, W, Cout, stride, 1) == ksplit
        want = oracle.conv_plane_forward(x, pw.cpu().numpy(), b, Cout, stride, 1, ksplit, True, 0.1)
        xd, bd = dv(x), dv(b)
        ran = _every_plane_variant(lambda: ops.conv_plane_forward(xd, pw, bd, Cout, stride, 1, True, 0.1), want, f"Cin {Cin} ksplit {ksplit} stride {stride}")
    finally:
        ops.set_plane_ksplit(0)
    assert ran >= 1


@pytest.mark.parametrize("cin_ksplit", PLANE_CIN + [(13, 1)])
def test_plane_deconv_chunk_counts_bitwise_in_every_variant(cin_ksplit):
    from flownet2_amd import ops
    (Cin, ksplit), N, H, W, Cout = cin_ksplit, 2, 5, 7, 64
    x, w, b = rnd((N, Cin, H, W), 4), rnd((Cin, Cout, 4, 4), 5, 0.2), rnd((Cout,), 6)
    pw = ops.deconv_plane_pack_weights(dv(w))
    try:
        ops.set_plane_ksplit(ksplit)
        assert ops.deconv_plane_ksplit(N, Cin, H, W, Cout) == ksplit
        want = oracle.deconv_plane_forward(x, pw.cpu().numpy(), b, Cout, ksplit, True, 0.1)
        assert want.shape == (N, Cout, 10, 14)
        xd, bd = dv(x), dv(b)
        ran = _every_plane_variant(lambda: ops.deconv_plane_forward(xd, pw, bd, Cout, True, 0.1), want, f"deconv Cin {Cin} ksplit {ksplit}")
    finally:
        ops.set_plane_ksplit(0)
    assert ran >= 1


def test_plane_conv_row_band_bitwise_in_every_variant():
    """One sample, 20x28 = 560 pixels: several pixel blocks per sample, each staging only its band of rows, 3 chunks.  The width is a
    multiple of 4: the 16-byte DMA variants run here (the 5x7 maps above take the dword path only), next to the dword ones."""
    from flownet2_amd import ops
    N, Cin, H, W, Cout = 1, 24, 20, 28, 64
    x, w, b = rnd((N, Cin, H, W), 7), rnd((Cout, Cin, 3, 3), 8, 0.2), rnd((Cout,), 9)
    pw = ops.conv_mfma_pack_weights(dv(w))
    try:
        ops.set_plane_ksplit(1)
        want = oracle.conv_plane_forward(x, pw.cpu().numpy(), b, Cout, 1, 1, 1, True, 0.1)
        xd, bd = dv(x), dv(b)
        ran = _every_plane_variant(lambda: ops.conv_plane_forward(xd, pw, bd, Cout, 1, 1, True, 0.1), want, "band")
    finally:
        ops.set_plane_ksplit(0)
    assert ran >= 2           # the stride-1 tiles in both DMA widths (all but the 576-slot ones cut 560 pixels into several blocks)


# (kernel, pad, Cin): 1, 2 and 3 chunks of the family's chunk (one channel quad for 5x5, two for 3x3)
DIRECT = [(5, 2, 4), (5, 2, 8), (5, 2, 12), (3, 1, 8), (3, 1, 16), (3, 1, 24)]


@pytest.mark.parametrize("case", DIRECT)
def test_direct_conv_chunk_counts_bitwise_in_every_variant(case):
    from flownet2_amd import ops
    (k, p, Cin), N, H, W, Cout, s = case, 1, 16, 16, 64, 2
    x, w, b = rnd((N, Cin, H, W), 10), rnd((Cout, Cin, k, k), 11, 0.2), rnd((Cout,), 12)
    pw = ops.conv_mfma_pack_weights(dv(w))
    want = oracle.conv_mfma_forward(x, pw.cpu().numpy(), b, Cout, k, s, p, True, 0.1)
    xd, bd = dv(x), dv(b)
    ran = 0
    try:
        nv = ops.conv_num_variants()
        for v in list(range(nv)) + [1000 + i for i in range(nv)]:          # plain launches, then the split-tail launches
            ops.set_conv_variant(v)
            try:
                got = ops.conv_mfma_forward(xd, pw, bd, Cout, k, s, p, True, 0.1)
            except flownet2_amd.Fn2Error:
                continue                                  # a variant of another kernel size / stride
            ran += 1
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), f"k {k} Cin {Cin}: variant {v}"
    finally:
        ops.set_conv_variant(-1)
    assert ran >= 1
