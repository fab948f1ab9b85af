"""The 1x1 tiles of csrc/conv_mfma.hip execute only the live channel quads of their last chunk (the packed weights pad K to whole chunks of
8 quads): every 1x1 tile variant, plain and split-tail launch, at channel counts whose last chunk holds every live count 1..8, against the
oracle twin BIT FOR BIT -- with whole blobs and with channel slices whose neighbouring channels are NaN, so a k-step too many or too few
that reaches them shows.  The Deconvolution form (GEMM + col2im) end to end on the same kernels."""
import numpy as np
import pytest
import torch

import flownet2_amd
import oracle

CINS = (3, 4, 28, 32, 36, 60, 68, 100)                  # 1, 1, 7, 8, 9, 15, 17, 25 live quads: last chunks of 1, 1, 7, 8, 1, 7, 1, 1 k-steps ...
CINS_ALL = CINS + (8, 12, 16, 20, 24)                   # ... and of 2 .. 6 (single-chunk layers): every live count of a last chunk
PLANES = ((8, 12), (5, 12))                             # 96 pixels; 60: a ragged pixel tile, H * W % 4 == 0
COUTS = (32, 64, 128)
N = 2


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def test_channel_counts_cover_every_live_count():
    assert {(-(-c // 4) - 1) % 8 + 1 for c in CINS_ALL} == set(range(1, 9))
    assert {-(-c // 4) for c in CINS} == {1, 7, 8, 9, 15, 17, 25}


@pytest.mark.parametrize("Cin", CINS_ALL)
def test_oracle_twin_against_fp64(Cin):
    """The reference of the GPU tests below is itself a 1x1 convolution: fp32 products accumulated in k order, 2e-6 of the largest value."""
    x, w, b = rnd((N, Cin, 5, 12), 1), rnd((32, Cin, 1, 1), 2, 0.2), rnd((32,), 3)
    got = oracle.conv_mfma_forward(x, oracle.conv_mfma_pack_weights(w), b, 32, 1, 1, 0, True, 0.1)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double())
    want = torch.nn.functional.leaky_relu(y, 0.1).numpy()
    assert np.abs(got - want).max() <= 2e-6 * max(1.0, np.abs(want).max())


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("plane", PLANES)
def test_every_1x1_variant_equals_the_oracle_bitwise(plane, Cout):
    from flownet2_amd import ops
    H, W = plane
    nv = ops.conv_num_variants()
    ran = set()
    try:
        for Cin in CINS_ALL:
            x, w, b = rnd((N, Cin, H, W), 11 + Cin), rnd((Cout, Cin, 1, 1), 12 + Cin, 0.2), rnd((Cout,), 13)
            pw = ops.conv_mfma_pack_weights(torch.from_numpy(w).cuda())
            pwh = pw.cpu().numpy()
            assert np.array_equal(pwh, oracle.conv_mfma_pack_weights(w))            # the packed layout is what it was
            want = torch.from_numpy(oracle.conv_mfma_forward(x, pwh, b, Cout, 1, 1, 0, True, 0.1)).cuda()
            # the same layer as a channel slice [2, 2 + Cin) of a wider bottom whose other channels are NaN, into a slice of a wider top
            xs = np.full((N, Cin + 5, H, W), np.nan, np.float32)
            xs[:, 2:2 + Cin] = x
            want_s = oracle.conv_mfma_forward(xs, pwh, b, Cout, 1, 1, 0, True, 0.1, in_c0=2, Cin=Cin)
            assert np.array_equal(want_s.view(np.uint32), want.cpu().numpy().view(np.uint32))
            xd, xsd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(xs).cuda(), torch.from_numpy(b).cuda()
            for v in list(range(nv)) + [1000 + i for i in range(nv)]:              # plain launches, then the split-tail launches
                ops.set_conv_variant(v)
                try:
                    got = ops.conv_mfma_forward(xd, pw, bd, Cout, 1, 1, 0, True, 0.1)
                except flownet2_amd.Fn2Error:
                    continue                                                          # a variant of another kernel size / channel multiple
                ran.add(v)
                assert torch.equal(bits(got), bits(want)), f"Cin {Cin} variant {v}"
                top = torch.full((N, Cout + 5, H, W), 7.0, device="cuda")
                ops.conv_mfma_forward(xsd, pw, bd, Cout, 1, 1, 0, True, 0.1, out=top, out_c0=3, in_c0=2, Cin=Cin)
                assert torch.equal(bits(top[:, 3:3 + Cout]), bits(want)), f"Cin {Cin} variant {v}, channel slices"
                assert bool((top[:, :3] == 7).all()) and bool((top[:, 3 + Cout:] == 7).all()), f"Cin {Cin} variant {v}: wrote outside its slice"
    finally:
        ops.set_conv_variant(-1)
    plain, tails = {v for v in ran if v < 1000}, {v for v in ran if v >= 1000}
    # 32 channels: only the one-channel-block tiles (MW 2, WM 1) apply -- three 4x4-patch tiles, three row tiles, and the four small row
    # tiles for conv_redir; 64 / 128 channels take the two-block tiles too, which have split-tail launches
    assert len(plain) >= (10 if Cout == 32 else 20), sorted(plain)
    assert Cout == 32 or len(tails) >= 5, sorted(tails)


@pytest.mark.gpu
@pytest.mark.parametrize("Cin", (66, 98))
def test_deconvolution_gemm_route_end_to_end(Cin):
    """fn2_deconv_forward on the GEMM route: weight^T x bottom on the 1x1 tiles (17 / 25 live quads: a last chunk of one k-step), then
    col2im + bias + ReLU, against the same twin plus the oracle's col2im, bit for bit, in the tile the picker takes and in every variant."""
    from flownet2_amd import ops
    Cout, H, W = 8, 6, 8
    x, w, b = rnd((N, Cin, H, W), 21), rnd((Cin, Cout, 4, 4), 22, 0.1), rnd((Cout,), 23)
    desc = ops.conv_desc(N, Cin, H, W, Cout, 4, 2, 1)
    route = ops.DECONV_ROUTE_GEMM
    assert ops.deconv_forward_route(desc) == route
    dv = lambda a: torch.from_numpy(a).cuda()
    packed = ops.conv_pack_weights(dv(w), desc, route, transposed=True)
    col = oracle.conv_mfma_forward(x, packed.cpu().numpy(), None, Cout * 16, 1, 1, 0, relu=False)             # [N, 16 Cout, H, W]: the column matrix
    want = dv(oracle.col2im_bias_relu_forward(col.reshape(N, Cout * 16, H * W), b, N, Cout, 2 * H, 2 * W, 4, 1, 2, True, 0.1))
    got = ops.conv_forward(dv(x), packed, dv(b), desc, route, transposed=True, relu=True, negative_slope=0.1)
    assert torch.equal(bits(got), bits(want))
    ran = 0
    try:
        nv = ops.conv_num_variants()
        for v in list(range(nv)) + [1000 + i for i in range(nv)]:
            ops.set_conv_variant(v)
            try:
                got = ops.conv_forward(dv(x), packed, dv(b), desc, route, transposed=True, relu=True, negative_slope=0.1)
            except flownet2_amd.Fn2Error:
                continue
            ran += 1
            assert torch.equal(bits(got), bits(want)), f"variant {v}"
    finally:
        ops.set_conv_variant(-1)
    assert ran >= 20
