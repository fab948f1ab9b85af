"""The general-geometry Convolution / Deconvolution (csrc/conv_general.hip, include/flownet2_hip_conv_general.h) through the C ABI.

CPU tier: the fourth header is parsed and bound without moving the three older name lists, the constants or the structures; the host-only
answers (supported, sizes) over the row list, FlowNet's classes and the invalid descriptors; the NumPy statement of the packed operand
against fp64.  GPU tier: forward, data gradient, weight and bias gradient of every row against fp64 with the project's bounds (the exact
direct kernel's 4e-6 x scale; the weight gradient's 2e-6 x scale x sqrt(N Ht Wt); the bias gradient's 2e-6 x scale), channel slices, bit
reproducibility, batch independence, the pack kernel against the NumPy statement, and the refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conv_general_cases import (CONV, DECONV, FLOWNET, INVALID, ROWS, case, col_forward, col_transposed, gemm_view, layer64, leaky, out_hw,
                                pack_np, padded_dims, rand, row_id, scale_of, unpack_np)
from flownet2_amd import Fn2Error, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "flownet2_hip_conv_general.h"
NAMES = ["fn2_conv_general_supported", "fn2_debug_set_conv_general_groups", "fn2_conv_general_sizes", "fn2_conv_general_pack_weights", "fn2_conv_general_forward",
         "fn2_conv_general_backward_data", "fn2_conv_general_backward_weights"]
SENTINEL = -7.25
TOL_DIRECT = 4e-6          # TOL[DIRECT] of tests/test_conv_backward_routes.py


def desc_of(row, N=None):
    tr, n, Cin, H, W, Cout, k, s, p = row
    return ops.conv_desc(n if N is None else N, Cin, H, W, Cout, k, s, p)


def dev(a):
    return torch.tensor(a, device="cuda")            # (a copy: the shared reference arrays are read-only)


def ratio(what, row, got, ref, bound):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s %s: error %.3g, bound %.3g, ratio %.3f" % (what, row_id(row), err, bound, err / bound))
    return err / bound


# ------------------------------------------------------------------------------------------------------------------------------ CPU tier
def test_the_fourth_header_is_parsed_and_bound_beside_the_three():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    declared = {name: params.count(",") + 1 for name, params in re.findall(r"\b(fn2_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert list(declared) == NAMES == _lib.CONV_GENERAL_EXPORTS
    L = _lib.lib()
    for name, n in declared.items():
        fn = getattr(L, name)                                   # exported by the built library
        assert fn.restype is C.c_int and len(fn.argtypes) == n, name
        assert (fn.restype, list(fn.argtypes)) == _lib.PROTOTYPES[name]
        assert not name.endswith(("_bytes", "_floats", "_bytes_with_room", "_bytes_arith"))
    assert _lib.PROTOTYPES["fn2_conv_general_sizes"][1] == [C.POINTER(_lib.ConvDesc), C.c_int] + [C.POINTER(C.c_size_t)] * 4
    assert len(_lib.CONSTANTS) == 49 and len(_lib._STRUCTS) == 11
    assert [len(_lib.EXPORTS), len(_lib.SOLVER_EXPORTS), len(_lib.CORR_ROUTE_EXPORTS)] == [159, 3, 2]
    assert not set(NAMES) & (set(_lib.EXPORTS) | set(_lib.SOLVER_EXPORTS) | set(_lib.CORR_ROUTE_EXPORTS))


def test_supported_answers_on_the_host():
    for row in ROWS + FLOWNET:
        assert ops.conv_general_supported(desc_of(row), row[0]), row
    for row in INVALID:
        assert not ops.conv_general_supported(desc_of(row), row[0]), row
        with pytest.raises(Fn2Error) as e:
            ops.conv_general_sizes(desc_of(row), row[0])
        assert e.value.status == _lib.CONSTANTS["FN2_ERR_UNSUPPORTED"]
    # the dispatchers' pins stay: the general kernels sit beside them, not behind their route values
    assert ops.conv_route(2, 64, 16, 24, 96, 5, 2, 2) is None
    assert ops.conv_backward_data_route(ops.conv_desc(2, 40, 9, 12, 33, 3, 2, 2), False) == 0


def wgrad_parts(row):
    """The weight-gradient plan, stated on its own: tiles of 16 k-columns x 64 channels; N x ceil(P / 64) pixel chunks cut into at most 64
    parts, as many as bring the launch to about 2048 workgroups, none empty."""
    tr, N, Cin, H, W, Cout, k, s, p = row
    Ho, Wo = out_hw(row)
    Cs, Cl, Ps = (Cin, Cout, H * W) if tr else (Cout, Cin, Ho * Wo)           # the smaller map's side owns the rows of the weight blob
    G, ksteps = padded_dims(Cs, Cl * k * k)
    chunks = N * -(-Ps // 64)
    want = max(1, min(64, chunks, 2048 // ((ksteps // 4) * -(-G // 4))))
    per_part = -(-chunks // want)
    return -(-chunks // per_part), G, ksteps


@pytest.mark.parametrize("row", ROWS + FLOWNET, ids=row_id)
def test_sizes_equal_the_padded_layout(row):
    tr, N, Cin, H, W, Cout, k, s, p = row
    fwd, dgrad, wgrad, ws = ops.conv_general_sizes(desc_of(row), tr)
    Gf, kf = padded_dims(Cout, Cin * k * k)
    Gd, kd = padded_dims(Cin, Cout * k * k)
    assert (fwd, dgrad, wgrad) == (Gf * kf * 64, Gd * kd * 64, 0)
    parts, G, ksteps = wgrad_parts(row)
    assert ws == 4 * parts * 16 * G * 4 * ksteps


LAYOUTS = {"conv-forward": (False, False), "conv-data-gradient": (False, True), "deconv-forward": (True, False), "deconv-data-gradient": (True, True)}


def layout_case(name):
    """A layer whose operand of this pass is 7 x 27: 7 rows, 3 reduction channels of 3x3 taps."""
    tr, backward = LAYOUTS[name]
    Cin, Cout = (7, 3) if backward else (3, 7)
    return tr, backward, Cin, Cout, rand((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3), 11, 0.1)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_packed_layout_restated_in_numpy_multiplies_to_the_fp64_convolution(name):
    tr, backward, Cin, Cout, w = layout_case(name)
    s, p, H, W = 2, 1, 5, 6
    packed = pack_np(w, tr, backward)
    assert packed.shape == (1, 32 // 4, 64)                          # 7 rows in one group of 16; K = 27 in two chunks of four k-steps
    m = unpack_np(packed, 7, 27)                                     # the zero padding is where it belongs ...
    assert np.array_equal(m, gemm_view(w, tr, backward))
    r, tap = 1, 5                                                    # ... and the tap order: row 2, reduction channel 1, tap (ky 1, kx 2)
    assert m[2, r * 9 + tap] == (w[r, 2, 1, 2] if backward != tr else w[2, r, 1, 2])
    assert packed[0, (r * 9 + tap) // 4, 16 * ((r * 9 + tap) % 4) + 2] == m[2, r * 9 + tap]
    x = torch.from_numpy(rand((1, Cin, H, W), 12)).double().requires_grad_(True)
    top = layer64(x, torch.from_numpy(w).double(), None, tr, s, p)
    Ho, Wo = top.shape[2:]
    if not backward:
        ref, inp, OH, OW = top.detach().numpy()[0], x.detach().numpy()[0], Ho, Wo
    else:
        g = torch.from_numpy(rand(tuple(top.shape), 13)).double()
        ref, inp, OH, OW = torch.autograd.grad(top, x, g)[0].numpy()[0], g.numpy()[0], H, W
    col = (col_transposed if backward != tr else col_forward)(inp, 3, s, p, OH, OW)
    got = (m.astype(np.float64) @ col).reshape(7, OH, OW)
    assert np.abs(got - ref).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------------ GPU tier
def run_forward(row, c, bias=True, relu=False, slope=0.0, N=None, x=None):
    tr = row[0]
    desc = desc_of(row, N)
    packed = ops.conv_general_pack_weights(dev(c["w"]), desc, tr)
    return ops.conv_general_forward(dev(c["x"] if x is None else x), packed, dev(c["b"]) if bias else None, desc, tr, relu=relu, negative_slope=slope)


def run_dgrad(row, c, N=None, g=None):
    tr = row[0]
    desc = desc_of(row, N)
    packed = ops.conv_general_pack_weights(dev(c["w"]), desc, tr, backward=True)
    return ops.conv_general_backward_data(dev(c["g"] if g is None else g), packed, desc, tr)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_forward_matches_fp64(row):
    c = case(row)
    worst = 0.0
    for bias, relu, slope in ((True, True, 0.1), (False, False, 0.0), (True, True, 0.0)):
        ref = c["top"] if bias else c["top_nobias"]
        ref = leaky(ref, slope) if relu else ref
        got = run_forward(row, c, bias, relu, slope).cpu().numpy()
        assert got.shape == ref.shape
        worst = max(worst, ratio("forward bias=%d relu=%d slope=%g" % (bias, relu, slope), row, got, ref, TOL_DIRECT * scale_of(ref)))
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_data_gradient_matches_fp64(row):
    c = case(row)
    got = run_dgrad(row, c).cpu().numpy()
    assert got.shape == c["gx"].shape
    assert ratio("data gradient", row, got, c["gx"], TOL_DIRECT * scale_of(c["gx"])) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_weight_and_bias_gradient_match_fp64_with_and_without_accumulate(row):
    c = case(row)
    tr, N = row[0], row[1]
    Ho, Wo = out_hw(row)
    desc = desc_of(row)
    w0, b0 = rand(c["w"].shape, 21), rand(c["b"].shape, 22)          # non-zero diffs to start from
    for accumulate in (False, True):
        dw, db = dev(w0), dev(b0)
        ops.conv_general_backward_weights(dev(c["x"]), dev(c["g"]), desc, tr, weight_diff=dw, bias_diff=db, accumulate=accumulate)
        rw = c["gw"] + (w0.astype(np.float64) if accumulate else 0.0)
        rb = c["gb"] + (b0.astype(np.float64) if accumulate else 0.0)
        assert ratio("weight gradient accumulate=%d" % accumulate, row, dw.cpu().numpy(), rw, 2e-6 * scale_of(rw) * math.sqrt(N * Ho * Wo)) <= 1.0
        assert ratio("bias gradient accumulate=%d" % accumulate, row, db.cpu().numpy(), rb, 2e-6 * scale_of(rb)) <= 1.0
    dw, none = ops.conv_general_backward_weights(dev(c["x"]), dev(c["g"]), desc, tr, bias=False)          # no bias blob: the weight diff alone
    assert none is None and ratio("weight gradient alone", row, dw.cpu().numpy(), c["gw"], 2e-6 * scale_of(c["gw"]) * math.sqrt(N * Ho * Wo)) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pack_kernel_writes_the_restated_layout(name):
    tr, backward, Cin, Cout, w = layout_case(name)
    got = ops.conv_general_pack_weights(dev(w), ops.conv_desc(1, Cin, 5, 6, Cout, 3, 2, 1), tr, backward=backward).cpu().numpy()
    assert np.array_equal(got, pack_np(w, tr, backward).ravel())


@pytest.mark.gpu
@pytest.mark.parametrize("row", [ROWS[2], ROWS[10]], ids=row_id)
def test_channel_slices_of_odd_sized_blobs(row):
    """Bottom read from the middle of a wider blob, top written into the middle of a wider sentinel-filled one: nothing outside the slice
    moves, the bits inside equal the whole-blob run.  The planes (9x12 and 4x5 / 4x6 / ...) and the offsets are not multiples of four."""
    c = case(row)
    tr, N, Cin, H, W, Cout, k, s, p = row
    Ho, Wo = out_hw(row)
    desc = desc_of(row)

    def wide(a, c0, extra):
        blob = np.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], SENTINEL, np.float32)
        blob[:, c0:c0 + a.shape[1]] = a
        return dev(blob)

    def outside_untouched(blob, c0, Cc):
        b = blob.cpu().numpy()
        return (b[:, :c0] == SENTINEL).all() and (b[:, c0 + Cc:] == SENTINEL).all()

    # forward
    whole = run_forward(row, c, True, True, 0.1)
    packed = ops.conv_general_pack_weights(dev(c["w"]), desc, tr)
    top = torch.full((N, Cout + 5, Ho, Wo), SENTINEL, device="cuda")
    ops.conv_general_forward(wide(c["x"], 3, 4), packed, dev(c["b"]), desc, tr, relu=True, negative_slope=0.1, out=top, out_c0=2, in_c0=3)
    assert outside_untouched(top, 2, Cout) and torch.equal(top[:, 2:2 + Cout], whole)
    # data gradient
    whole = run_dgrad(row, c)
    packed = ops.conv_general_pack_weights(dev(c["w"]), desc, tr, backward=True)
    bd = torch.full((N, Cin + 3, H, W), SENTINEL, device="cuda")
    ops.conv_general_backward_data(wide(c["g"], 1, 2), packed, desc, tr, top_c0=1, out=bd, out_c0=2)
    assert outside_untouched(bd, 2, Cin) and torch.equal(bd[:, 2:2 + Cin], whole)
    # weight and bias gradient read slices of both blobs
    dw, db = ops.conv_general_backward_weights(dev(c["x"]), dev(c["g"]), desc, tr)
    dw2, db2 = ops.conv_general_backward_weights(wide(c["x"], 3, 4), wide(c["g"], 1, 2), desc, tr, bottom_c0=3, top_c0=1)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_a_sample_does_not_see_its_batch():
    row = ROWS[2]                                                     # three samples
    c = case(row)
    tr = row[0]
    f1, f2, d1, d2 = run_forward(row, c, True, True, 0.1), run_forward(row, c, True, True, 0.1), run_dgrad(row, c), run_dgrad(row, c)
    assert torch.equal(f1, f2) and torch.equal(d1, d2)
    w1 = ops.conv_general_backward_weights(dev(c["x"]), dev(c["g"]), desc_of(row), tr)
    w2 = ops.conv_general_backward_weights(dev(c["x"]), dev(c["g"]), desc_of(row), tr)
    assert torch.equal(w1[0], w2[0]) and torch.equal(w1[1], w2[1])
    for n in range(row[1]):
        assert torch.equal(run_forward(row, c, True, True, 0.1, N=1, x=c["x"][n:n + 1])[0], f1[n])
        assert torch.equal(run_dgrad(row, c, N=1, g=c["g"][n:n + 1])[0], d1[n])
    row = ROWS[13]                                                    # and a deconvolution, run twice
    c = case(row)
    assert torch.equal(run_forward(row, c), run_forward(row, c)) and torch.equal(run_dgrad(row, c), run_dgrad(row, c))


@pytest.mark.gpu
@pytest.mark.parametrize("row", [ROWS[1], ROWS[2], ROWS[6], ROWS[13]], ids=row_id)
def test_every_channel_group_variant_gives_the_same_bits(row):
    """The gather kernels exist with 1, 2 and 4 groups of 16 output channels per workgroup (picked by the channel count alone); forced one
    after the other they write the same bits, forward and data gradient, on 7, 33, 96 and 5 output channels."""
    c = case(row)
    try:
        got = []
        for groups in (0, 1, 2, 4):
            ops.set_conv_general_groups(groups)
            got.append((run_forward(row, c, True, True, 0.1), run_dgrad(row, c)))
    finally:
        ops.set_conv_general_groups(0)
    assert all(torch.equal(f, got[0][0]) and torch.equal(d, got[0][1]) for f, d in got[1:])
    with pytest.raises(Fn2Error):
        ops.set_conv_general_groups(3)


@pytest.mark.gpu
def test_supported_sizes_and_the_launches_refuse_the_same_descriptors():
    L = _lib.lib()
    UNSUPPORTED, INVALID_ARG, WORKSPACE = (_lib.CONSTANTS["FN2_ERR_" + n] for n in ("UNSUPPORTED", "INVALID_ARG", "WORKSPACE"))
    buf = torch.zeros(1 << 16, device="cuda")
    ptr, null, st = C.c_void_p(buf.data_ptr()), C.c_void_p(0), C.c_void_p(0)

    def launches(desc, tr, bottom=ptr, top=ptr, weight=ptr, ws=ptr, ws_bytes=4 << 16):
        d = C.byref(desc)
        return [L.fn2_conv_general_pack_weights(d, tr, 0, weight, ptr, st),
                L.fn2_conv_general_forward(d, tr, bottom, desc.Cin, 0, weight, null, top, desc.Cout, 0, 0, C.c_float(0), st),
                L.fn2_conv_general_backward_data(d, tr, top, desc.Cout, 0, weight, bottom, desc.Cin, 0, st),
                L.fn2_conv_general_backward_weights(d, tr, bottom, desc.Cin, 0, top, desc.Cout, 0, weight, null, 0, ws, ws_bytes, st)]

    for row in (INVALID[0], INVALID[1], INVALID[2]):                  # empty output of a convolution, of a deconvolution; kernel = 0
        desc, tr = desc_of(row), int(row[0])
        assert L.fn2_conv_general_supported(C.byref(desc), tr) == 0
        assert L.fn2_conv_general_sizes(C.byref(desc), tr, None, None, None, None) == UNSUPPORTED
        assert launches(desc, tr) == [UNSUPPORTED] * 4
        assert "no kernel for" in L.fn2_last_error_string().decode()
    row = ROWS[1]
    desc, tr = desc_of(row), 0
    assert launches(desc, tr, bottom=null) == [0, INVALID_ARG, INVALID_ARG, INVALID_ARG]
    assert launches(desc, tr, top=null)[1:] == [INVALID_ARG] * 3
    assert launches(desc, tr, weight=null) == [INVALID_ARG] * 4
    assert launches(desc, tr, ws=null)[3] == WORKSPACE and launches(desc, tr, ws_bytes=16)[3] == WORKSPACE
    assert L.fn2_conv_general_pack_weights(C.byref(desc), tr, 3, ptr, ptr, st) == INVALID_ARG
    assert L.fn2_conv_general_forward(C.byref(desc), tr, ptr, desc.Cin, 1, ptr, null, ptr, desc.Cout, 0, 0, C.c_float(0), st) == INVALID_ARG     # slice outside
    torch.cuda.synchronize()
