"""The general convolution with rectangular taps, per-axis stride / pad / dilation and groups (csrc/conv_general.hip widened,
include/flownet2_hip_conv_geometry.h) through the C ABI.

CPU tier: the fifth header is parsed and bound beside the four without moving their name lists, the constants or the structures; the
host-only answers (supported, out_shape, sizes) over the row list and the invalid geometries; the NumPy statement of the packed operand per
group and of the two gathers against fp64.  GPU tier: forward, data gradient, weight and bias gradient of every row against fp64 with the
bounds of tests/test_conv_general.py (4e-6 x scale; the weight gradient's 2e-6 x scale x sqrt(N Ht Wt); the bias gradient's 2e-6 x scale:
group and dilation only shorten K, so they stand as derived), channel slices on a grouped row, bit reproducibility, batch independence, the
three row-group instantiations, bit identity with fn2_conv_general_* on square rows, the pack kernel against NumPy, and the refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import conv_general_cases as sq
from conv_geometry_cases import (CONV, DECONV, INVALID, ROWS, case, col_forward, col_transposed, gemm_views, layer64, out_hw, pack_np, padded_dims,
                                 row_id, unpack_np, weight_shape)
from conv_general_cases import leaky, rand, scale_of
from flownet2_amd import Fn2Error, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "flownet2_hip_conv_geometry.h"
NAMES = ["fn2_conv_geometry_supported", "fn2_conv_geometry_out_shape", "fn2_conv_geometry_sizes", "fn2_conv_geometry_pack_weights",
         "fn2_conv_geometry_forward", "fn2_conv_geometry_backward_data", "fn2_conv_geometry_backward_weights"]
SENTINEL = -7.25
TOL_DIRECT = 4e-6
GROUPED = ROWS[5]               # conv, group 2, 5 rows per group


def geom_of(row, N=None):
    tr, n, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group = row
    return ops.conv_geometry(n if N is None else N, Cin, H, W, Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), group)


def square_as_geometry(row):
    tr, N, Cin, H, W, Cout, k, s, p = row
    return (tr, N, Cin, H, W, Cout, k, k, s, s, p, p, 1, 1, 1)


def dev(a):
    return torch.tensor(a, device="cuda")            # (a copy: the shared reference arrays are read-only)


def ratio(what, row, got, ref, bound):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s %s: error %.3g, bound %.3g, ratio %.3f" % (what, row_id(row), err, bound, err / bound))
    return err / bound


# ------------------------------------------------------------------------------------------------------------------------------ CPU tier
def test_the_fifth_header_is_parsed_and_bound_beside_the_four():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    assert "FN2_" not in re.sub(r"^\s*#.*$", " ", text, flags=re.M) and "typedef" not in text and "enum" not in text
    declared = {name: params.count(",") + 1 for name, params in re.findall(r"\b(fn2_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert list(declared) == NAMES == _lib.CONV_GEOMETRY_EXPORTS
    L = _lib.lib()
    for name, n in declared.items():
        fn = getattr(L, name)                                   # exported by the built library
        assert fn.restype is C.c_int and len(fn.argtypes) == n, name
        assert (fn.restype, list(fn.argtypes)) == _lib.PROTOTYPES[name]
    assert _lib.PROTOTYPES["fn2_conv_geometry_sizes"][1] == [C.POINTER(C.c_int), C.c_int] + [C.POINTER(C.c_size_t)] * 4
    assert _lib.PROTOTYPES["fn2_conv_geometry_out_shape"][1] == [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    # same argument lists after the descriptor as the fourth header's
    for tail in ("pack_weights", "forward", "backward_data", "backward_weights", "sizes", "supported"):
        assert _lib.PROTOTYPES["fn2_conv_geometry_" + tail][1][1:] == _lib.PROTOTYPES["fn2_conv_general_" + tail][1][1:], tail
    assert len(_lib.CONSTANTS) == 49 and len(_lib._STRUCTS) == 11
    assert [len(_lib.EXPORTS), len(_lib.SOLVER_EXPORTS), len(_lib.CORR_ROUTE_EXPORTS), len(_lib.CONV_GENERAL_EXPORTS)] == [159, 3, 2, 7]
    assert not set(NAMES) & (set(_lib.EXPORTS) | set(_lib.SOLVER_EXPORTS) | set(_lib.CORR_ROUTE_EXPORTS) | set(_lib.CONV_GENERAL_EXPORTS))


def test_supported_and_out_shape_answer_on_the_host():
    for row in ROWS:
        assert ops.conv_geometry_supported(geom_of(row), row[0]), row
        assert ops.conv_geometry_out_shape(geom_of(row), row[0]) == out_hw(row), row
    for row in INVALID:
        assert not ops.conv_geometry_supported(geom_of(row), row[0]), row
        for call in (ops.conv_geometry_sizes, ops.conv_geometry_out_shape):
            with pytest.raises(Fn2Error) as e:
                call(geom_of(row), row[0])
            assert e.value.status == _lib.CONSTANTS["FN2_ERR_UNSUPPORTED"]
    L = _lib.lib()
    assert L.fn2_conv_geometry_supported(None, 0) == 0
    assert L.fn2_conv_geometry_sizes(None, 0, None, None, None, None) == _lib.CONSTANTS["FN2_ERR_UNSUPPORTED"]


def wgrad_parts(row):
    """The weight-gradient plan, stated on its own: tiles of 16 k-columns x 64 channels inside one group; N x ceil(P / 64) pixel chunks cut
    into at most 64 parts, as many as bring the launch to about 2048 workgroups, none empty."""
    tr, N, Cin, H, W, Cout, kh, kw = row[:8]
    group = row[14]
    Ho, Wo = out_hw(row)
    Cs, Cl, Ps = (Cin, Cout, H * W) if tr else (Cout, Cin, Ho * Wo)           # the smaller map's side owns the rows of the weight blob
    G, ksteps = padded_dims(Cs // group, (Cl // group) * kh * kw)
    chunks = N * -(-Ps // 64)
    want = max(1, min(64, chunks, 2048 // ((ksteps // 4) * -(-G // 4) * group)))
    per_part = -(-chunks // want)
    return -(-chunks // per_part), G, ksteps


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_sizes_equal_the_padded_layout_per_group(row):
    tr, N, Cin, H, W, Cout, kh, kw = row[:8]
    group = row[14]
    fwd, dgrad, wgrad, ws = ops.conv_geometry_sizes(geom_of(row), tr)
    Gf, kf = padded_dims(Cout // group, (Cin // group) * kh * kw)
    Gd, kd = padded_dims(Cin // group, (Cout // group) * kh * kw)
    assert (fwd, dgrad, wgrad) == (group * Gf * kf * 64, group * Gd * kd * 64, 0)
    parts, G, ksteps = wgrad_parts(row)
    assert ws == 4 * parts * group * 16 * G * 4 * ksteps


@pytest.mark.parametrize("row", sq.ROWS + sq.FLOWNET, ids=sq.row_id)
def test_sizes_of_a_square_geometry_equal_the_general_sizes(row):
    tr, N, Cin, H, W, Cout, k, s, p = row
    assert ops.conv_geometry_sizes(geom_of(square_as_geometry(row)), tr) == ops.conv_general_sizes(ops.conv_desc(N, Cin, H, W, Cout, k, s, p), tr)
    assert ops.conv_geometry_out_shape(geom_of(square_as_geometry(row)), tr) == sq.out_hw(row)


# one small layer per pass and kind: rectangular taps 3 x 2, stride (2, 1), pad (1, 0), dilation (1, 2), group 2; 3 -> 5 channels per group
LAYOUTS = {"conv-forward": (False, False), "conv-data-gradient": (False, True), "deconv-forward": (True, False), "deconv-data-gradient": (True, True)}
LAYOUT_GEOM = dict(kh=3, kw=2, sh=2, sw=1, ph=1, pw=0, dh=1, dw=2, group=2)


def layout_case(name):
    """A layer whose operand of this pass is, per group, 5 x 18: 5 rows, 3 reduction channels of 3x2 taps."""
    tr, backward = LAYOUTS[name]
    Cin, Cout = (10, 6) if backward else (6, 10)
    g = LAYOUT_GEOM
    row = (tr, 1, Cin, 5, 6, Cout, g["kh"], g["kw"], g["sh"], g["sw"], g["ph"], g["pw"], g["dh"], g["dw"], g["group"])
    return row, backward, rand(weight_shape(row), 11, 0.1)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_packed_layout_per_group_restated_in_numpy_multiplies_to_the_fp64_convolution(name):
    row, backward, w = layout_case(name)
    tr, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group = row
    packed = pack_np(w, tr, backward, group)
    assert packed.shape == (2, 1, 32 // 4, 64)                       # two groups; 5 rows in one row group; K = 18 in two chunks of four k-steps
    views = gemm_views(w, tr, backward, group)
    for g in range(group):
        assert np.array_equal(unpack_np(packed[g], 5, 18), views[g])  # the zero padding is where it belongs
    # the tap order: group 1, row 2, reduction channel 1, tap (ky 2, kx 1) = 2 kw + 1
    r, tap = 1, 2 * kw + 1
    swapped = backward != tr
    blob = w[3 + r, 2, 2, 1] if swapped else w[5 + 2, r, 2, 1]       # swapped: blob rows are the reduction channels (3 per group)
    assert views[1][2, r * kh * kw + tap] == blob
    assert packed[1, 0, (r * 6 + tap) // 4, 16 * ((r * 6 + tap) % 4) + 2] == blob
    x = torch.from_numpy(rand((1, Cin, H, W), 12)).double().requires_grad_(True)
    top = layer64(x, torch.from_numpy(w).double(), None, row)
    Ho, Wo = top.shape[2:]
    assert (Ho, Wo) == out_hw(row)
    if not backward:
        ref, inp, OH, OW = top.detach().numpy()[0], x.detach().numpy()[0], Ho, Wo
    else:
        gt = torch.from_numpy(rand(tuple(top.shape), 13)).double()
        ref, inp, OH, OW = torch.autograd.grad(top, x, gt)[0].numpy()[0], gt.numpy()[0], H, W
    rg = inp.shape[0] // group                                        # reduction channels per group
    for g in range(group):
        col = (col_transposed if swapped else col_forward)(inp[g * rg:(g + 1) * rg], kh, kw, sh, sw, ph, pw, dh, dw, OH, OW)
        got = (views[g].astype(np.float64) @ col).reshape(5, OH, OW)
        assert np.abs(got - ref[5 * g:5 * g + 5]).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------------ GPU tier
def run_forward(row, c, bias=True, relu=False, slope=0.0, N=None, x=None):
    tr = row[0]
    geom = geom_of(row, N)
    packed = ops.conv_geometry_pack_weights(dev(c["w"]), geom, tr)
    return ops.conv_geometry_forward(dev(c["x"] if x is None else x), packed, dev(c["b"]) if bias else None, geom, tr, relu=relu, negative_slope=slope)


def run_dgrad(row, c, N=None, g=None):
    tr = row[0]
    geom = geom_of(row, N)
    packed = ops.conv_geometry_pack_weights(dev(c["w"]), geom, tr, backward=True)
    return ops.conv_geometry_backward_data(dev(c["g"] if g is None else g), packed, geom, tr)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_forward_matches_fp64(row):
    c = case(row)
    worst = 0.0
    for bias, relu, slope in ((True, False, 0.0), (False, False, 0.0), (True, True, 0.1)):
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
    geom = geom_of(row)
    w0, b0 = rand(c["w"].shape, 21), rand(c["b"].shape, 22)          # non-zero diffs to start from
    for accumulate in (False, True):
        dw, db = dev(w0), dev(b0)
        ops.conv_geometry_backward_weights(dev(c["x"]), dev(c["g"]), geom, tr, weight_diff=dw, bias_diff=db, accumulate=accumulate)
        rw = c["gw"] + (w0.astype(np.float64) if accumulate else 0.0)
        rb = c["gb"] + (b0.astype(np.float64) if accumulate else 0.0)
        assert ratio("weight gradient accumulate=%d" % accumulate, row, dw.cpu().numpy(), rw, 2e-6 * scale_of(rw) * math.sqrt(N * Ho * Wo)) <= 1.0
        assert ratio("bias gradient accumulate=%d" % accumulate, row, db.cpu().numpy(), rb, 2e-6 * scale_of(rb)) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pack_kernel_writes_the_restated_layout(name):
    row, backward, w = layout_case(name)
    got = ops.conv_geometry_pack_weights(dev(w), geom_of(row), row[0], backward=backward).cpu().numpy()
    assert np.array_equal(got, pack_np(w, row[0], backward, row[14]).ravel())


@pytest.mark.gpu
@pytest.mark.parametrize("row", [GROUPED, ROWS[13]], ids=row_id)
def test_channel_slices_on_a_grouped_row(row):
    """Bottom read from the middle of a wider blob, top written into the middle of a wider sentinel-filled one, on layers with groups: the
    group offsets add to the caller's c0; nothing outside the slice (other channels, and so the memory beyond the map of the last written
    channel) moves, the bits inside equal the whole-blob run."""
    c = case(row)
    tr, N, Cin, H, W, Cout = row[:6]
    Ho, Wo = out_hw(row)
    geom = geom_of(row)

    def wide(a, c0, extra):
        blob = np.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], SENTINEL, np.float32)
        blob[:, c0:c0 + a.shape[1]] = a
        return dev(blob)

    def outside_untouched(blob, c0, Cc):
        b = blob.cpu().numpy()
        return (b[:, :c0] == SENTINEL).all() and (b[:, c0 + Cc:] == SENTINEL).all()

    whole = run_forward(row, c, True, True, 0.1)
    packed = ops.conv_geometry_pack_weights(dev(c["w"]), geom, tr)
    top = torch.full((N, Cout + 5, Ho, Wo), SENTINEL, device="cuda")
    ops.conv_geometry_forward(wide(c["x"], 3, 4), packed, dev(c["b"]), geom, tr, relu=True, negative_slope=0.1, out=top, out_c0=2, in_c0=3)
    assert outside_untouched(top, 2, Cout) and torch.equal(top[:, 2:2 + Cout], whole)
    whole = run_dgrad(row, c)
    packed = ops.conv_geometry_pack_weights(dev(c["w"]), geom, tr, backward=True)
    bd = torch.full((N, Cin + 3, H, W), SENTINEL, device="cuda")
    ops.conv_geometry_backward_data(wide(c["g"], 1, 2), packed, geom, tr, top_c0=1, out=bd, out_c0=2)
    assert outside_untouched(bd, 2, Cin) and torch.equal(bd[:, 2:2 + Cin], whole)
    dw, db = ops.conv_geometry_backward_weights(dev(c["x"]), dev(c["g"]), geom, tr)
    dw2, db2 = ops.conv_geometry_backward_weights(wide(c["x"], 3, 4), wide(c["g"], 1, 2), geom, tr, bottom_c0=3, top_c0=1)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_a_sample_does_not_see_its_batch():
    for row in (ROWS[9], ROWS[13]):                                   # "everything at once" and the grouped deconvolution: N = 2 both
        c = case(row)
        tr = row[0]
        f1, f2, d1, d2 = run_forward(row, c, True, True, 0.1), run_forward(row, c, True, True, 0.1), run_dgrad(row, c), run_dgrad(row, c)
        assert torch.equal(f1, f2) and torch.equal(d1, d2)
        w1 = ops.conv_geometry_backward_weights(dev(c["x"]), dev(c["g"]), geom_of(row), tr)
        w2 = ops.conv_geometry_backward_weights(dev(c["x"]), dev(c["g"]), geom_of(row), tr)
        assert torch.equal(w1[0], w2[0]) and torch.equal(w1[1], w2[1])
        n = 1                                                         # sample 1 of the N = 2 run equals the N = 1 run of that sample
        assert torch.equal(run_forward(row, c, True, True, 0.1, N=1, x=c["x"][n:n + 1])[0], f1[n])
        assert torch.equal(run_dgrad(row, c, N=1, g=c["g"][n:n + 1])[0], d1[n])


@pytest.mark.gpu
@pytest.mark.parametrize("row", [ROWS[1], ROWS[6], ROWS[9], ROWS[14]], ids=row_id)
def test_every_row_group_variant_gives_the_same_bits(row):
    """The gather kernels exist with 1, 2 and 4 row groups of 16 output channels per workgroup; forced one after the other they write the
    same bits, forward and data gradient, with rectangular taps (18 rows), groups of 20 rows, everything at once, and a grouped deconvolution."""
    c = case(row)
    try:
        got = []
        for groups in (0, 1, 2, 4):
            ops.set_conv_general_groups(groups)
            got.append((run_forward(row, c, True, True, 0.1), run_dgrad(row, c)))
    finally:
        ops.set_conv_general_groups(0)
    assert all(torch.equal(f, got[0][0]) and torch.equal(d, got[0][1]) for f, d in got[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("row", [sq.ROWS[1], sq.ROWS[2], sq.ROWS[10], sq.ROWS[13]], ids=sq.row_id)
def test_a_square_geometry_gives_the_bits_of_the_general_entry_points(row):
    """Rows of tests/conv_general_cases.py through fn2_conv_geometry_* with (k, k, s, s, p, p, 1, 1, 1): the packed operands and the results
    of all three passes are bit-identical to fn2_conv_general_*."""
    tr, N, Cin, H, W, Cout, k, s, p = row
    c = sq.case(row)
    desc, geom = ops.conv_desc(N, Cin, H, W, Cout, k, s, p), geom_of(square_as_geometry(row))
    x, w, b, g = dev(c["x"]), dev(c["w"]), dev(c["b"]), dev(c["g"])
    for backward in (False, True):
        pg, pq = ops.conv_geometry_pack_weights(w, geom, tr, backward=backward), ops.conv_general_pack_weights(w, desc, tr, backward=backward)
        assert torch.equal(pg, pq)
        if backward:
            assert torch.equal(ops.conv_geometry_backward_data(g, pg, geom, tr), ops.conv_general_backward_data(g, pq, desc, tr))
        else:
            assert torch.equal(ops.conv_geometry_forward(x, pg, b, geom, tr, relu=True, negative_slope=0.1),
                               ops.conv_general_forward(x, pq, b, desc, tr, relu=True, negative_slope=0.1))
    wg, wq = ops.conv_geometry_backward_weights(x, g, geom, tr), ops.conv_general_backward_weights(x, g, desc, tr)
    assert torch.equal(wg[0], wq[0]) and torch.equal(wg[1], wq[1])


@pytest.mark.gpu
def test_supported_sizes_and_the_launches_refuse_the_same_geometries():
    L = _lib.lib()
    UNSUPPORTED, INVALID_ARG, WORKSPACE = (_lib.CONSTANTS["FN2_ERR_" + n] for n in ("UNSUPPORTED", "INVALID_ARG", "WORKSPACE"))
    buf = torch.full((1 << 16,), SENTINEL, device="cuda")
    ptr, null, st = C.c_void_p(buf.data_ptr()), C.c_void_p(0), C.c_void_p(0)

    def launches(geom, tr, bottom=ptr, top=ptr, weight=ptr, ws=ptr, ws_bytes=4 << 16, bottom_c0=0, top_channels=None):
        Cin, Cout = geom[1], geom[4]
        tc = Cout if top_channels is None else top_channels
        return [L.fn2_conv_geometry_pack_weights(geom, tr, 0, weight, ptr, st),
                L.fn2_conv_geometry_forward(geom, tr, bottom, Cin, bottom_c0, weight, null, top, tc, 0, 0, C.c_float(0), st),
                L.fn2_conv_geometry_backward_data(geom, tr, top, tc, 0, weight, bottom, Cin, bottom_c0, st),
                L.fn2_conv_geometry_backward_weights(geom, tr, bottom, Cin, bottom_c0, top, tc, 0, weight, null, 0, ws, ws_bytes, st)]

    for row in INVALID:
        geom, tr = geom_of(row), int(row[0])
        assert L.fn2_conv_geometry_supported(geom, tr) == 0
        assert L.fn2_conv_geometry_sizes(geom, tr, None, None, None, None) == UNSUPPORTED
        assert launches(geom, tr) == [UNSUPPORTED] * 4
        assert "no kernel for" in L.fn2_last_error_string().decode()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                              # refused on the host: nothing was launched, nothing written
    geom, tr = geom_of(GROUPED), 0
    assert launches(geom, tr, bottom=null) == [0, INVALID_ARG, INVALID_ARG, INVALID_ARG]
    assert launches(geom, tr, top=null)[1:] == [INVALID_ARG] * 3
    assert launches(geom, tr, weight=null) == [INVALID_ARG] * 4
    assert launches(geom, tr, bottom_c0=1)[1:] == [INVALID_ARG] * 3                  # a slice outside its blob, bottom side
    assert launches(geom, tr, top_channels=geom[4] - 1)[1:] == [INVALID_ARG] * 3     # and top side
    assert launches(geom, tr, ws=null)[3] == WORKSPACE and launches(geom, tr, ws_bytes=16)[3] == WORKSPACE
    assert L.fn2_conv_geometry_pack_weights(geom, tr, 3, ptr, ptr, st) == INVALID_ARG
    torch.cuda.synchronize()
    # the valid calls among these (a pack; with a bad workspace alone the pack, forward and data gradient) write the layer's blobs at the
    # start of the buffer, 1120 floats at the most; the refused ones wrote nothing beyond
    assert max(ops.conv_geometry_sizes(geom, tr)[0], 2 * 10 * 7 * 8) <= 2048 and bool((buf[2048:] == SENTINEL).all())
