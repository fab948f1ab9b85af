"""The general convolution over 0 to 3 spatial axes (the depth tier of csrc/conv_general.hip, include/flownet2_hip_conv_volume.h) through the
C ABI.

CPU tier: the sixth header is parsed and bound beside the five without moving their name lists, the constants or the structures; the
host-only answers (supported, out_shape, sizes) over the row list and the invalid geometries; the folding of fewer axes; the NumPy statement
of the packed operand per group and of the two gathers with the depth digit against fp64.  GPU tier: forward, data gradient, weight and bias
gradient of every row against fp64 (torch's double conv3d / conv_transpose3d on the CPU) with the bounds of tests/test_conv_general.py (4e-6 x
scale; the weight gradient's 2e-6 x scale x sqrt(N Dt Ht Wt); the bias gradient's 2e-6 x scale: every K here is below the largest there --
320 against 2400, see tests/conv_volume_cases.py -- so they stand as derived), channel slices on a grouped row, bit reproducibility, batch
independence, the three row-group instantiations, the pack kernel against NumPy, the refusals, and the bit identities with
fn2_conv_geometry_* of a volume whose depth axis is trivial and of a layer over one spatial axis."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import conv_geometry_cases as flat
from conv_general_cases import leaky, rand, scale_of
from conv_geometry_cases import padded_dims, unpack_np
from conv_volume_cases import (GROUPED, INVALID, ROWS, case, col_forward, col_transposed, fields, gemm_views, layer64, out_size, pack_np, row_id,
                               weight_shape)
from flownet2_amd import Fn2Error, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "flownet2_hip_conv_volume.h"
NAMES = ["fn2_conv_volume_supported", "fn2_conv_volume_out_shape", "fn2_conv_volume_sizes", "fn2_conv_volume_pack_weights",
         "fn2_conv_volume_forward", "fn2_conv_volume_backward_data", "fn2_conv_volume_backward_weights"]
SENTINEL = -7.25
TOL_DIRECT = 4e-6


def geom_of(row, N=None):
    tr, n, Cin, size, Cout, kernel, stride, pad, dilation, group = fields(row)
    return ops.conv_volume(n if N is None else N, Cin, size, Cout, kernel, stride, pad, dilation, group)


def dev(a):
    return torch.tensor(a, device="cuda")            # (a copy: the shared reference arrays are read-only)


def ratio(what, row, got, ref, bound):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s %s: error %.3g, bound %.3g, ratio %.3f" % (what, row_id(row), err, bound, err / bound))
    return err / bound


# ------------------------------------------------------------------------------------------------------------------------------ CPU tier
def test_the_sixth_header_is_parsed_and_bound_beside_the_five():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    assert "FN2_" not in re.sub(r"^\s*#.*$", " ", text, flags=re.M) and "typedef" not in text and "enum" not in text
    assert '#include "flownet2_hip.h"' in text
    declared = {name: params.count(",") + 1 for name, params in re.findall(r"\b(fn2_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert list(declared) == NAMES == _lib.CONV_VOLUME_EXPORTS
    L = _lib.lib()
    for name, n in declared.items():
        fn = getattr(L, name)                                   # exported by the built library
        assert fn.restype is C.c_int and len(fn.argtypes) == n, name
        assert (fn.restype, list(fn.argtypes)) == _lib.PROTOTYPES[name]
    assert _lib.PROTOTYPES["fn2_conv_volume_out_shape"][1] == [C.POINTER(C.c_int), C.c_int] + [C.POINTER(C.c_int)] * 3
    # same argument lists after the descriptor as the fifth header's
    for tail in ("pack_weights", "forward", "backward_data", "backward_weights", "sizes", "supported"):
        assert _lib.PROTOTYPES["fn2_conv_volume_" + tail][1] == _lib.PROTOTYPES["fn2_conv_geometry_" + tail][1], tail
    assert len(_lib.CONSTANTS) == 49 and len(_lib._STRUCTS) == 11
    assert [len(_lib.EXPORTS), len(_lib.SOLVER_EXPORTS), len(_lib.CORR_ROUTE_EXPORTS), len(_lib.CONV_GENERAL_EXPORTS),
            len(_lib.CONV_GEOMETRY_EXPORTS)] == [159, 3, 2, 7, 7]
    others = set(_lib.EXPORTS) | set(_lib.SOLVER_EXPORTS) | set(_lib.CORR_ROUTE_EXPORTS) | set(_lib.CONV_GENERAL_EXPORTS) | set(_lib.CONV_GEOMETRY_EXPORTS)
    assert not set(NAMES) & others


def test_supported_and_out_shape_answer_on_the_host():
    for row in ROWS:
        assert ops.conv_volume_supported(geom_of(row), row[0]), row
        assert ops.conv_volume_out_shape(geom_of(row), row[0]) == out_size(row), row
    for row in INVALID:
        assert not ops.conv_volume_supported(geom_of(row), row[0]), row
        for call in (ops.conv_volume_sizes, ops.conv_volume_out_shape):
            with pytest.raises(Fn2Error) as e:
                call(geom_of(row), row[0])
            assert e.value.status == _lib.CONSTANTS["FN2_ERR_UNSUPPORTED"]
            assert "no kernel for" in str(e.value) and "x".join(str(v) for v in row[3:6]) in str(e.value)      # the refusal names all three extents
    L = _lib.lib()
    assert L.fn2_conv_volume_supported(None, 0) == 0
    assert L.fn2_conv_volume_sizes(None, 0, None, None, None, None) == _lib.CONSTANTS["FN2_ERR_UNSUPPORTED"]
    assert L.fn2_conv_volume_out_shape(None, 1, None, None, None) == _lib.CONSTANTS["FN2_ERR_UNSUPPORTED"]
    d = C.c_int(-1)
    assert L.fn2_conv_volume_out_shape(geom_of(ROWS[7]), 0, C.byref(d), None, None) == 0 and d.value == 1       # Din + 2 pd == ext: one plane


def test_fewer_axes_fold_onto_the_trailing_ones_and_four_are_refused_by_name():
    assert list(ops.conv_volume(2, 3, (4, 5, 6), 7, (1, 2, 3), (4, 5, 6), (7, 8, 9), (1, 2, 1), 1)) == [2, 3, 4, 5, 6, 7, 1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 2, 1, 1]
    assert list(ops.conv_volume(2, 3, (5, 6), 7, (2, 3), 2, (1, 0), 1, 1)) == [2, 3, 1, 5, 6, 7, 1, 2, 3, 1, 2, 2, 0, 1, 0, 1, 1, 1, 1]
    assert list(ops.conv_volume(2, 4, (9,), 6, 3, 2, 1, 2, 2)) == [2, 4, 1, 1, 9, 6, 1, 1, 3, 1, 1, 2, 0, 0, 1, 1, 1, 2, 2]
    assert list(ops.conv_volume(2, 4, (), 6, 1)) == [2, 4, 1, 1, 1, 6, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    # the host answers of a folded geometry are those of the 2-D layer
    for tr in (False, True):
        assert ops.conv_volume_sizes(ops.conv_volume(2, 4, (9,), 6, 3, 2, 1, 2, 2), tr) == \
            ops.conv_geometry_sizes(ops.conv_geometry(2, 4, 1, 9, 6, (1, 3), (1, 2), (0, 1), (1, 2), 2), tr)
        assert ops.conv_volume_out_shape(ops.conv_volume(2, 4, (9,), 6, 3, 2, 1, 2, 2), tr)[1:] == \
            ops.conv_geometry_out_shape(ops.conv_geometry(2, 4, 1, 9, 6, (1, 3), (1, 2), (0, 1), (1, 2), 2), tr)
    with pytest.raises(ValueError, match="4 spatial axes"):
        ops.conv_volume(1, 2, (3, 3, 3, 3), 2, 1)
    with pytest.raises(ValueError, match="one per spatial axis"):
        ops.conv_volume(1, 2, (3, 3, 3), 2, (1, 1))


@pytest.mark.parametrize("row", flat.ROWS, ids=flat.row_id)
def test_sizes_of_a_trivial_depth_axis_equal_the_two_axis_sizes(row):
    tr, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group = row
    geom = ops.conv_volume(N, Cin, (H, W), Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), group)
    flat_geom = ops.conv_geometry(N, Cin, H, W, Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), group)
    assert ops.conv_volume_sizes(geom, tr) == ops.conv_geometry_sizes(flat_geom, tr)
    assert ops.conv_volume_out_shape(geom, tr) == (1,) + ops.conv_geometry_out_shape(flat_geom, tr)


def wgrad_parts(row):
    """The weight-gradient plan, stated on its own: tiles of 16 k-columns x 64 channels inside one group; N x ceil(P / 64) voxel chunks cut
    into at most 64 parts, as many as bring the launch to about 2048 workgroups, none empty."""
    tr, N, Cin, size, Cout, kernel, stride, pad, dilation, group = fields(row)
    taps = int(np.prod(kernel))
    Cs, Cl, Ps = (Cin, Cout, int(np.prod(size))) if tr else (Cout, Cin, int(np.prod(out_size(row))))
    G, ksteps = padded_dims(Cs // group, (Cl // group) * taps)
    chunks = N * -(-Ps // 64)
    want = max(1, min(64, chunks, 2048 // ((ksteps // 4) * -(-G // 4) * group)))
    per_part = -(-chunks // want)
    return -(-chunks // per_part), G, ksteps


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_sizes_equal_the_padded_layout_per_group(row):
    tr, N, Cin, size, Cout, kernel, stride, pad, dilation, group = fields(row)
    taps = int(np.prod(kernel))
    fwd, dgrad, wgrad, ws = ops.conv_volume_sizes(geom_of(row), tr)
    Gf, kf = padded_dims(Cout // group, (Cin // group) * taps)
    Gd, kd = padded_dims(Cin // group, (Cout // group) * taps)
    assert (fwd, dgrad, wgrad) == (group * Gf * kf * 64, group * Gd * kd * 64, 0)
    parts, G, ksteps = wgrad_parts(row)
    assert ws == 4 * parts * group * 16 * G * 4 * ksteps


# one small layer per pass and kind: taps 2 x 3 x 2, stride (2, 1, 1), pad (1, 0, 1), dilation (2, 1, 2), group 2; 3 -> 5 channels per group
LAYOUTS = {"conv-forward": (False, False), "conv-data-gradient": (False, True), "deconv-forward": (True, False), "deconv-data-gradient": (True, True)}
LAYOUT_TAPS = ((2, 3, 2), (2, 1, 1), (1, 0, 1), (2, 1, 2))


def layout_case(name):
    """A layer whose operand of this pass is, per group, 5 x 36: 5 rows, 3 reduction channels of 2x3x2 taps."""
    tr, backward = LAYOUTS[name]
    Cin, Cout = (10, 6) if backward else (6, 10)
    kernel, stride, pad, dilation = LAYOUT_TAPS
    row = (tr, 1, Cin, 3, 4, 3, Cout) + kernel + stride + pad + dilation + (2,)
    return row, backward, rand(weight_shape(row), 11, 0.1)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_packed_layout_and_the_depth_gathers_restated_in_numpy_multiply_to_the_fp64_convolution(name):
    row, backward, w = layout_case(name)
    tr, N, Cin, size, Cout, kernel, stride, pad, dilation, group = fields(row)
    kd, kh, kw = kernel
    packed = pack_np(w, tr, backward, group)
    assert packed.shape == (2, 1, 48 // 4, 64)                       # two groups; 5 rows in one row group; K = 36 in three chunks of four k-steps
    views = gemm_views(w, tr, backward, group)
    for g in range(group):
        assert np.array_equal(unpack_np(packed[g], 5, 36), views[g])  # the zero padding is where it belongs
    # the tap order: group 1, row 2, reduction channel 1, tap (kz 1, ky 2, kx 1) = (1 kh + 2) kw + 1
    r, tap = 1, (1 * kh + 2) * kw + 1
    swapped = backward != tr
    blob = w[3 + r, 2, 1, 2, 1] if swapped else w[5 + 2, r, 1, 2, 1]  # swapped: blob rows are the reduction channels (3 per group)
    assert views[1][2, r * 12 + tap] == blob
    assert packed[1, 0, (r * 12 + tap) // 4, 16 * ((r * 12 + tap) % 4) + 2] == blob
    x = torch.from_numpy(rand((1, Cin) + tuple(size), 12)).double().requires_grad_(True)
    top = layer64(x, torch.from_numpy(w).double(), None, row)
    assert tuple(top.shape[2:]) == out_size(row)
    if not backward:
        ref, inp, out = top.detach().numpy()[0], x.detach().numpy()[0], out_size(row)
    else:
        gt = torch.from_numpy(rand(tuple(top.shape), 13)).double()
        ref, inp, out = torch.autograd.grad(top, x, gt)[0].numpy()[0], gt.numpy()[0], tuple(size)
    rg = inp.shape[0] // group                                        # reduction channels per group
    for g in range(group):
        col = (col_transposed if swapped else col_forward)(inp[g * rg:(g + 1) * rg], kernel, stride, pad, dilation, out)
        got = (views[g].astype(np.float64) @ col).reshape((5,) + tuple(out))
        assert np.abs(got - ref[5 * g:5 * g + 5]).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------------ GPU tier
def run_forward(row, c, bias=True, relu=False, slope=0.0, N=None, x=None):
    tr = row[0]
    geom = geom_of(row, N)
    packed = ops.conv_volume_pack_weights(dev(c["w"]), geom, tr)
    return ops.conv_volume_forward(dev(c["x"] if x is None else x), packed, dev(c["b"]) if bias else None, geom, tr, relu=relu, negative_slope=slope)


def run_dgrad(row, c, N=None, g=None):
    tr = row[0]
    geom = geom_of(row, N)
    packed = ops.conv_volume_pack_weights(dev(c["w"]), geom, tr, backward=True)
    return ops.conv_volume_backward_data(dev(c["g"] if g is None else g), packed, geom, tr)


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
    voxels = int(np.prod(out_size(row)))
    geom = geom_of(row)
    w0, b0 = rand(c["w"].shape, 21), rand(c["b"].shape, 22)          # non-zero diffs to start from
    for accumulate in (False, True):
        dw, db = dev(w0), dev(b0)
        ops.conv_volume_backward_weights(dev(c["x"]), dev(c["g"]), geom, tr, weight_diff=dw, bias_diff=db, accumulate=accumulate)
        rw = c["gw"] + (w0.astype(np.float64) if accumulate else 0.0)
        rb = c["gb"] + (b0.astype(np.float64) if accumulate else 0.0)
        assert ratio("weight gradient accumulate=%d" % accumulate, row, dw.cpu().numpy(), rw, 2e-6 * scale_of(rw) * math.sqrt(N * voxels)) <= 1.0
        assert ratio("bias gradient accumulate=%d" % accumulate, row, db.cpu().numpy(), rb, 2e-6 * scale_of(rb)) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pack_kernel_writes_the_restated_layout(name):
    row, backward, w = layout_case(name)
    got = ops.conv_volume_pack_weights(dev(w), geom_of(row), row[0], backward=backward).cpu().numpy()
    assert np.array_equal(got, pack_np(w, row[0], backward, row[19]).ravel())


@pytest.mark.gpu
@pytest.mark.parametrize("row", [GROUPED, ROWS[11]], ids=row_id)
def test_channel_slices_on_a_grouped_row(row):
    """Bottom read from the middle of a wider blob, top written into the middle of a wider sentinel-filled one, on layers with groups: the
    group offsets add to the caller's c0; nothing outside the slice moves, the bits inside equal the whole-blob run."""
    c = case(row)
    tr, N, Cin, size, Cout = fields(row)[:5]
    geom = geom_of(row)

    def wide(a, c0, extra):
        blob = np.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], SENTINEL, np.float32)
        blob[:, c0:c0 + a.shape[1]] = a
        return dev(blob)

    def outside_untouched(blob, c0, Cc):
        b = blob.cpu().numpy()
        return (b[:, :c0] == SENTINEL).all() and (b[:, c0 + Cc:] == SENTINEL).all()

    whole = run_forward(row, c, True, True, 0.1)
    packed = ops.conv_volume_pack_weights(dev(c["w"]), geom, tr)
    top = torch.full((N, Cout + 5) + out_size(row), SENTINEL, device="cuda")
    ops.conv_volume_forward(wide(c["x"], 3, 4), packed, dev(c["b"]), geom, tr, relu=True, negative_slope=0.1, out=top, out_c0=2, in_c0=3)
    assert outside_untouched(top, 2, Cout) and torch.equal(top[:, 2:2 + Cout], whole)
    whole = run_dgrad(row, c)
    packed = ops.conv_volume_pack_weights(dev(c["w"]), geom, tr, backward=True)
    bd = torch.full((N, Cin + 3) + tuple(size), SENTINEL, device="cuda")
    ops.conv_volume_backward_data(wide(c["g"], 1, 2), packed, geom, tr, top_c0=1, out=bd, out_c0=2)
    assert outside_untouched(bd, 2, Cin) and torch.equal(bd[:, 2:2 + Cin], whole)
    dw, db = ops.conv_volume_backward_weights(dev(c["x"]), dev(c["g"]), geom, tr)
    dw2, db2 = ops.conv_volume_backward_weights(wide(c["x"], 3, 4), wide(c["g"], 1, 2), geom, tr, bottom_c0=3, top_c0=1)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_a_sample_does_not_see_its_batch():
    for row in (ROWS[2], ROWS[6], ROWS[8]):                           # N = 2 each; ROWS[6]: a tile that holds the end of sample 0 and the start of nothing else
        c = case(row)
        tr = row[0]
        f1, f2, d1, d2 = run_forward(row, c, True, True, 0.1), run_forward(row, c, True, True, 0.1), run_dgrad(row, c), run_dgrad(row, c)
        assert torch.equal(f1, f2) and torch.equal(d1, d2)
        w1 = ops.conv_volume_backward_weights(dev(c["x"]), dev(c["g"]), geom_of(row), tr)
        w2 = ops.conv_volume_backward_weights(dev(c["x"]), dev(c["g"]), geom_of(row), tr)
        assert torch.equal(w1[0], w2[0]) and torch.equal(w1[1], w2[1])
        n = 1                                                         # sample 1 of the N = 2 run equals the N = 1 run of that sample
        assert torch.equal(run_forward(row, c, True, True, 0.1, N=1, x=c["x"][n:n + 1])[0], f1[n])
        assert torch.equal(run_dgrad(row, c, N=1, g=c["g"][n:n + 1])[0], d1[n])


@pytest.mark.gpu
@pytest.mark.parametrize("row", [ROWS[2], ROWS[3], ROWS[8], ROWS[11]], ids=row_id)
def test_every_row_group_variant_gives_the_same_bits(row):
    """The depth gather kernels exist with 1, 2 and 4 row groups of 16 output channels per workgroup; forced one after the other they write
    the same bits, forward and data gradient."""
    c = case(row)
    try:
        got = []
        for groups in (0, 1, 2, 4):
            ops.set_conv_general_groups(groups)
            got.append((run_forward(row, c, True, True, 0.1), run_dgrad(row, c)))
    finally:
        ops.set_conv_general_groups(0)
    assert all(torch.equal(f, got[0][0]) and torch.equal(d, got[0][1]) for f, d in got[1:])


def three_passes(api, geom, tr, x, w, b, g):
    pack, forward, dgrad, wgrad = (getattr(ops, "conv_%s_%s" % (api, n)) for n in ("pack_weights", "forward", "backward_data", "backward_weights"))
    pf, pb = pack(w, geom, tr), pack(w, geom, tr, backward=True)
    return [pf, pb, forward(x, pf, b, geom, tr, relu=True, negative_slope=0.1), dgrad(g, pb, geom, tr), *wgrad(x, g, geom, tr)]


@pytest.mark.gpu
@pytest.mark.parametrize("row", [flat.ROWS[1], flat.ROWS[9], flat.ROWS[13]], ids=flat.row_id)
def test_a_trivial_depth_axis_gives_the_bits_of_the_two_axis_entry_points(row):
    """Identity (a): rows of tests/conv_geometry_cases.py through fn2_conv_volume_* with Din = kd = sd = dd = 1, pd = 0: the packed operands
    and the results of all three passes are bit-identical to fn2_conv_geometry_*."""
    tr, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group = row
    c = flat.case(row)
    geom2 = ops.conv_geometry(N, Cin, H, W, Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), group)
    geom3 = ops.conv_volume(N, Cin, (1, H, W), Cout, (1, kh, kw), (1, sh, sw), (0, ph, pw), (1, dh, dw), group)
    x, w, b, g = dev(c["x"]), dev(c["w"]), dev(c["b"]), dev(c["g"])
    two = three_passes("geometry", geom2, tr, x, w, b, g)
    three = three_passes("volume", geom3, tr, x.unsqueeze(2), w.unsqueeze(2), b, g.unsqueeze(2))
    for a, v in zip(two, three):
        assert torch.equal(a.reshape(-1), v.reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("tr", [False, True], ids=["conv", "deconv"])
def test_one_spatial_axis_gives_the_bits_of_the_folded_two_axis_layer(tr):
    """Identity (b): a layer on [N, C, L] blobs -- 7 taps, stride 2, pad 3, dilation 2, group 2 -- is the 2-D layer with H = 1, kh = 1, sh = 1,
    ph = 0, dh = 1."""
    N, Cin, L, Cout, k, s, p, d, group = 2, 6, 37, 10, 7, 2, 3, 2, 2
    geom1 = ops.conv_volume(N, Cin, (L,), Cout, k, s, p, d, group)
    geom2 = ops.conv_geometry(N, Cin, 1, L, Cout, (1, k), (1, s), (0, p), (1, d), group)
    Lo = ops.conv_geometry_out_shape(geom2, tr)[1]
    assert ops.conv_volume_out_shape(geom1, tr) == (1, 1, Lo)
    x, b, g = dev(rand((N, Cin, L), 31)), dev(rand((Cout,), 33)), dev(rand((N, Cout, Lo), 34))
    w = dev(rand((Cin, Cout // group, k) if tr else (Cout, Cin // group, k), 32, 0.1))
    one = three_passes("volume", geom1, tr, x[:, :, None, None], w[:, :, None, None], b, g[:, :, None, None])
    two = three_passes("geometry", geom2, tr, x[:, :, None], w[:, :, None], b, g[:, :, None])
    for a, v in zip(two, one):
        assert torch.equal(a.reshape(-1), v.reshape(-1))
    ref = (torch.nn.functional.conv_transpose1d if tr else torch.nn.functional.conv1d)(x.double().cpu(), w.double().cpu(), b.double().cpu(), stride=s,
                                                                                       padding=p, dilation=d, groups=group)
    ref = leaky(ref.numpy(), 0.1)
    assert ratio("1-axis forward", (tr, N, Cin, L, Cout), one[2].reshape(N, Cout, Lo).cpu().numpy(), ref, TOL_DIRECT * scale_of(ref)) <= 1.0


@pytest.mark.gpu
def test_supported_sizes_and_the_launches_refuse_the_same_geometries():
    L = _lib.lib()
    UNSUPPORTED, INVALID_ARG, WORKSPACE = (_lib.CONSTANTS["FN2_ERR_" + n] for n in ("UNSUPPORTED", "INVALID_ARG", "WORKSPACE"))
    buf = torch.full((1 << 16,), SENTINEL, device="cuda")
    ptr, null, st = C.c_void_p(buf.data_ptr()), C.c_void_p(0), C.c_void_p(0)

    def launches(geom, tr, bottom=ptr, top=ptr, weight=ptr, ws=ptr, ws_bytes=4 << 16, bottom_c0=0, top_channels=None):
        Cin, Cout = (geom[1], geom[5]) if geom is not None else (1, 1)
        tc = Cout if top_channels is None else top_channels
        return [L.fn2_conv_volume_pack_weights(geom, tr, 0, weight, ptr, st),
                L.fn2_conv_volume_forward(geom, tr, bottom, Cin, bottom_c0, weight, null, top, tc, 0, 0, C.c_float(0), st),
                L.fn2_conv_volume_backward_data(geom, tr, top, tc, 0, weight, bottom, Cin, bottom_c0, st),
                L.fn2_conv_volume_backward_weights(geom, tr, bottom, Cin, bottom_c0, top, tc, 0, weight, null, 0, ws, ws_bytes, st)]

    for row in INVALID:
        geom, tr = geom_of(row), int(row[0])
        assert L.fn2_conv_volume_supported(geom, tr) == 0
        assert L.fn2_conv_volume_sizes(geom, tr, None, None, None, None) == UNSUPPORTED
        assert launches(geom, tr) == [UNSUPPORTED] * 4
        assert "no kernel for" in L.fn2_last_error_string().decode()
    assert launches(None, 0) == [UNSUPPORTED] * 4                     # a null geom
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                              # refused on the host: nothing was launched, nothing written
    geom, tr = geom_of(GROUPED), 0
    assert launches(geom, tr, bottom=null) == [0, INVALID_ARG, INVALID_ARG, INVALID_ARG]
    assert launches(geom, tr, top=null)[1:] == [INVALID_ARG] * 3
    assert launches(geom, tr, weight=null) == [INVALID_ARG] * 4
    assert launches(geom, tr, bottom_c0=1)[1:] == [INVALID_ARG] * 3                  # a slice outside its blob, bottom side
    assert launches(geom, tr, top_channels=geom[5] - 1)[1:] == [INVALID_ARG] * 3     # and top side
    assert launches(geom, tr, ws=null)[3] == WORKSPACE and launches(geom, tr, ws_bytes=16)[3] == WORKSPACE
    assert L.fn2_conv_volume_pack_weights(geom, tr, 3, ptr, ptr, st) == INVALID_ARG
    torch.cuda.synchronize()
    # the valid calls among these (a pack; with a bad workspace alone the pack, forward and data gradient) write the layer's blobs at the
    # start of the buffer -- the forward operand (2 groups x 2 row groups x 4 k-steps x 64 = 1024 floats), the top blob (34 x 2 x 3 x 4 = 816)
    # or the bottom blob (4 x 3 x 4 x 5 = 240) at the most; the refused ones wrote nothing beyond
    assert max(ops.conv_volume_sizes(geom, tr)[0], 34 * 2 * 3 * 4, 4 * 3 * 4 * 5) <= 1024 and bool((buf[1024:] == SENTINEL).all())
