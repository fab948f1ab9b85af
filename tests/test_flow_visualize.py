"""The visualisation kernels (csrc/flow_visualize.hip) through the C ABI of include/flownet2_hip_flow_visualize.h.  Colour coding: every
byte equal to the truncated float64 evaluation wherever that lies farther than the operation-count bound from an integer (and wherever
the bound is 0: zero flow is white and a saturated channel 255, bit for bit), either neighbour elsewhere; unknown flow black; the radius
used within one ulp of the restatement's.  Error image: the bin's colour wherever the float64 n lies farther than its bound from a bin
edge.  Both: the same bytes for a sample alone and in a batch, from run to run, at both alignments and with or without maxrad_out; no byte
outside [N,H,W,3]; functional.flow_to_color / flow_error_map equal to the C call.

Figures seen on an MI355X (printed by the tests): the ordinary case leaves at most 0.033 % of the colour values and 1.7 % of the error
pixels (the ones placed on a bin edge on purpose) to the loose rule, against the cap of 3 %; delta stays below 9.2e-4; every byte of every
case also equalled the float32 restatement."""
import functools

import numpy as np
import pytest
import torch

import flow_visualize_ref as VR
from flownet2_amd import functional as Fn

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
MARGIN = 64
SAMPLE, BATCH, FIXED = VR.NORM["SAMPLE"], VR.NORM["BATCH"], VR.NORM["FIXED"]
# name -> (shape, offset: every float blob starts that many floats, and rgb that many bytes, into its allocation).  A thread owns four
# neighbouring pixels of a row where W % 4 == 0 (16-byte loads and 4-byte stores where the pointers allow) and one pixel otherwise; a
# sample is cut into ceil(H W / 1024) <= 128 workgroups of 256 threads.
SHAPES = {
    "1x2x1x1": ((1, 2, 1, 1), 0),
    "2x2x3x5": ((2, 2, 3, 5), 0),
    "3x2x7x67": ((3, 2, 7, 67), 0),                       # odd width: one pixel per thread, a ragged second step
    "2x2x16x64": ((2, 2, 16, 64), 0),                     # the aligned path: 16-byte loads, three 4-byte stores
    "2x2x16x64_offset1": ((2, 2, 16, 64), 1),             # every pointer advanced: 4-byte loads and byte stores, the same bytes
    "1x2x33x67": ((1, 2, 33, 67), 0),                     # one pixel per thread, 3 workgroups per sample, a ragged last one
    "2x2x36x60": ((2, 2, 36, 60), 0),                     # four pixels per thread, 3 workgroups per sample, a ragged last one
}
KINDS = ("zero", "right2", "up2", "negzero", "nonfinite", "ordinary", "outlier")
FIXED_MAX = 2.5                                            # under NORM_FIXED: a good share of the ordinary case lies beyond it


def make_flow(kind, shape, seed):
    N, _, H, W = shape
    flow = np.zeros(shape, np.float32)
    if kind == "right2":
        flow[:, 0] = 2.0
    elif kind == "up2":
        flow[:, 1] = -2.0
    elif kind == "negzero":
        flow[:] = -0.0
        flow[:, 0, :, W // 2:] = 1.5                                                # u > 0 with v = -0.0f: the far side of the seam
    elif kind in ("nonfinite", "ordinary", "outlier"):
        flow = VR.smooth_flow(shape, seed)
    if kind == "nonfinite":
        rng = np.random.default_rng(seed + 77)
        bad = [np.nan, np.inf, -np.inf, 1e10, -1e10]
        flat = flow.reshape(N, 2, H * W)
        for k, pos in enumerate(rng.permutation(H * W)[:min(H * W, 10)]):
            flat[k % N, k % 2, pos] = bad[k % len(bad)]
        if N > 1:
            flat[N - 1] = np.nan                                                    # a sample without a known pixel: its maximum is 1
    if kind == "outlier":
        flow[N - 1, :, H // 2, W // 2] = (30.0, -40.0)                              # ten times the rest
    return flow


@functools.lru_cache(maxsize=None)
def _flow(name, kind):
    base = name.replace("_offset1", "")
    flow = make_flow(kind, SHAPES[name][0], seed=1 + sorted(SHAPES).index(base) * 10 + KINDS.index(kind))
    flow.setflags(write=False)
    return flow


@functools.lru_cache(maxsize=None)
def _error_case(name):
    base = name.replace("_offset1", "")
    case = VR.error_case(SHAPES[name][0], seed=100 + sorted(SHAPES).index(base))
    for a in case:
        a.setflags(write=False)
    return case


def _dev(a, offset=0):
    """A device copy of float32 array `a` that starts `offset` floats into its (256-byte aligned) allocation; None stays None."""
    if a is None:
        return None
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def _rgb(shape, offset):
    """(the whole sentinel-filled allocation, the [N,H,W,3] view that starts MARGIN + offset bytes into it)."""
    N, _, H, W = shape
    n = N * H * W * 3
    buf = torch.full((n + 2 * MARGIN + offset,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf[MARGIN + offset:MARGIN + offset + n].view(N, H, W, 3)
    assert view.data_ptr() % 4 == offset % 4
    return buf, view


def _take(buf, view, offset):
    """The picture on the host, after checking that every byte around it still holds the sentinel."""
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    n = view.numel()
    assert np.all(host[:MARGIN + offset] == SENTINEL) and np.all(host[MARGIN + offset + n:] == SENTINEL), "a byte outside [N,H,W,3] was written"
    return host[MARGIN + offset:MARGIN + offset + n].reshape(tuple(view.shape)).copy()


def run_color(flow, norm=SAMPLE, max_flow=0.0, offset=0, want_maxrad=True):
    """One call in fresh allocations -> (uint8 [N,H,W,3], float32 [N] or None) on the host."""
    shape = flow.shape
    N, _, H, W = shape
    dflow = _dev(np.asarray(flow), offset)
    buf, view = _rgb(shape, offset)
    ws_bytes = VR.sizes(N, H, W)
    ws = torch.full((ws_bytes,), SENTINEL, dtype=torch.uint8, device="cuda") if norm != FIXED else None
    used = torch.full((N + 2,), -7.0, dtype=torch.float32, device="cuda") if want_maxrad else None
    assert VR.call_color(dflow, shape, view, norm, max_flow, used[1:] if want_maxrad else None, ws, ws_bytes if ws is not None else 0) == VR.OK
    rgb = _take(buf, view, offset)
    if not want_maxrad:
        return rgb, None
    used = used.cpu().numpy()
    assert used[0] == -7.0 and used[-1] == -7.0
    return rgb, used[1:-1]


@functools.lru_cache(maxsize=None)
def _color(name, kind, norm):
    return run_color(_flow(name, kind), norm, FIXED_MAX if norm == FIXED else 0.0, SHAPES[name][1])


def run_error(pred, gt, valid=None, occ=None, offset=0, abs_thresh=VR.ABS_THRESH, rel_thresh=VR.REL_THRESH):
    shape = pred.shape
    buf, view = _rgb(shape, offset)
    d = [_dev(None if a is None else np.asarray(a), offset) for a in (pred, gt, valid, occ)]
    assert VR.call_error(d[0], d[1], shape, view, d[2], d[3], abs_thresh, rel_thresh) == VR.OK
    return _take(buf, view, offset)


@functools.lru_cache(maxsize=None)
def _error(name):
    return run_error(*_error_case(name), offset=SHAPES[name][1])


# ---- the colour coding -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_colour_coding_against_the_float64_evaluation(name, kind):
    flow = _flow(name, kind)
    known = VR._known(flow)
    for norm, label in ((SAMPLE, "sample"), (BATCH, "batch"), (FIXED, "fixed")):
        max_flow = FIXED_MAX if norm == FIXED else None
        rgb, used = _color(name, kind, norm)
        wrong, loose, delta = VR.color_check(rgb, flow, norm, max_flow)
        ref32, maxrad = VR.color32(flow, norm, max_flow)
        print(f"{name} {kind} {label}: wrong {wrong}, loose share {loose:.5f}, largest delta {delta:.3e}, bytes off the float32 "
              f"restatement {(rgb != ref32).sum()} of {rgb.size}")
        assert wrong == 0
        assert not rgb[~known].any(), "unknown flow must be black"
        assert np.all(np.abs(used.astype(np.float64) - maxrad.astype(np.float64)) <= np.spacing(maxrad)), (used, maxrad)
        if norm == FIXED:
            assert np.all(used == np.float32(FIXED_MAX))
        if kind == "ordinary":
            assert loose <= 0.03, "vacuous: too many values left to the loose rule"
    if kind == "outlier":
        beyond = VR.color_bounds(flow, FIXED, FIXED_MAX)["rn"] > 1
        assert beyond[-1, flow.shape[2] // 2, flow.shape[3] // 2] and (flow.shape[2] * flow.shape[3] == 1 or not beyond.all())
    if kind == "nonfinite" and flow.shape[0] > 1:
        assert _color(name, kind, SAMPLE)[1][-1] == 1.0 and not _color(name, kind, SAMPLE)[0][-1].any()


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_cases_bit_for_bit(name):
    N, _, H, W = SHAPES[name][0]
    for norm in (SAMPLE, BATCH, FIXED):
        assert np.all(_color(name, "zero", norm)[0] == 255), "zero flow is white"
        right = _color(name, "right2", norm)[0]
        assert np.all(right[..., 0] == 255), "a saturated channel stays 255"
        neg = _color(name, "negzero", norm)[0]
        assert np.all(neg[:, :, :W // 2] == 255) and np.all(neg[:, :, W // 2:, 0] == 255)
    for norm in (SAMPLE, BATCH):
        assert np.all(_color(name, "right2", norm)[0] == np.array([255, 0, 0], np.uint8))      # rn == 1 at every pixel: the wheel's entry 0
        assert np.all(_color(name, "right2", norm)[1] == 2.0) and np.all(_color(name, "zero", norm)[1] == 1.0)
        up = _color(name, "up2", norm)[0]
        assert np.all(up[..., 1] == 0) and np.all(up[..., 2] == 255) and np.all(np.abs(up[..., 0].astype(int) - 88) <= 1)
        neg = _color(name, "negzero", norm)[0]
        if W > 1:
            assert np.all(neg[:, :, W // 2:] == np.array([255, 0, 43], np.uint8))                # the seam's far side: entry 54


def test_the_batch_shares_the_largest_maximum():
    name = "3x2x7x67"
    flow = _flow(name, "outlier")
    _, per_sample = _color(name, "outlier", SAMPLE)
    rgb, shared = _color(name, "outlier", BATCH)
    assert len(set(per_sample.tolist())) == 3 and np.all(shared == per_sample.max()) and shared[0] == np.float32(50.0)
    alone, _ = run_color(flow[:1], FIXED, 50.0)                                      # which is sample 0 under that fixed radius
    assert np.array_equal(rgb[0], alone[0])


@pytest.mark.parametrize("name", ["3x2x7x67", "2x2x36x60", "2x2x16x64_offset1"])
def test_a_sample_has_the_same_bytes_alone_and_in_any_batch(name):
    offset = SHAPES[name][1]
    one, other = _flow(name, "ordinary")[:1], _flow(name, "outlier")[-1:]
    p, g, v, o = (a[:1] for a in _error_case(name))
    p2, g2, v2, o2 = (a[-1:] for a in _error_case(name))
    for norm, max_flow in ((SAMPLE, 0.0), (FIXED, FIXED_MAX)):
        alone, r_alone = run_color(one, norm, max_flow, offset)
        first, r_first = run_color(np.concatenate([one, other, other]), norm, max_flow, offset)
        third, r_third = run_color(np.concatenate([other, other, one]), norm, max_flow, offset)
        assert np.array_equal(alone[0], first[0]) and np.array_equal(alone[0], third[2]) and r_alone[0] == r_first[0] == r_third[2]
        again, r_again = run_color(one, norm, max_flow, offset)                     # and from run to run
        assert np.array_equal(alone, again) and np.array_equal(r_alone, r_again)
        assert np.array_equal(alone, _color(name, "ordinary", norm)[0][:1])
    e_alone = run_error(p, g, v, o, offset)
    e_first = run_error(*(np.concatenate([a, b, b]) for a, b in ((p, p2), (g, g2), (v, v2), (o, o2))), offset=offset)
    e_third = run_error(*(np.concatenate([b, b, a]) for a, b in ((p, p2), (g, g2), (v, v2), (o, o2))), offset=offset)
    assert np.array_equal(e_alone[0], e_first[0]) and np.array_equal(e_alone[0], e_third[2])
    assert np.array_equal(e_alone, run_error(p, g, v, o, offset)) and np.array_equal(e_alone[0], _error(name)[0])


@pytest.mark.parametrize("kind", ["ordinary", "nonfinite", "outlier"])
def test_alignment_and_maxrad_out_change_no_byte(kind):
    for norm in (SAMPLE, BATCH, FIXED):
        aligned, r0 = _color("2x2x16x64", kind, norm)
        shifted, r1 = _color("2x2x16x64_offset1", kind, norm)
        assert np.array_equal(aligned, shifted) and np.array_equal(r0, r1)
        for name in ("2x2x16x64", "2x2x16x64_offset1", "3x2x7x67"):
            without, none = run_color(_flow(name, kind), norm, FIXED_MAX if norm == FIXED else 0.0, SHAPES[name][1], want_maxrad=False)
            assert none is None and np.array_equal(without, _color(name, kind, norm)[0])
    # the mixed forms: 16-byte loads with byte stores, 4-byte loads with 4-byte stores
    flow = _flow("2x2x16x64", kind)
    shape = flow.shape
    ws = torch.empty(VR.sizes(2, 16, 64), dtype=torch.uint8, device="cuda")
    for f_off, b_off in ((0, 1), (1, 0), (2, 2), (0, 3)):
        buf, view = _rgb(shape, b_off)
        assert VR.call_color(_dev(np.asarray(flow), f_off), shape, view, SAMPLE, 0.0, None, ws, ws.numel()) == VR.OK
        assert np.array_equal(_take(buf, view, b_off), _color("2x2x16x64", kind, SAMPLE)[0]), (f_off, b_off)
    assert np.array_equal(_error("2x2x16x64"), _error("2x2x16x64_offset1"))


# ---- the error image -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_error_map_against_the_float64_evaluation(name):
    pred, gt, valid, occ = _error_case(name)
    rgb = _error(name)
    wrong, loose = VR.error_check(rgb, pred, gt, valid, occ)
    ref32 = VR.error_map32(pred, gt, valid, occ)
    print(f"{name}: wrong {wrong}, loose share {loose:.5f}, pixels off the float32 restatement {(rgb != ref32).any(-1).sum()} of {rgb[..., 0].size}")
    assert wrong == 0 and loose <= 0.03
    use = VR._ok(gt[:, 0]) & VR._ok(gt[:, 1]) & (valid[:, 0] != 0)
    assert not rgb[~use].any(), "no ground truth: black"
    bad_pred = use & ~(VR._ok(pred[:, 0]) & VR._ok(pred[:, 1]))
    last = np.where(occ[:, 0, ..., None] != 0, VR.BIN_COLORS[9] // 2, VR.BIN_COLORS[9])
    assert np.array_equal(rgb[bad_pred], last[bad_pred])
    # the optional planes one by one, and other thresholds
    offset = SHAPES[name][1]
    for v, o in ((None, None), (valid, None), (None, occ)):
        got = run_error(pred, gt, v, o, offset)
        assert VR.error_check(got, pred, gt, v, o)[0] == 0
    got = run_error(pred, gt, valid, occ, offset, abs_thresh=1.0, rel_thresh=0.5)
    assert VR.error_check(got, pred, gt, valid, occ, 1.0, 0.5)[0] == 0 and (name == "1x2x1x1" or not np.array_equal(got, rgb))


def test_error_map_exact_cases():
    gt = np.zeros((1, 2, 1, 12), np.float32)
    gt[:, 0], gt[:, 1] = 30.0, 40.0
    pred = gt.copy()
    pred[0, 0, 0] += np.array([0.0, 0.125, 0.25, 0.5, 1.0, 2.0, 2.5, 2.75, 7.0, 13.0, 30.0, 50.0], np.float32)
    bins = [0, 0, 1, 2, 3, 4, 4, 4, 6, 7, 8, 9]
    assert [tuple(c) for c in run_error(pred, gt)[0, 0]] == [tuple(VR.BIN_COLORS[b]) for b in bins]
    zero = np.zeros((1, 2, 1, 3), np.float32)                                       # mag == 0: the absolute term alone
    p3 = zero.copy()
    p3[0, 1, 0] = (0.0, 1.25, 60.0)
    assert [tuple(c) for c in run_error(p3, zero)[0, 0]] == [tuple(VR.BIN_COLORS[b]) for b in (0, 3, 9)]
    g4, p4 = gt[:, :, :, :6].copy(), gt[:, :, :, :6].copy()
    g4[0, 0, 0, 0], g4[0, 1, 0, 1], p4[0, 0, 0, 2], p4[0, 1, 0, 3] = np.nan, 1e10, np.nan, -np.inf
    valid = np.ones((1, 1, 1, 6), np.float32)
    valid[0, 0, 0, 4] = 0
    occ = np.zeros((1, 1, 1, 6), np.float32)
    occ[0, 0, 0, 3:] = 1
    want = [(0, 0, 0), (0, 0, 0), (165, 0, 38), (82, 0, 19), (0, 0, 0), (24, 27, 74)]
    assert [tuple(c) for c in run_error(p4, g4, valid, occ)[0, 0]] == want
    assert np.array_equal(run_error(p4, g4, valid, occ), VR.error_map32(p4, g4, valid, occ))


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_functional_returns_the_bytes_of_the_c_call():
    name = "2x2x36x60"
    flow = _flow(name, "outlier")
    d = torch.from_numpy(np.array(flow)).cuda()
    for kw, norm in ((dict(), SAMPLE), (dict(norm="batch"), BATCH), (dict(max_flow=FIXED_MAX), FIXED)):
        got = Fn.flow_to_color(d, **kw)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (2, 36, 60, 3)
        assert np.array_equal(got.cpu().numpy(), _color(name, "outlier", norm)[0])
    pred, gt, valid, occ = (torch.from_numpy(np.array(a)).cuda() for a in _error_case(name))
    got = Fn.flow_error_map(pred, gt, valid, occ)
    assert got.dtype == torch.uint8 and got.is_cuda and np.array_equal(got.cpu().numpy(), _error(name))
    with pytest.raises(ValueError, match="must both be"):
        Fn.flow_error_map(pred, gt[:, :, :-1])
    with pytest.raises(ValueError, match="valid"):
        Fn.flow_error_map(pred, gt, valid[:, :, :-1])
    with pytest.raises(Exception, match="max_flow"):
        Fn.flow_to_color(d, max_flow=0.0)


def test_consistency_masks_dim_the_error_map():
    import flow_consistency_ref as CR
    fw, bw = CR.make_case((2, 2, 36, 60), 3)
    dfw, dbw = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    gt = torch.from_numpy(fw + np.float32(0.25)).cuda()
    c = Fn.flow_consistency(dfw, dbw)
    plain, dimmed = Fn.flow_error_map(dfw, gt).cpu().numpy(), Fn.flow_error_map(dfw, gt, occ=c.occ_fw).cpu().numpy()
    occ = c.occ_fw.cpu().numpy()[:, 0] != 0
    assert 0 < occ.sum() < occ.size and np.array_equal(dimmed[~occ], plain[~occ]) and np.array_equal(dimmed[occ], plain[occ] // 2)
    assert VR.error_check(dimmed, fw, gt.cpu().numpy(), None, c.occ_fw.cpu().numpy())[0] == 0
