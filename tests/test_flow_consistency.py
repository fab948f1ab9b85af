"""The forward-backward consistency kernel (csrc/flow_consistency.hip) through the C ABI of include/flownet2_hip_flow_consistency.h: the
flag, occ, err and warped maps equal to the float32 restatement (flow_consistency_ref.ref32) bit for bit at every pixel, the counts equal,
ERR_SUM within the operation-count bound of a float64 evaluation, ERR_MAX exact; the sampled flow against fn2_flow_warp_forward; the same
bits for a sample alone and in a batch, from run to run, at any alignment and with or without the optional outputs; and
functional.flow_consistency feeding functional.flow_metrics."""
import functools

import numpy as np
import pytest
import torch

import flow_consistency_ref as CR
from flownet2_amd import ops
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import CONSISTENCY_COL as COL, CONSISTENCY_FLAGS as FLAG, CONSISTENCY_K as K

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
# name -> (shape, float offset of every float blob inside its allocation).  A thread owns four neighbouring pixels of a row where
# W % 4 == 0 (16-byte accesses where every pointer allows, else 4-byte ones) and one pixel otherwise; a (direction, sample) is cut into
# ceil(H W / 1024) <= 128 workgroups of 256 threads.
SHAPES = {
    "1x2x1x1": ((1, 2, 1, 1), 0),
    "2x2x3x5": ((2, 2, 3, 5), 0),
    "3x2x7x67": ((3, 2, 7, 67), 0),                       # odd width: one pixel per thread, a ragged second step
    "2x2x16x64": ((2, 2, 16, 64), 0),                     # the aligned 16-byte path
    "2x2x16x64_offset1": ((2, 2, 16, 64), 1),             # every float pointer advanced by one float: 4-byte accesses, the same bits
    "1x2x33x67": ((1, 2, 33, 67), 0),                     # one pixel per thread, 3 workgroups per sample, a ragged last one
    "2x2x36x60": ((2, 2, 36, 60), 0),                     # four pixels per thread, 3 workgroups per sample, a ragged last one
}
KINDS = ("zero", "shift2", "edge", "negzero", "nonfinite", "ordinary")


def _smooth(shape, seed, scale=1.0):
    fw, _ = CR.make_case(shape, seed, occluder=False)
    return (fw * np.float32(scale)).astype(np.float32)


def make_inputs(kind, shape, seed):
    N, _, H, W = shape
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    if kind == "zero":
        return np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    if kind == "shift2":
        fw, bw = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        fw[:, 0], bw[:, 0] = 2.0, -2.0
        return fw, bw
    if kind == "edge":
        # even rows point exactly at (W - 1, H - 1): the right and bottom taps clamp onto the corner; odd rows at x2 = W - 0.25, inside by a
        # quarter of a pixel with its right tap clamped; the backward flow points at (0, 0) and at x2 = 0.25 likewise
        fw, bw = np.zeros(shape, np.float32), _smooth(shape, seed)
        odd = (np.arange(H) % 2 == 1)[:, None]
        fw[:, 0] = np.where(odd, np.float32(W - 0.25) - x, np.float32(W - 1) - x)
        fw[:, 1] = np.where(odd, np.float32(0), np.float32(H - 1) - y)
        bw[:, 0, ::3] = np.float32(0.25) - x
        bw[:, 1, ::3] = 0
        return fw, bw
    if kind == "negzero":
        fw, bw = np.full(shape, -0.0, np.float32), _smooth(shape, seed, 0.3)
        bw[:, :, 0, :] = -0.0                                                       # targets at -0.0f in both directions
        return fw, bw
    fw, bw = CR.make_case(shape, seed)
    if kind == "nonfinite":
        rng = np.random.default_rng(seed + 77)
        bad = [np.nan, np.inf, -np.inf, 1e10, -1e10]
        hw = H * W
        for t in (fw, bw):
            flat = t.reshape(N, 2, hw)
            for k, pos in enumerate(rng.permutation(hw)[:min(hw, 10)]):
                flat[k % N, k % 2, pos] = bad[k % len(bad)]
                if hw == 1:
                    break
    return fw, bw


def _dev(a, offset=0):
    """A device copy of float32 array `a` that starts `offset` floats into its (256-byte aligned) allocation."""
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


@functools.lru_cache(maxsize=None)
def _inputs(name, kind):
    shape, _ = SHAPES[name]
    base = name.replace("_offset1", "")
    fw, bw = make_inputs(kind, shape, seed=1 + sorted(SHAPES).index(base) * 10 + KINDS.index(kind))
    fw.setflags(write=False)
    bw.setflags(write=False)
    return fw, bw


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """ref32 of a case, computed once and shared."""
    return CR.ref32(*_inputs(name.replace("_offset1", ""), kind))


def run_arrays(fw, bw, offset=0, outputs=True, alpha=CR.ALPHA, beta=CR.BETA):
    """One call in fresh allocations -> (results [2, N + 1, K] float64, [per direction dict of maps]) on the host."""
    shape = fw.shape
    N, _, H, W = shape
    dfw, dbw = _dev(np.asarray(fw), offset), _dev(np.asarray(bw), offset)
    ws_bytes, _ = CR.sizes(N, H, W)
    ws = torch.full((ws_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    results = torch.full((2 * (N + 1) * K,), float("nan"), dtype=torch.float64, device="cuda")
    maps = {}
    if outputs:
        maps["flags"] = tuple(torch.full((N, 1, H, W), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2))
        for key, ch in (("occ", 1), ("err", 1), ("warped", 2)):
            maps[key] = tuple(_dev(np.full((N, ch, H, W), 7.0, np.float32), offset) for _ in range(2))
    assert CR.call(dfw, dbw, shape, results, ws, ws_bytes, alpha, beta, **maps) == CR.OK
    torch.cuda.synchronize()
    host = [{k: v[d].cpu().numpy() for k, v in maps.items()} for d in range(2)]
    return results.cpu().numpy().reshape(2, N + 1, K), host


@functools.lru_cache(maxsize=None)
def _run(name, kind, outputs=True):
    return run_arrays(*_inputs(name, kind), offset=SHAPES[name][1], outputs=outputs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same_floats(got, want):
    """Equal bit for bit where `want` is a number, NaN exactly where it is NaN."""
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_maps_and_rows_against_the_restatement(name, kind):
    fw, bw = _inputs(name, kind)
    N, _, H, W = fw.shape
    ref = _reference(name, kind)
    results, maps = _run(name, kind)
    for d, (a, o) in enumerate(((fw, bw), (bw, fw))):
        got, want = maps[d], ref[d]
        assert np.array_equal(got["flags"], want["flags"]), f"direction {d}: {(got['flags'] != want['flags']).sum()} flag bytes differ"
        assert np.array_equal(_bits(got["occ"]), _bits(want["occ"]))
        assert _same_floats(got["err"], want["err"]), f"direction {d}: err differs"
        assert _same_floats(got["warped"], want["warped"]), f"direction {d}: warped differs"
        rows = results[d]
        assert np.array_equal(rows[:, CR.COUNT_COLUMNS], want["rows"][:, CR.COUNT_COLUMNS]), "counts differ from the restatement"
        assert np.array_equal(rows[:, COL["ERR_MAX"]], want["rows"][:, COL["ERR_MAX"]])
        ref64, bnd, full = CR.err_sum_bound(a, o)
        assert np.array_equal(full, ~np.isnan(want["err"][:, 0]))
        e = np.abs(rows[:, COL["ERR_SUM"]] - ref64)
        print(f"{name} {kind} direction {d}: ERR_SUM |err| {e.max():.3e}, worst err / bound {(e / np.maximum(bnd, 1e-300)).max():.3f}")
        assert np.isfinite(rows).all() and np.all(e <= bnd)
        # against the float64 sum of the very float32 values: only the order of the fp64 additions differs
        s32 = want["rows"][:, COL["ERR_SUM"]]
        assert np.all(np.abs(rows[:, COL["ERR_SUM"]] - s32) <= N * H * W * 2.0 ** -53 * s32)


@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_flow_is_consistent_everywhere(name):
    results, maps = _run(name, "zero")
    N, _, H, W = SHAPES[name][0]
    for d in range(2):
        assert not maps[d]["flags"].any() and not maps[d]["occ"].any() and not _bits(maps[d]["err"]).any() and not _bits(maps[d]["warped"]).any()
        want = np.zeros(K)
        want[COL["PIXELS"]] = H * W
        assert np.array_equal(results[d, :N], np.tile(want, (N, 1)))
        want[COL["PIXELS"]] = N * H * W
        assert np.array_equal(results[d, N], want)


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_shift_of_two_leaves_exactly_two_columns_outside(name):
    results, maps = _run(name, "shift2")
    N, _, H, W = SHAPES[name][0]
    cols = np.arange(W)
    for d, outside in enumerate((cols >= W - 2, cols < 2)):
        want = np.where(outside, FLAG["OUTSIDE"], 0).astype(np.uint8)
        assert np.array_equal(maps[d]["flags"], np.broadcast_to(want, (N, 1, H, W)))
        assert np.array_equal(maps[d]["occ"], np.broadcast_to(outside.astype(np.float32), (N, 1, H, W)))
        err = maps[d]["err"]
        assert np.array_equal(np.isnan(err), np.broadcast_to(outside, err.shape)) and not _bits(err[..., ~outside]).any()
        assert np.array_equal(results[d, :N, COL["OUTSIDE"]], np.full(N, H * min(2, W))) and not results[d, :, COL["ERR_SUM"]].any()


def test_edge_targets_clamp_their_taps():
    """x2 = W - 1 and y2 = H - 1 exactly, and x2 = W - 0.25: inside, the right / bottom tap clamped onto the last column / row."""
    name = "3x2x7x67"
    fw, bw = _inputs(name, "edge")
    N, _, H, W = fw.shape
    _, maps = _run(name, "edge")
    f0 = maps[0]["flags"][:, 0]
    assert not (f0 & (FLAG["OUTSIDE"] | FLAG["NONFINITE"])).any()                   # every forward target is inside
    wu = maps[0]["warped"][:, 0]
    for n in range(N):
        assert np.all(wu[n, 0::2] == bw[n, 0, H - 1, W - 1])                        # al = be = 0 at the corner: the corner value itself
        v = np.broadcast_to(bw[n, 0, 1::2, W - 1:W], (H // 2, W))                  # both taps are column W - 1: 0.25 v + 0.75 v, three roundings
        assert np.all(np.abs(wu[n, 1::2] - v) <= 3 * 2.0 ** -24 * np.abs(v))
    f1 = maps[1]["flags"][:, 0]
    assert not (f1[:, ::3] & (FLAG["OUTSIDE"] | FLAG["NONFINITE"])).any()           # x2 = 0.25 with a small v: inside


def test_nonfinite_inputs_reach_the_pixel_and_its_samplers():
    name = "3x2x7x67"
    fw, bw = _inputs(name, "nonfinite")
    _, maps = _run(name, "nonfinite")
    for d, (a, o) in enumerate(((fw, bw), (bw, fw))):
        own_bad = ~(np.abs(a) <= 1e9).all(1)
        fl = maps[d]["flags"][:, 0]
        assert own_bad.sum() >= 5 and np.all(fl[own_bad] == FLAG["NONFINITE"])      # the flag alone: nothing else was computed there
        sampled_bad = ~own_bad & ((fl & FLAG["NONFINITE"]) != 0)
        assert sampled_bad.any()                                                    # an otherwise finite pixel with a bad tap
        assert np.isnan(maps[d]["err"][:, 0][own_bad | sampled_bad]).all() and np.all(maps[d]["occ"][:, 0][own_bad | sampled_bad] == 1)


@pytest.mark.parametrize("name", ["2x2x3x5", "3x2x7x67", "2x2x16x64", "2x2x16x64_offset1", "2x2x36x60"])
def test_sampled_flow_against_flow_warp(name):
    """Independent of the restatement: the other flow sampled at the target, against fn2_flow_warp_forward(o, a, FN2_FILL_NAN) -- the
    kernel pinned to the reference's layer.  Both are convex combinations of the same four taps, rounded at most eight times each, hence
    16 * 2^-24 * max |tap|; and both have NaN at the same pixels."""
    fw, bw = _inputs(name, "ordinary")
    N, _, H, W = fw.shape
    _, maps = _run(name, "ordinary")
    for d, (a, o) in enumerate(((fw, bw), (bw, fw))):
        warp = ops.flow_warp_forward(torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(a)).cuda(), ops.FILL_NAN).cpu().numpy()
        got = maps[d]["warped"]
        assert np.array_equal(np.isnan(got), np.isnan(warp)) and 0 < np.isnan(warp).sum() < warp.size
        _, inside, (ixL, ixR, iyT, iyB), _, _ = CR._taps(np.asarray(a), H, W)
        for c in (0, 1):
            taps = np.stack([np.abs(CR._gather(np.asarray(o), c, iy, ix)) for iy, ix in ((iyT, ixL), (iyT, ixR), (iyB, ixL), (iyB, ixR))])
            bound = 16 * 2.0 ** -24 * taps.max(0).astype(np.float64)
            diff = np.abs(got[:, c].astype(np.float64) - warp[:, c].astype(np.float64))
            print(f"{name} direction {d} channel {c}: worst |diff| / bound {np.nanmax(np.where(inside, diff / np.maximum(bound, 1e-300), 0)):.3f}")
            assert np.all(diff[inside] <= bound[inside])


@pytest.mark.parametrize("name", ["3x2x7x67", "2x2x36x60", "2x2x16x64_offset1"])
def test_a_sample_has_the_same_bits_alone_and_in_any_batch(name):
    fw, bw = _inputs(name, "ordinary")
    offset = SHAPES[name][1]
    one_fw, one_bw = fw[:1], bw[:1]
    other_fw, other_bw = _inputs(name, "nonfinite")
    alone, maps_alone = run_arrays(one_fw, one_bw, offset)
    first, maps_first = run_arrays(np.concatenate([one_fw, other_fw[:1], other_fw[:1]]), np.concatenate([one_bw, other_bw[:1], other_bw[:1]]), offset)
    third, maps_third = run_arrays(np.concatenate([other_fw[:1], other_fw[:1], one_fw]), np.concatenate([other_bw[:1], other_bw[:1], one_bw]), offset)
    for d in range(2):
        assert np.array_equal(_bits(alone[d, 0]), _bits(first[d, 0])) and np.array_equal(_bits(alone[d, 0]), _bits(third[d, 2]))
        assert np.array_equal(_bits(alone[d, 0]), _bits(alone[d, 1]))               # the totals row of a batch of one
        for key in ("flags", "occ", "err", "warped"):
            assert np.array_equal(_bits(maps_alone[d][key][0]), _bits(maps_first[d][key][0])), key
            assert np.array_equal(_bits(maps_alone[d][key][0]), _bits(maps_third[d][key][2])), key
    again, maps_again = run_arrays(one_fw, one_bw, offset)                          # and from run to run
    assert np.array_equal(_bits(alone), _bits(again))
    assert all(np.array_equal(_bits(maps_alone[d][k]), _bits(maps_again[d][k])) for d in range(2) for k in maps_alone[d])


@pytest.mark.parametrize("name", list(SHAPES))
def test_optional_outputs_and_alignment_change_no_bit(name):
    with_maps, maps = _run(name, "ordinary")
    without, none = _run(name, "ordinary", outputs=False)
    assert none == [{}, {}] and np.array_equal(_bits(with_maps), _bits(without))
    if name.endswith("_offset1"):
        aligned, aligned_maps = _run(name.replace("_offset1", ""), "ordinary")
        assert np.array_equal(_bits(with_maps), _bits(aligned))
        assert all(np.array_equal(_bits(maps[d][k]), _bits(aligned_maps[d][k])) for d in range(2) for k in maps[d])
    # one output alone: the same bits as beside the others
    fw, bw = _inputs(name, "ordinary")
    N, _, H, W = fw.shape
    offset = SHAPES[name][1]
    ws_bytes, _ = CR.sizes(N, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    results = torch.empty(2 * (N + 1) * K, dtype=torch.float64, device="cuda")
    occ_bw = _dev(np.full((N, 1, H, W), 7.0, np.float32), offset)
    assert CR.call(_dev(np.asarray(fw), offset), _dev(np.asarray(bw), offset), fw.shape, results, ws, ws_bytes, occ=(None, occ_bw)) == CR.OK
    assert np.array_equal(_bits(occ_bw.cpu().numpy()), _bits(maps[1]["occ"])) and np.array_equal(_bits(results.cpu().numpy().reshape(2, N + 1, K)), _bits(with_maps))


def test_thresholds_are_arguments():
    fw, bw = _inputs("2x2x16x64", "ordinary")
    for alpha, beta in (((0.0, 0.0), (0.0, 0.0)), ((0.05, 2.0), (0.1, 0.5)), ((1e9, 1e9), (1e9, 1e9))):
        results, maps = run_arrays(fw, bw, alpha=alpha, beta=beta)
        ref = CR.ref32(fw, bw, alpha, beta)
        for d in range(2):
            assert np.array_equal(maps[d]["flags"], ref[d]["flags"]) and np.array_equal(results[d][:, CR.COUNT_COLUMNS], ref[d]["rows"][:, CR.COUNT_COLUMNS])
    assert not (maps[0]["flags"] & (FLAG["INCONSISTENT"] | FLAG["BOUNDARY"])).any()  # the last pair: nothing exceeds 1e9 |.|^2 + 1e9


def test_functional_feeds_flow_metrics():
    fw, bw = _inputs("2x2x36x60", "ordinary")
    ref = _reference("2x2x36x60", "ordinary")
    dfw, dbw = torch.from_numpy(np.array(fw)).cuda(), torch.from_numpy(np.array(bw)).cuda()
    c = Fn.flow_consistency(dfw, dbw)
    assert len(c) == 2 and c.flags_fw is None and c.err_bw is None and c.warped_fw is None
    assert np.array_equal(c.occ_fw.cpu().numpy(), ref[0]["occ"]) and np.array_equal(c.occ_bw.cpu().numpy(), ref[1]["occ"])
    assert np.array_equal(c.rows_fw[:, CR.COUNT_COLUMNS], ref[0]["rows"][:2, CR.COUNT_COLUMNS])
    s = c.summary()
    assert s["fw"]["occluded"] == ref[0]["rows"][2, COL["OCCLUDED"]] / ref[0]["rows"][2, COL["PIXELS"]] and 0 < s["fw"]["occluded"] < 0.5
    full = Fn.flow_consistency(dfw, dbw, flags=True, err=True, warped=True)
    assert np.array_equal(full.flags_bw.cpu().numpy(), ref[1]["flags"]) and _same_floats(full.err_fw.cpu().numpy(), ref[0]["err"])
    assert np.array_equal(_bits(full.rows_fw), _bits(c.rows_fw)) and np.array_equal(_bits(full.rows_bw), _bits(c.rows_bw))
    # the occlusion plane goes straight into the metrics: the matched / unmatched split exists without a mask file
    gt = torch.from_numpy(np.array(fw) + np.float32(0.25)).cuda()
    m = Fn.flow_metrics(dfw, gt, occ=c.occ_fw)
    assert np.array_equal(m.column("OCC_COUNT"), c.rows_fw[:, COL["OCCLUDED"]]) and m.summary()["epe_unmatched"] > 0
    with pytest.raises(RuntimeError, match="not differentiable"):
        Fn.flow_consistency(dfw.clone().requires_grad_(True), dbw)
    with pytest.raises(ValueError, match="must both be"):
        Fn.flow_consistency(dfw, dbw[:, :, :-1])
