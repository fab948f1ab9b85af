"""The point-trajectory kernels (csrc/flow_track.hip) through the C ABI of include/flownet2_hip_flow_track.h: tracks, last positions, states
and steps equal to the float32 restatement (flow_track_ref.ref32) bit for bit at every element, the counts equal, DISP_SUM within the
operation-count bound of a float64 evaluation, DISP_MAX exact; a dense one-frame call against fn2_flow_consistency's flags; one call
over T frames against T chained calls; the same bits for a sample alone and in a batch, from run to run, at both alignments and with or
without the optional outputs, inside sentinel-filled margins; the reseeding against its restatement; and FlowTracks.long_range_flow
feeding functional.flow_metrics and flow_to_color."""
import functools

import numpy as np
import pytest
import torch

import flow_track_ref as TR
from flownet2_amd import functional as Fn
from flownet2_amd import ops
from flownet2_amd.evaluate import CONSISTENCY_FLAGS as FLAG, TRACK_COL as COL, TRACK_K as K, TRACK_STOP as STOP

pytestmark = pytest.mark.gpu

MARGIN = 64                                                # elements of sentinel before and after every output
# name -> (N, T, H, W, P or None for the dense grid, float offset of every float blob inside its allocation).  One point per thread, a
# sample cut into ceil(P / 1024) <= 128 workgroups of 256 threads.
SHAPES = {
    "1x1x1x1": (1, 1, 1, 1, None, 0),
    "2x1x3x5": (2, 1, 3, 5, None, 0),
    "2x3x7x67_p100": (2, 3, 7, 67, 100, 0),               # sub-pixel starts
    "1x4x16x64": (1, 4, 16, 64, None, 0),                 # every pointer 16-byte aligned
    "1x4x16x64_offset1": (1, 4, 16, 64, None, 1),         # every float pointer advanced by one float: the same bits
    "3x2x33x67": (3, 2, 33, 67, None, 0),                 # P = 2211: three workgroups per sample, a ragged last one
}
ORDINARY_OF = {"2x3x7x67_p100": "subpixel", "1x4x16x64": "aligned", "3x2x33x67": "ragged"}
KINDS = ("zero", "shift", "edge", "negzero", "nonfinite", "badstart", "ordinary")
BIG_ALPHA = (1e9, 1e9)                                     # nothing is inconsistent: the edge targets are kept


def make_inputs(kind, name, seed):
    """-> dict(fw, bw, stop or None, points, state or None, alpha)."""
    N, T, H, W, P, _ = SHAPES[name]
    shape5 = (N, T, 2, H, W)
    points = TR.ordinary_case(ORDINARY_OF[name])[3] if name in ORDINARY_OF else TR.start_points(N, H, W, P, seed)
    out = dict(stop=None, state=None, alpha=TR.ALPHA, points=points)
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    if kind == "zero":
        return dict(out, fw=np.zeros(shape5, np.float32), bw=np.zeros(shape5, np.float32))
    if kind == "shift":
        fw, bw = np.zeros(shape5, np.float32), np.zeros(shape5, np.float32)
        fw[:, :, 0], bw[:, :, 0] = 1.0, -1.0
        fw[:, :, 1], bw[:, :, 1] = 0.5, -0.5
        return dict(out, fw=fw, bw=bw)
    if kind == "edge":
        # frame 0: even rows point exactly at (W - 1, H - 1), the right and bottom taps clamped onto the corner; odd rows at x2 = W - 0.25,
        # inside by a quarter of a pixel with the right tap clamped.  Later frames move the points that sit there by a small smooth flow.
        fw, bw, _ = TR.make_sequence((N, H, W), T, seed, marks=False, bad=False)
        fw, bw = (fw * np.float32(0.2)).astype(np.float32), (bw * np.float32(0.2)).astype(np.float32)
        odd = (np.arange(H) % 2 == 1)[:, None]
        fw[:, 0, 0] = np.where(odd, np.float32(W - 0.25) - x, np.float32(W - 1) - x)
        fw[:, 0, 1] = np.where(odd, np.float32(0), np.float32(H - 1) - y)
        points = np.floor(points) if P is not None else points                      # on the pixels, where the flow is exactly the target
        return dict(out, fw=fw, bw=bw, alpha=BIG_ALPHA, points=points.astype(np.float32))
    if kind == "negzero":
        fw, bw, _ = TR.make_sequence((N, H, W), T, seed, marks=False, bad=False)
        fw[:, 0] = -0.0
        bw[:, :, :, 0, :] = -0.0
        pts = points.copy()
        pts[:, :, ::3] = np.where(pts[:, :, ::3] < 1, np.float32(-0.0), pts[:, :, ::3])      # starts at -0.0f
        return dict(out, fw=fw, bw=(bw * np.float32(0.3)).astype(np.float32), points=pts)
    fw, bw, stop = TR.ordinary_case(ORDINARY_OF[name])[:3] if name in ORDINARY_OF else TR.make_sequence((N, H, W), T, seed)
    if kind == "nonfinite":
        rng = np.random.default_rng(seed + 77)
        bad = [np.nan, np.inf, -np.inf, 1e10, -1e10]
        fw, bw = fw.copy(), bw.copy()
        for t in (fw, bw):
            flat = t.reshape(N, T, 2, H * W)
            for k, pos in enumerate(rng.permutation(H * W)[:min(H * W, 12)]):
                flat[k % N, k % T, k % 2, pos] = bad[k % len(bad)]
        return dict(out, fw=fw, bw=bw, stop=stop)
    if kind == "badstart":
        pts = points.copy()
        starts = [(np.nan, 0), (0, np.nan), (np.inf, 0), (0, -np.inf), (1e10, 0), (0, -1e10), (-0.25, 0), (0, -0.25), (W, 0), (0, H), (W - 0.5, H - 0.5)]
        for k, (sx, sy) in enumerate(starts):
            pts[k % N, :, (k * 7) % pts.shape[2]] = (sx, sy)
        state = np.zeros((N, pts.shape[2]), np.uint8)
        state[:, 1::5] = TR.INC                                                      # and some points arrive stopped
        state[:, 3::7] = 0x80                                                        # with a value that is no reason of ours: passed through
        return dict(out, fw=fw, bw=bw, stop=stop, points=pts, state=state)
    return dict(out, fw=fw, bw=bw, stop=stop)


def _dev(a, offset=0):
    """A device copy of float32 array `a` that starts `offset` floats into its (256-byte aligned) allocation."""
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


_SENTINEL = {torch.float32: 7.0, torch.float64: 7.0, torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A}


def _out(shape, dtype, offset=0):
    """(allocation, view of `shape` inside it) filled with a sentinel, MARGIN elements before and after the view."""
    n = int(np.prod(shape))
    buf = torch.full((MARGIN + offset + n + MARGIN,), _SENTINEL[dtype], dtype=dtype, device="cuda")
    return buf, buf[MARGIN + offset:MARGIN + offset + n].view(shape)


def _margins_intact(buf, view):
    n, lead = view.numel(), (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    host = buf.cpu()
    return bool((host[:lead] == _SENTINEL[buf.dtype]).all() and (host[lead + n:] == _SENTINEL[buf.dtype]).all())


def run_arrays(fw, bw, points, stop=None, state=None, alpha=TR.ALPHA, stop_mask=TR.BOUNDARY, offset=0, outputs=("tracks", "points_out", "steps"),
               in_place=False):
    """One call in fresh allocations -> (rows [N + 1, K] float64, dict of host arrays).  Every output lies inside a sentinel margin that
    must come back untouched.  in_place: points_out = points and state_out = state_in."""
    N, T, _, H, W = fw.shape
    P = points.shape[2]
    dfw, dbw, dpts = _dev(np.asarray(fw), offset), _dev(np.asarray(bw), offset), _dev(np.asarray(points), offset)
    dstop = torch.from_numpy(np.array(stop)).cuda() if stop is not None else None
    dstate = torch.from_numpy(np.array(state)).cuda() if state is not None else None
    ws_bytes, _ = TR.sizes(N, T, H, W, P)
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    bufs = {"results": _out(((N + 1) * K,), torch.float64), "state": _out((N, P), torch.uint8)}
    if "tracks" in outputs:
        bufs["tracks"] = _out((N, T + 1, 2, P), torch.float32, offset)
    if "points_out" in outputs:
        bufs["points_out"] = _out((N, 2, P), torch.float32, offset)
    if "steps" in outputs:
        bufs["steps"] = _out((N, P), torch.int32)
    view = lambda k: bufs[k][1] if k in bufs else None
    if in_place:
        assert dstate is not None
        rc = TR.call(dfw, dbw, dpts, (N, T, H, W, P), view("results"), dstate, ws, ws_bytes, stop=dstop, stop_mask=stop_mask, state_in=dstate, alpha=alpha,
                     tracks=view("tracks"), points_out=dpts, steps=view("steps"))
    else:
        rc = TR.call(dfw, dbw, dpts, (N, T, H, W, P), view("results"), view("state"), ws, ws_bytes, stop=dstop, stop_mask=stop_mask, state_in=dstate,
                     alpha=alpha, tracks=view("tracks"), points_out=view("points_out"), steps=view("steps"))
    assert rc == TR.OK
    torch.cuda.synchronize()
    for k, (buf, v) in bufs.items():
        assert _margins_intact(buf, v), f"{k}: the margin around the output was written"
    host = {k: v.cpu().numpy() for k, (_, v) in bufs.items()}
    if in_place:
        host["points_out"], host["state"] = dpts.cpu().numpy(), dstate.cpu().numpy()
    return host.pop("results").reshape(N + 1, K), host


@functools.lru_cache(maxsize=None)
def _inputs(name, kind):
    base = name.replace("_offset1", "")
    d = make_inputs(kind, base, seed=1 + sorted(SHAPES).index(base) * 10 + KINDS.index(kind))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """ref32 of a case, computed once and shared."""
    d = _inputs(name, kind)
    return TR.ref32(d["fw"], d["bw"], d["points"], state=d["state"], stop=d["stop"], alpha=d["alpha"])


@functools.lru_cache(maxsize=None)
def _run(name, kind, outputs=("tracks", "points_out", "steps")):
    d = _inputs(name, kind)
    return run_arrays(d["fw"], d["bw"], d["points"], stop=d["stop"], state=d["state"], alpha=d["alpha"], offset=SHAPES[name][5], outputs=outputs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want):
    """Equal bit for bit where `want` is no NaN, NaN exactly where it is NaN (integers: equal)."""
    if want.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    isnan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), isnan) and np.array_equal(_bits(got)[~isnan], _bits(want)[~isnan]))


def _check_rows(rows, want_rows, points, got, label):
    assert np.isfinite(rows).all()
    assert np.array_equal(rows[:, TR.EXACT_COLUMNS], want_rows[:, TR.EXACT_COLUMNS]), f"{label}: counts differ from the restatement"
    ref64, bnd = TR.disp_sum_bound(points, got["points_out"], got["state"])
    e = np.abs(rows[:, COL["DISP_SUM"]] - ref64)
    print(f"{label}: DISP_SUM |err| {e.max():.3e}, worst err / bound {(e / np.maximum(bnd, 1e-300)).max():.3f}")
    assert np.all(e <= bnd)
    s32 = want_rows[:, COL["DISP_SUM"]]                                             # the float64 sum of the very float32 values: only the order differs
    assert np.all(np.abs(rows[:, COL["DISP_SUM"]] - s32) <= points.shape[0] * points.shape[2] * 2.0 ** -53 * s32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_outputs_and_rows_against_the_restatement(name, kind):
    d, ref = _inputs(name, kind), _reference(name, kind)
    rows, got = _run(name, kind)
    for key in ("state", "steps", "points_out", "tracks"):
        assert _same(got[key], ref[key]), f"{key}: {(_bits(got[key]) != _bits(ref[key])).sum()} elements differ"
    _check_rows(rows, ref["rows"], d["points"], got, f"{name} {kind}")


@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_flow_keeps_every_point_where_it_is(name):
    N, T, H, W, P, _ = SHAPES[name]
    d = _inputs(name, "zero")
    rows, got = _run(name, "zero")
    n = d["points"].shape[2]
    assert not got["state"].any() and np.all(got["steps"] == T) and np.array_equal(_bits(got["points_out"]), _bits(d["points"]))
    assert np.array_equal(_bits(got["tracks"]), _bits(np.broadcast_to(d["points"][:, None], (N, T + 1, 2, n))))
    want = np.zeros(K)
    want[[COL["POINTS"], COL["ALIVE"], COL["STEPS_SUM"], COL["STEPS_MAX"]]] = (n, n, n * T, T)
    assert np.array_equal(rows[:N], np.tile(want, (N, 1)))
    want[[COL["POINTS"], COL["ALIVE"], COL["STEPS_SUM"]]] = (N * n, N * n, N * n * T)
    assert np.array_equal(rows[N], want)


def test_a_constant_shift_walks_every_point_off_the_plane():
    """(+1, +0.5) per frame on a 16 x 64 plane, 4 frames: a point leaves through the right or the lower border, and not before."""
    name = "1x4x16x64"
    d = _inputs(name, "shift")
    _, got = _run(name, "shift")
    x, y = d["points"][0, 0], d["points"][0, 1]
    frames = np.minimum(np.minimum(np.ceil(64 - x) - 1, np.ceil((16 - y) / 0.5) - 1), 4).astype(np.int32)
    assert np.array_equal(got["steps"][0], frames) and np.array_equal(got["state"][0] != 0, frames < 4)
    assert np.all(got["state"][0][frames < 4] == STOP["OUTSIDE"])
    assert np.array_equal(got["points_out"][0, 0], x + frames) and np.array_equal(got["points_out"][0, 1], y + np.float32(0.5) * frames)


def test_edge_targets_clamp_their_taps():
    """x2 = W - 1 and y2 = H - 1 exactly, and x2 = W - 0.25: inside; from there the right / bottom taps are the last column / row."""
    name = "3x2x33x67"
    N, T, H, W, _, _ = SHAPES[name]
    _, got = _run(name, "edge")
    first = got["tracks"][:, 1].reshape(N, 2, H, W)
    assert np.all(first[:, 0, 0::2] == W - 1) and np.all(first[:, 1, 0::2] == H - 1)
    assert np.all(first[:, 0, 1::2] == np.float32(W - 0.25)) and np.all(first[:, 1, 1::2] == np.arange(H, dtype=np.float32)[1::2, None])
    assert (got["steps"] >= 1).all() and (got["steps"] == T).any()


def test_nonfinite_values_stop_the_point_and_its_samplers():
    name = "3x2x33x67"
    d = _inputs(name, "nonfinite")
    _, got = _run(name, "nonfinite")
    N, T, H, W, _, _ = SHAPES[name]
    own_bad = ~(np.abs(d["fw"][:, 0]) <= 1e9).all(1).reshape(N, -1)                  # a dense grid: the point's own flow in frame 0
    assert own_bad.sum() >= 3 and np.all(got["state"][own_bad] == STOP["NONFINITE"]) and np.all(got["steps"][own_bad] == 0)
    assert ((got["state"] == STOP["NONFINITE"]) & ~own_bad).any()                   # an otherwise finite point with a bad tap, or in a later frame


@pytest.mark.parametrize("name", ["2x1x3x5", "1x4x16x64", "1x4x16x64_offset1", "3x2x33x67"])
def test_a_dense_one_frame_call_against_the_consistency_kernel(name):
    """On all-finite flows: stopped exactly where flags_fw has NONFINITE, OUTSIDE or INCONSISTENT; the new position is grid + fw in float32
    bit for bit where alive; and with stop = flags_fw the MARKED points are the BOUNDARY pixels, every other point as before."""
    N, T, H, W, _, offset = SHAPES[name]
    fw, bw, _ = TR.make_sequence((N, H, W), 1, seed=31 + H, marks=False, bad=False)
    grid = TR.grid(N, H, W)
    dfw, dbw = _dev(fw[:, 0], offset), _dev(bw[:, 0], offset)
    flags = ops.flow_consistency(dfw, dbw, flags=True)[2][0].cpu().numpy()          # flags_fw [N,1,H,W]
    _, got = run_arrays(fw, bw, grid, offset=offset)
    occluded = (flags.reshape(N, -1) & (FLAG["NONFINITE"] | FLAG["OUTSIDE"] | FLAG["INCONSISTENT"])) != 0
    assert np.array_equal(got["state"] != 0, occluded) and 0 < occluded.sum() < occluded.size
    assert np.array_equal(got["state"][occluded], (flags.reshape(N, -1) & 7)[occluded])      # and for the same reason: they exclude one another
    moved = grid + fw[:, 0].reshape(N, 2, H * W)
    alive = np.broadcast_to(~occluded[:, None], moved.shape)
    assert np.array_equal(_bits(got["tracks"][:, 1])[alive], _bits(moved)[alive]) and np.isnan(got["tracks"][:, 1][~alive]).all()
    _, marked = run_arrays(fw, bw, grid, stop=flags[:, None], offset=offset)
    boundary = (flags.reshape(N, -1) & FLAG["BOUNDARY"]) != 0
    assert boundary.any() and np.array_equal(marked["state"] == STOP["MARKED"], boundary)
    assert np.array_equal(marked["state"][~boundary], got["state"][~boundary])
    assert np.array_equal(_bits(marked["points_out"])[:, 0][~boundary], _bits(got["points_out"])[:, 0][~boundary])


@pytest.mark.parametrize("kind", ["ordinary", "badstart"])
@pytest.mark.parametrize("name", ["2x3x7x67_p100", "1x4x16x64", "1x4x16x64_offset1", "3x2x33x67"])
def test_one_call_over_T_frames_equals_T_chained_calls(name, kind):
    d = _inputs(name, kind)
    N, T, H, W, _, offset = SHAPES[name]
    rows, whole = _run(name, kind)
    points, state = np.array(d["points"]), (np.array(d["state"]) if d["state"] is not None else np.zeros(whole["state"].shape, np.uint8))
    steps, tracks, reasons = np.zeros_like(whole["steps"]), [points], np.zeros((N + 1, 4))
    cols = [COL[n] for n in ("NONFINITE", "OUTSIDE", "INCONSISTENT", "MARKED")]
    for t in range(T):
        before = points
        r, got = run_arrays(d["fw"][:, t:t + 1], d["bw"][:, t:t + 1], points, stop=d["stop"][:, t:t + 1], state=state, alpha=d["alpha"], offset=offset,
                            in_place=t % 2 == 1)                                    # every other step in place: points_out = points
        points, state = got["points_out"], got["state"]
        steps += got["steps"]
        tracks.append(got["tracks"][:, 1])
        reasons += r[:, cols]
        assert np.array_equal(_bits(got["tracks"][:, 0]), _bits(before))            # a call's first frame is the points it was given
    assert _same(points, whole["points_out"]) and np.array_equal(state, whole["state"]) and np.array_equal(steps, whole["steps"])
    assert np.array_equal(reasons, rows[:, cols])
    # a chained call starts a stopped point's frame with its last position and NaN after; the whole call has NaN from the stop on
    chained = np.stack(tracks, 1)
    reached = ~np.isnan(whole["tracks"])
    assert np.array_equal(_bits(chained)[reached], _bits(whole["tracks"])[reached]) and np.isnan(chained[~reached]).all()


@pytest.mark.parametrize("name", ["2x3x7x67_p100", "3x2x33x67", "1x4x16x64_offset1"])
def test_a_sample_has_the_same_bits_alone_and_in_any_batch(name):
    d, o = _inputs(name, "ordinary"), _inputs(name, "nonfinite")
    offset = SHAPES[name][5]
    one = lambda k, src=d: src[k][:1]
    cat = lambda k, order: np.concatenate([one(k, s) for s in order])
    call = lambda order: run_arrays(cat("fw", order), cat("bw", order), cat("points", order), stop=cat("stop", order), offset=offset)
    alone, maps_alone = call([d])
    first, maps_first = call([d, o, o])
    third, maps_third = call([o, o, d])
    assert np.array_equal(_bits(alone[0]), _bits(first[0])) and np.array_equal(_bits(alone[0]), _bits(third[2]))
    assert np.array_equal(_bits(alone[0]), _bits(alone[1]))                         # the totals row of a batch of one
    for key in ("tracks", "points_out", "state", "steps"):
        assert np.array_equal(_bits(maps_alone[key][0]), _bits(maps_first[key][0])), key
        assert np.array_equal(_bits(maps_alone[key][0]), _bits(maps_third[key][2])), key
    again, maps_again = call([d])                                                   # and from run to run
    assert np.array_equal(_bits(alone), _bits(again)) and all(np.array_equal(_bits(maps_alone[k]), _bits(maps_again[k])) for k in maps_alone)


@pytest.mark.parametrize("name", list(SHAPES))
def test_optional_outputs_and_alignment_change_no_bit(name):
    rows, full = _run(name, "ordinary")
    for outputs in ((), ("tracks",), ("points_out",), ("steps",)):
        r, got = _run(name, "ordinary", outputs=outputs)
        assert set(got) == set(outputs) | {"state"} and np.array_equal(_bits(r), _bits(rows))
        assert all(np.array_equal(_bits(got[k]), _bits(full[k])) for k in got)
    if name.endswith("_offset1"):
        aligned_rows, aligned = _run(name.replace("_offset1", ""), "ordinary")
        assert np.array_equal(_bits(rows), _bits(aligned_rows)) and all(np.array_equal(_bits(full[k]), _bits(aligned[k])) for k in full)


def test_thresholds_and_mask_are_arguments():
    d = _inputs("1x4x16x64", "ordinary")
    for alpha, mask in (((0.0, 0.0), TR.BOUNDARY), ((0.05, 2.0), 1 | 2), (BIG_ALPHA, 0), (TR.ALPHA, 0xFF)):
        rows, got = run_arrays(d["fw"], d["bw"], d["points"], stop=d["stop"], alpha=alpha, stop_mask=mask)
        ref = TR.ref32(d["fw"], d["bw"], d["points"], stop=d["stop"], alpha=alpha, stop_mask=mask)
        assert np.array_equal(got["state"], ref["state"]) and _same(got["tracks"], ref["tracks"])
        assert np.array_equal(rows[:, TR.EXACT_COLUMNS], ref["rows"][:, TR.EXACT_COLUMNS])
        if mask == 0:
            assert rows[1, COL["INCONSISTENT"]] == 0 and rows[1, COL["MARKED"]] == 0 and rows[1, COL["NONFINITE"]] > 0


# ---- reseeding ---------------------------------------------------------------------------------------------------------------------------
def run_reseed(points, state, size, cell, born=True):
    N, _, P = points.shape
    bufs = {"points": _out((N, 2, P), torch.float32), "state": _out((N, P), torch.uint8)}
    if born:
        bufs["born"] = _out((N, P), torch.uint8)
    bufs["points"][1].copy_(torch.from_numpy(np.array(points)))
    bufs["state"][1].copy_(torch.from_numpy(np.array(state)))
    ws_buf, ws = _out((N * P,), torch.uint8)
    view = lambda k: bufs[k][1] if k in bufs else None
    assert TR.call_reseed(view("points"), view("state"), view("born"), N, size[0], size[1], cell, ws, N * P) == TR.OK
    torch.cuda.synchronize()
    for k, (buf, v) in list(bufs.items()) + [("workspace", (ws_buf, ws))]:
        assert _margins_intact(buf, v), f"{k}: the margin was written"
    return tuple(view(k).cpu().numpy() if k in bufs else None for k in ("points", "state", "born"))


@pytest.mark.parametrize("N,H,W,cell", [(1, 36, 60, 4), (2, 5, 7, 2), (1, 3, 5, 1), (2, 33, 67, 8)])
def test_reseed_against_the_restatement(N, H, W, cell):
    ch, cw = TR.cells(H, W, cell)
    P = ch * cw
    # every slot stopped: the grid
    junk = np.full((N, 2, P), np.nan, np.float32)
    p0, s0, b0 = run_reseed(junk, np.full((N, P), STOP["OUTSIDE"], np.uint8), (H, W), cell)
    assert np.array_equal(_bits(p0), _bits(TR.grid(N, H, W, cell))) and not s0.any() and b0.all()
    grid_t = Fn.flow_track_grid(N, H, W, cell)
    assert grid_t.shape == (N, 2, P) and np.array_equal(_bits(grid_t.cpu().numpy()), _bits(p0))
    # one tracker step on an ordinary sequence loses points; some wander into a neighbour's cell
    fw, bw, stop = TR.make_sequence((N, H, W), 1, seed=H + cell)
    fw = (fw * np.float32(max(1.0, cell / 2))).astype(np.float32)
    moved = TR.ref32(fw, bw, p0, stop=stop)
    points, state = moved["points_out"].copy(), moved["state"].copy()
    points[:, :, P // 2] = (np.nan, 1e10)                                            # an alive slot with no position covers nothing and keeps its slot
    state[:, P // 2] = 0
    points[:, :, 0], state[:, 0] = p0[:, :, 1], 0                                    # slot 0 sits on cell 1's centre, and slot 1 has stopped:
    state[:, 1] = STOP["INCONSISTENT"]                                               # cell 1 is covered, cell 0's slot is busy
    want_p, want_s, want_b = TR.reseed32(points, state, (H, W), cell)
    got_p, got_s, got_b = run_reseed(points, state, (H, W), cell)
    assert _same(got_p, want_p) and np.array_equal(got_s, want_s) and np.array_equal(got_b, want_b)
    assert 0 < want_b.sum() and np.array_equal(got_b != 0, (state != 0) & (got_s == 0))      # born marks exactly the new slots
    assert np.all(want_s[:, 1] == STOP["INCONSISTENT"]) and not want_b[:, :2].any()   # slot 1 stays stopped, cell 0 stays uncovered
    # born is optional and changes nothing; a second reseed changes nothing
    alone_p, alone_s, none = run_reseed(points, state, (H, W), cell, born=False)
    assert none is None and _same(alone_p, got_p) and np.array_equal(alone_s, got_s)
    again_p, again_s, again_b = run_reseed(got_p, got_s, (H, W), cell)
    assert _same(again_p, got_p) and np.array_equal(again_s, got_s) and not again_b.any()
    # the Python wrapper, in place
    tp, ts = torch.from_numpy(points).cuda(), torch.from_numpy(state).cuda()
    born = Fn.flow_track_reseed(tp, ts, (H, W), cell)
    assert _same(tp.cpu().numpy(), want_p) and np.array_equal(ts.cpu().numpy(), want_s) and np.array_equal(born.cpu().numpy(), want_b)
    with pytest.raises(ValueError, match="must be contiguous float32"):
        Fn.flow_track_reseed(tp[:, :, :-1], ts, (H, W), cell)


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_functional_flow_track_merge_and_long_range_flow():
    name = "1x4x16x64"
    d, ref = _inputs(name, "ordinary"), _reference(name, "ordinary")
    N, T, H, W, _, _ = SHAPES[name]
    fw, bw, stop = (torch.from_numpy(np.array(d[k])).cuda() for k in ("fw", "bw", "stop"))
    t = Fn.flow_track(fw, bw, stop=stop)                                            # points=None: the dense grid
    assert len(t) == N and t.size == (H, W) and tuple(t.tracks.shape) == (N, T + 1, 2, H * W)
    for key, got in (("tracks", t.tracks), ("points_out", t.points), ("state", t.state), ("steps", t.steps)):
        assert _same(got.cpu().numpy(), ref[key]), key
    assert np.array_equal(t.rows[:, TR.EXACT_COLUMNS], ref["rows"][:N, TR.EXACT_COLUMNS])
    s = t.summary()
    assert s["alive"] == ref["rows"][N, COL["ALIVE"]] / (N * H * W) and 0.25 <= s["alive"] < 1 and s["steps_max"] == T
    assert Fn.flow_track(fw, bw, stop=stop, tracks=False).tracks is None
    # [N,2,H,W] flows are one step; consecutive calls merge into the whole
    calls, points, state = [], None, None
    for k in range(T):
        c = Fn.flow_track(fw[:, k], bw[:, k], points=points, state=state, stop=stop[:, k])
        points, state = c.points, c.state
        calls.append(c)
    m = calls[0].merge(calls[1:])
    for key, got in (("points_out", m.points), ("state", m.state), ("steps", m.steps)):
        assert _same(got.cpu().numpy(), ref[key]), key
    assert np.array_equal(m.rows[:, TR.EXACT_COLUMNS], t.rows[:, TR.EXACT_COLUMNS]) and tuple(m.tracks.shape) == tuple(t.tracks.shape)
    assert np.all(np.abs(m.rows[:, COL["DISP_SUM"]] - t.rows[:, COL["DISP_SUM"]]) <= H * W * 2.0 ** -53 * t.rows[:, COL["DISP_SUM"]])
    # the long-range flow: last position minus grid where alive, the unknown-flow value where stopped; flow_metrics and flow_to_color
    # leave the stopped points out
    lr = t.long_range_flow()
    assert tuple(lr.shape) == (N, 2, H, W) and lr.is_cuda
    alive = ref["state"].reshape(N, H, W) == 0
    want = (ref["points_out"] - TR.grid(N, H, W)).reshape(N, 2, H, W)
    host = lr.cpu().numpy()
    assert np.array_equal(_bits(host)[:, 0][alive], _bits(want)[:, 0][alive]) and np.all(host[:, 0][~alive] == np.float32(1e10))
    assert np.all(host[:, 1][~alive] == np.float32(1e10))
    met = Fn.flow_metrics(lr + 0.25, lr)                                            # gt = the long-range flow: unknown where stopped
    assert np.array_equal(met.column("VALID"), alive.reshape(N, -1).sum(1)) and abs(met.summary()["epe"] - 0.25 * np.sqrt(2)) < 1e-5
    rgb = Fn.flow_to_color(lr).cpu().numpy()
    assert rgb.shape == (N, H, W, 3) and not rgb[~alive].any() and rgb[alive].any()      # unknown flow is drawn black
    with pytest.raises(ValueError, match="must be"):
        Fn.flow_track(fw, bw, points=torch.zeros(N + 1, 2, 5, device="cuda"))
    with pytest.raises(ValueError, match="expected uint8"):
        Fn.flow_track(fw, bw, stop=stop.float())
