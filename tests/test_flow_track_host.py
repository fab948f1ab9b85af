"""Point trajectories, everything that needs no GPU: the header and its binding, the host-only entry point and the refusals of
include/flownet2_hip_flow_track.h, the float32 restatement against a 3 x 4 example worked by hand, FlowTracks.merge / summary /
long_range_flow, the restatement of the reseeding on a 5 x 7 plane, the validity of the sequences the GPU test calls ordinary, the npz
layout and the runner's output names."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flow_track_ref as TR
from flownet2_amd import _lib, evaluate
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import TRACK_COL as COL, TRACK_COLUMNS, TRACK_K as K, TRACK_STOP, FlowTracks

WANT_COLUMNS = ["POINTS", "ALIVE", "NONFINITE", "OUTSIDE", "INCONSISTENT", "MARKED", "STEPS_SUM", "STEPS_MAX", "DISP_SUM", "DISP_MAX"]
NF, OUT, INC, MARK = 1, 2, 4, 8
nan = np.float32(np.nan)


def row(**kw):
    out = np.zeros(K)
    for k, v in kw.items():
        out[COL[k]] = v
    return out


# ---- the header, the binding, sizes and refusals ----------------------------------------------------------------------------------
def test_header_declares_exactly_what_the_library_exports():
    with open(os.path.join(_lib.INCLUDE_DIR, "flownet2_hip_flow_track.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    want = ["fn2_flow_track_sizes", "fn2_flow_track", "fn2_flow_track_reseed"]
    assert re.findall(r"\b(fn2_\w+)\s*\(", body) == want and list(_lib.FLOW_TRACK_EXPORTS) == want
    assert "typedef" not in body                                                    # no structure: _STRUCTS keeps its size
    symbols = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode().split()
    assert sorted(s for s in symbols if s.startswith("fn2_flow_track")) == sorted(want)
    L = _lib.lib()
    for name in want:
        restype, argtypes = _lib.FLOW_TRACK_PROTOTYPES[name]
        assert restype is C.c_int and getattr(L, name).argtypes == argtypes
    args = _lib.FLOW_TRACK_PROTOTYPES["fn2_flow_track"][1]
    assert len(args) == 21 and args[2] is C.c_void_p and args[3] is C.c_uint and args[13] is C.c_void_p      # stop, stop_mask, results
    assert len(_lib.FLOW_TRACK_PROTOTYPES["fn2_flow_track_reseed"][1]) == 10 and len(_lib.FLOW_TRACK_PROTOTYPES["fn2_flow_track_sizes"][1]) == 7
    # the enums reach the binding through the parser, in a table of their own; every other table keeps its size
    enum = _lib.FLOW_TRACK_CONSTANTS
    assert [enum["FN2_FLOW_TRACK_" + n] for n in WANT_COLUMNS] == list(range(10)) and enum["FN2_FLOW_TRACK_K"] == 10 and len(enum) == 15
    assert TRACK_STOP == dict(NONFINITE=NF, OUTSIDE=OUT, INCONSISTENT=INC, MARKED=MARK)
    assert len(_lib.CONSTANTS) == 49 and len(_lib.EXPORTS) == 159 and len(_lib._STRUCTS) == 11 and len(_lib.FLOW_METRICS_CONSTANTS) == 16
    assert len(_lib.FLOW_CONSISTENCY_CONSTANTS) == 13
    others = set(_lib.CONSTANTS) | set(_lib.FLOW_METRICS_CONSTANTS) | set(_lib.FLOW_CONSISTENCY_CONSTANTS) | set(_lib.FLOW_VISUALIZE_CONSTANTS)
    assert not set(enum) & others
    assert not set(want) & (set(_lib.PROTOTYPES) | set(_lib.FLOW_CONSISTENCY_PROTOTYPES) | set(_lib.FLOW_VISUALIZE_PROTOTYPES))
    lengths = [len(t) for t in (_lib.EXPORTS, _lib.SOLVER_EXPORTS, _lib.CORR_ROUTE_EXPORTS, _lib.CONV_GENERAL_EXPORTS, _lib.CONV_GEOMETRY_EXPORTS,
                                _lib.CONV_VOLUME_EXPORTS, _lib.LPQ_LOSS_EXPORTS, _lib.FLOW_METRICS_EXPORTS)]
    assert sum(lengths) == len(_lib.PROTOTYPES)                                     # the first eight headers, as before
    assert list(TRACK_COLUMNS) == WANT_COLUMNS and K == 10 and TR.sizes(1, 1, 1, 1, 1)[1] == 10
    # the stop reasons are the consistency kernel's flag bits where both have the reason, and MARKED is the bit of the default mask
    flags = evaluate.CONSISTENCY_FLAGS
    assert all(TRACK_STOP[n] == flags[n] for n in ("NONFINITE", "OUTSIDE", "INCONSISTENT")) and TR.BOUNDARY == flags["BOUNDARY"]
    # the header states the invariant the border tests hold
    assert "nothing outside [0,W) x [0,H) of the point's own sample is ever read" in " ".join(text.replace("*", " ").split())


def test_sizes_grow_with_the_points_and_are_per_sample():
    """max(8 K N B, N P) bytes with B = min(ceil(P / 1024), 128): the partial rows of the tracker or the coverage bytes of the reseed."""
    counts = [1, 35, 80, 81, 1024, 1025, 4096, 143360, 1 << 20]
    per_sample = [TR.sizes(1, 1, 2048, 2048, p)[0] for p in counts]
    assert per_sample == [max(8 * K * min(-(-p // 1024), 128), p) for p in counts] and per_sample == sorted(per_sample)
    assert per_sample[:6] == [80, 80, 80, 81, 1024, 1025] and per_sample[-1] == 1 << 20
    for p, one in zip(counts, per_sample):
        for n in (2, 3, 17):
            assert TR.sizes(n, 3, 2048, 2048, p)[0] == n * one                      # T and the plane do not enter
    L = _lib.lib()
    assert L.fn2_flow_track_sizes(2, 3, 5, 7, 35, None, None) == TR.OK              # either out-pointer may be NULL
    nbytes = C.c_size_t(77)
    for shape in ((0, 1, 5, 7, 35), (2, 0, 5, 7, 35), (2, 1, 5, 7, 0), (1 << 5, 1 << 5, 1 << 10, 1 << 10, 35), (2, 3, 5, 7, 1 << 28),
                  (1 << 21, 1 << 21, 1 << 11, 1 << 10, 35)):
        assert L.fn2_flow_track_sizes(*shape, C.byref(nbytes), None) == TR.INVALID and nbytes.value == 77


def test_every_host_refusal_writes_nothing_and_names_the_argument():
    """Refusals are decided before any launch, so they need no device: the pointers are host buffers that nobody dereferences."""
    ws_bytes, _ = TR.sizes(2, 3, 5, 7, 35)
    assert ws_bytes == 2 * K * 8
    buf = lambda n: (C.c_ubyte * n)(*([0x5A] * n))
    flow, pts = 2 * 3 * 2 * 35 * 4, 2 * 2 * 35 * 4
    bufs = {k: buf(n) for k, n in (("fw", flow), ("bw", flow), ("stop", 210), ("points", pts), ("state_in", 70), ("results", 3 * K * 8),
                                   ("tracks", 4 * pts), ("points_out", pts), ("state_out", 70), ("steps", 280), ("born", 70), ("ws", ws_bytes))}
    cases = TR.refusals(bufs, ws_bytes)
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels) == 29
    for label, want, names, prefix, thunk in cases:
        assert thunk() == want, label
        text = _lib.lib().fn2_last_error_string().decode()
        assert text.startswith(prefix) and names in text, (label, text)
    for k, b in bufs.items():
        assert bytes(b) == b"\x5a" * len(b), k


def test_python_refusals_need_no_device():
    z = torch.zeros(1, 2, 3, 4)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.flow_track(z, z, points=torch.zeros(1, 2, 5))
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.flow_track(z, z)                                                         # the dense grid would be made on the flows' device
    with pytest.raises(RuntimeError, match="not differentiable"):
        Fn.flow_track(z.clone().requires_grad_(True), z, points=torch.zeros(1, 2, 5))
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.flow_track_reseed(torch.zeros(1, 2, 12), torch.zeros(1, 12, dtype=torch.uint8), (5, 7), 2)
    with pytest.raises(ValueError, match="N,T,2,H,W"):
        Fn.flow_track(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))
    import flownet2_amd
    assert flownet2_amd.flow_track is Fn.flow_track and flownet2_amd.FlowTracks is FlowTracks
    assert flownet2_amd.flow_track_reseed is Fn.flow_track_reseed and flownet2_amd.flow_track_grid is Fn.flow_track_grid
    assert all(n in flownet2_amd.__all__ for n in ("flow_track", "flow_track_reseed", "flow_track_grid", "FlowTracks"))


# ---- the restatement on a case worked by hand ------------------------------------------------------------------------------------------
def _hand_case():
    """3 x 4, two frames, (+1, 0) forward and (-1, 0) backward everywhere, but: bw[0] is (-3, 0) at (x, y) = (1, 2); fw[1] has the
    unknown-flow value 1e10 in u at (2, 2); stop[1] carries the BOUNDARY bit (and stop[0] only other bits) at (2, 1)."""
    fw = np.zeros((1, 2, 2, 3, 4), np.float32)
    fw[0, :, 0] = 1.0
    fw[0, 1, 0, 2, 2] = 1e10
    bw = np.zeros((1, 2, 2, 3, 4), np.float32)
    bw[0, :, 0] = -1.0
    bw[0, 0, 0, 2, 1] = -3.0
    stop = np.zeros((1, 2, 1, 3, 4), np.uint8)
    stop[0, 0] = 7
    stop[0, 1, 0, 1, 2] = 8 | 1
    #                 A    B    C       D    E    F    G    H
    x = np.array([0.0, 2.5, np.nan, 0.0, 0.5, 1.0, 4.0, 1.0], np.float32)
    y = np.array([0.0, 1.0, 0.0,    2.0, 1.0, 2.0, 1.0, 1.0], np.float32)
    state = np.array([[0, 0, 0, 0, 0, 0, 0, INC]], np.uint8)
    return fw, bw, stop, np.stack([x, y])[None], state


def test_restatement_on_a_3x4_case_worked_by_hand():
    """A (0, 0) walks to (1, 0) and (2, 0): alive, 2 steps, displacement 2.  B (2.5, 1) reaches (3.5, 1) -- its backward sample takes the
    clamped column 3 twice -- and then points to x2 = 4.5: OUTSIDE after 1 step, staying at (3.5, 1).  C starts at NaN: NONFINITE, 0 steps.
    D (0, 2) points to (1, 2), where bw is (-3, 0): s = 4 > 0.01 * 10 + 0.5, INCONSISTENT, 0 steps.  E (0.5, 1) reaches (1.5, 1), whose
    nearest pixel (2, 1) is marked in frame 1 (its lower taps, one of them the 1e10, carry weight 0 and 0 * 1e10 is 0): MARKED after 1 step.
    F (1, 2) reaches (2, 2), where fw[1] is 1e10: NONFINITE after 1 step.  G starts at x = W: OUTSIDE, 0 steps.  H arrives stopped
    (INCONSISTENT) and passes through: in no count but POINTS."""
    fw, bw, stop, points, state = _hand_case()
    r = TR.ref32(fw, bw, points, state=state, stop=stop)
    assert r["state"].tolist() == [[0, OUT, NF, INC, MARK, NF, OUT, INC]] and r["steps"].tolist() == [[2, 1, 0, 0, 1, 1, 0, 0]]
    assert r["state"].dtype == np.uint8 and r["steps"].dtype == np.int32 and r["tracks"].dtype == np.float32 and r["points_out"].dtype == np.float32
    want_x = np.array([[0, 2.5, nan, 0, 0.5, 1, 4, 1], [1, 3.5, nan, nan, 1.5, 2, nan, nan], [2, nan, nan, nan, nan, nan, nan, nan]], np.float32)
    want_y = np.array([[0, 1, 0, 2, 1, 2, 1, 1], [0, 1, nan, nan, 1, 2, nan, nan], [0, nan, nan, nan, nan, nan, nan, nan]], np.float32)
    assert np.array_equal(r["tracks"][0, :, 0], want_x, equal_nan=True) and np.array_equal(r["tracks"][0, :, 1], want_y, equal_nan=True)
    assert np.array_equal(r["points_out"][0], np.array([[2, 3.5, nan, 0, 1.5, 2, 4, 1], [0, 1, 0, 2, 1, 2, 1, 1]], np.float32), equal_nan=True)
    want = row(POINTS=8, ALIVE=1, NONFINITE=2, OUTSIDE=2, INCONSISTENT=1, MARKED=1, STEPS_SUM=5, STEPS_MAX=2, DISP_SUM=2.0, DISP_MAX=2.0)
    assert np.array_equal(r["rows"], np.stack([want, want]))
    # without the stop map, or with a mask that leaves the bit out, E walks on to (2.5, 1); with mask 1 it stops in frame 0 (stop[0] is 7)
    for kw in (dict(stop=None), dict(stop=stop, stop_mask=16)):
        q = TR.ref32(fw, bw, points, state=state, **kw)
        assert q["state"][0, 4] == 0 and q["steps"][0, 4] == 2 and q["points_out"][0, :, 4].tolist() == [2.5, 1.0]
    q = TR.ref32(fw, bw, points, state=state, stop=stop, stop_mask=1)
    assert q["state"].tolist() == [[MARK, MARK, NF, MARK, MARK, MARK, OUT, INC]] and q["steps"].sum() == 0
    # the float64 evaluation agrees with the float32 sum within its own bound, and the bound is small
    ref, bnd = TR.disp_sum_bound(points, r["points_out"], r["state"])
    assert np.all(np.abs(r["rows"][:, COL["DISP_SUM"]] - ref) <= bnd) and np.all(bnd <= 1e-5 * ref) and np.all(bnd > 0)


def test_restatement_never_converts_what_it_must_not():
    """NaN, +-Inf, 1e10 and positions off the plane as start points, and the same as flow values: no warning from a conversion."""
    import warnings
    fw, bw, stop, _, _ = _hand_case()
    pts = np.array([[[np.nan, np.inf, -np.inf, 1e10, -1e10, -0.25, 4.0, 1.0, 1.0]], [[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0, -1e-3]]], np.float32).reshape(1, 2, 9)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = TR.ref32(fw, bw, pts, stop=stop)
        assert r["state"].tolist() == [[NF, NF, NF, NF, NF, OUT, OUT, OUT, OUT]] and r["steps"].sum() == 0
        assert np.array_equal(r["points_out"], pts, equal_nan=True) and np.isnan(r["tracks"][:, 1:]).all()
        for bad in (np.nan, np.inf, -np.inf, 1e10, -1e10):
            f2, b2 = fw.copy(), bw.copy()
            f2[0, 0, 1, 0, 0] = bad
            b2[0, 0, 0, 1, 2] = bad
            q = TR.ref32(f2, b2, TR.grid(1, 3, 4), stop=None)
            assert q["state"][0, 0] == NF and q["state"][0, 4 + 1] == NF, bad          # (0, 0) by its own flow, (1, 1) by its backward sample


# ---- FlowTracks ------------------------------------------------------------------------------------------------------------------------
def _tracks_of(r, points, size):
    return FlowTracks(r["rows"][:-1], tracks=r["tracks"], points=r["points_out"], state=r["state"], steps=r["steps"], start=points, size=size)


def test_merge_summary_and_long_range_flow_by_hand():
    fw, bw, stop, points, state = _hand_case()
    whole = _tracks_of(TR.ref32(fw, bw, points, state=state, stop=stop), points, (3, 4))
    r0 = TR.ref32(fw[:, :1], bw[:, :1], points, state=state, stop=stop[:, :1])
    r1 = TR.ref32(fw[:, 1:], bw[:, 1:], r0["points_out"], state=r0["state"], stop=stop[:, 1:])
    a, b = _tracks_of(r0, points, (3, 4)), _tracks_of(r1, r0["points_out"], (3, 4))
    assert a.rows[0].tolist() == row(POINTS=8, ALIVE=4, NONFINITE=1, OUTSIDE=1, INCONSISTENT=1, STEPS_SUM=4, STEPS_MAX=1, DISP_SUM=4.0, DISP_MAX=1.0).tolist()
    assert b.rows[0].tolist() == row(POINTS=8, ALIVE=1, NONFINITE=1, OUTSIDE=1, MARKED=1, STEPS_SUM=1, STEPS_MAX=1, DISP_SUM=1.0, DISP_MAX=1.0).tolist()
    m = a.merge([b])
    assert np.array_equal(m.rows, whole.rows) and len(m) == 1 and len(a) == 1
    assert np.array_equal(np.asarray(m.tracks), whole.tracks, equal_nan=True) and np.array_equal(np.asarray(m.steps), whole.steps)
    assert np.array_equal(np.asarray(m.state), whole.state) and np.array_equal(np.asarray(m.points), whole.points, equal_nan=True)
    assert np.array_equal(np.asarray(m.start), points, equal_nan=True) and m.size == (3, 4)
    s = m.summary()
    assert list(s) == ["alive", "nonfinite", "outside", "inconsistent", "marked", "steps_mean", "steps_max", "disp_mean", "disp_max", "points", "samples",
                       "alpha"]
    assert s == dict(alive=1 / 8, nonfinite=2 / 8, outside=2 / 8, inconsistent=1 / 8, marked=1 / 8, steps_mean=5 / 8, steps_max=2.0, disp_mean=2.0,
                     disp_max=2.0, points=8, samples=1, alpha=[0.01, 0.5])
    empty = FlowTracks().summary()
    assert math.isnan(empty["alive"]) and math.isnan(empty["disp_mean"]) and empty["samples"] == 0
    with pytest.raises(ValueError, match="must be"):
        FlowTracks(np.zeros((2, K + 1)))
    with pytest.raises(ValueError, match="calls differ"):
        a.merge([FlowTracks(b.rows, points=b.points, state=b.state, steps=b.steps, start=b.start, size=(3, 4), alpha=(0.02, 0.5))])
    with pytest.raises(ValueError, match="needs the points"):
        a.merge([FlowTracks(b.rows, size=(3, 4))])
    with pytest.raises(ValueError, match="no dense grid"):
        m.long_range_flow()
    # a dense grid: the flow to the last frame where the point is alive, the .flo unknown-flow value where it stopped
    grid = TR.grid(1, 3, 4)
    assert grid[0, 0].reshape(3, 4)[1].tolist() == [0, 1, 2, 3] and grid[0, 1].reshape(3, 4)[:, 2].tolist() == [0, 1, 2]
    d = _tracks_of(TR.ref32(fw, bw, grid, stop=stop), grid, (3, 4))
    lr = d.long_range_flow()
    assert lr.shape == (1, 2, 3, 4) and lr.dtype == np.float32
    big = np.float32(1e10)
    assert np.array_equal(lr[0, 0], np.array([[2, 2, big, big], [2, big, big, big], [big, big, big, big]], np.float32))
    assert np.array_equal(lr[0, 1], np.where(lr[0, 0] == big, big, np.float32(0)))
    t = FlowTracks(d.rows, points=torch.from_numpy(d.points), state=torch.from_numpy(d.state), start=torch.from_numpy(grid), size=(3, 4))
    assert isinstance(t.long_range_flow(), torch.Tensor) and np.array_equal(t.long_range_flow().numpy(), lr)


# ---- reseeding ---------------------------------------------------------------------------------------------------------------------------
def test_reseed_restatement_on_a_5x7_plane():
    """cell = 2: 3 x 4 cells, the last column one pixel wide and the last row one pixel high, so their centres are clamped to 6 and 4."""
    points, state, born = TR.reseed32(np.full((1, 2, 12), 77, np.float32), np.full((1, 12), OUT, np.uint8), (5, 7), 2)
    assert points[0, 0].reshape(3, 4).tolist() == [[0.5, 2.5, 4.5, 6.0]] * 3 and points[0, 1].reshape(3, 4).T.tolist() == [[0.5, 2.5, 4.0]] * 4
    assert not state.any() and born.all()                                           # every slot stopped: the grid
    assert np.array_equal(TR.grid(1, 5, 7, 2), points)
    # slot 0 wanders into cell 1; slots 1 and 5 stop; slot 7 is alive at NaN (it covers nothing and keeps its slot); slot 11 stops while
    # slot 10 sits in cell 11
    points[0, :, 0] = (2.2, 0.3)
    points[0, :, 7] = (np.nan, 2.5)
    points[0, :, 10] = (6.5, 4.9)
    state[0, [1, 5, 11]] = (INC, OUT, MARK)
    before = points.copy()
    p2, s2, b2 = TR.reseed32(points, state, (5, 7), 2)
    assert b2.tolist() == [[0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]]                    # cell 1 is covered by slot 0, cell 11 by slot 10
    assert s2.tolist() == [[0, INC, 0, 0, 0, 0, 0, 0, 0, 0, 0, MARK]] and p2[0, :, 5].tolist() == [2.5, 2.5]
    keep = np.arange(12) != 5
    assert np.array_equal(p2[:, :, keep], before[:, :, keep], equal_nan=True)
    # cell 0 (home of the busy slot 0) and cell 10 stay uncovered: a second reseed changes nothing
    p3, s3, b3 = TR.reseed32(p2, s2, (5, 7), 2)
    assert np.array_equal(p3, p2, equal_nan=True) and np.array_equal(s3, s2) and not b3.any()
    assert TR.cells(36, 60, 4) == (9, 15) and TR.cells(5, 7, 1) == (5, 7) and TR.cells(5, 7, 8) == (1, 1)


# ---- the sequences the GPU test calls ordinary --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TR.ORDINARY))
def test_ordinary_sequences_exercise_every_reason(name):
    """A condition on the inputs, by the restatement alone: every reason stops at least one point of every sample, a quarter of the
    points or more are alive at the end, and some point advances through every frame."""
    fw, bw, stop, points = TR.ordinary_case(name)
    N, T = fw.shape[:2]
    rows = TR.ref32(fw, bw, points, stop=stop)["rows"]
    for n in range(N):
        for reason in ("NONFINITE", "OUTSIDE", "INCONSISTENT", "MARKED"):
            assert rows[n, COL[reason]] >= 1, (n, reason)
        assert rows[n, COL["ALIVE"]] >= 0.25 * rows[n, COL["POINTS"]] and rows[n, COL["STEPS_MAX"]] == T
        assert rows[n, COL["DISP_MAX"]] > 0.5


# ---- the npz layout and the output names ------------------------------------------------------------------------------------------------
def test_tracks_npz_layout_and_bytes(tmp_path):
    path = evaluate.track_names(str(tmp_path))
    assert path == os.path.join(str(tmp_path), "tracks.npz")
    pos = np.arange(3 * 2 * 4, dtype=np.float64).reshape(3, 2, 4)
    pos[1, :, 2] = np.nan
    ids = np.array([[0, 1, 2, 3], [0, 1, -1, 3], [0, 1, 4, 3]])
    state = np.array([0, 0, 0, 2])
    evaluate.write_tracks_npz(path, pos, ids, state)
    first = open(path, "rb").read()
    with np.load(path) as z:
        assert z.files == ["pos", "track_id", "state"]
        assert z["pos"].dtype == np.float32 and z["track_id"].dtype == np.int32 and z["state"].dtype == np.uint8
        assert np.array_equal(z["pos"], pos.astype(np.float32), equal_nan=True) and np.array_equal(z["track_id"], ids) and np.array_equal(z["state"], state)
    other = str(tmp_path / "again.npz")
    evaluate.write_tracks_npz(other, pos, ids, state)
    assert open(other, "rb").read() == first                                        # no time of day in the file
    with pytest.raises(ValueError, match="write_tracks_npz"):
        evaluate.write_tracks_npz(path, pos, ids[:2], state)


def test_runner_names_its_outputs_and_takes_its_flags_from_the_other_runners():
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("track_flownet", os.path.join(here, "..", "scripts", "track_flownet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["frames.txt", "out", "--weights", "w.h5", "--window", "3", "--general-conv", "own"])
    assert (a.frames, a.out_dir, a.window, a.cell, a.no_reseed, a.long_range, a.general_conv) == ("frames.txt", "out", 3, 4, False, None, "own")
    b = mod.parse_args(["frames.txt", "out", "--weights", "w.h5", "--long-range", "lr.flo", "--color", "lr.png"])
    assert (b.cell, b.no_reseed, b.long_range, b.color) == (1, True, "lr.flo", "lr.png")
    with pytest.raises(SystemExit):
        mod.parse_args(["frames.txt", "out", "--weights", "w.h5", "--color", "lr.png"])      # --color draws the long-range flow
    # the identities of the trajectories: a new id at every born slot
    ids, nxt = mod.next_ids(np.array([0, 1, 2, 3], np.int32), 4, state=np.array([0, 2, 0, 4]), born=np.array([0, 0, 0, 1]))
    assert ids.tolist() == [0, -1, 2, 4] and nxt == 5
