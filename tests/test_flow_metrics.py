"""The flow-metrics kernel (csrc/flow_metrics.hip) through the C ABI of include/flownet2_hip_flow_metrics.h: counts equal to, and sums
within flow_metrics_ref.bound of, the float64 restatement; the classification edges on exactly representable values; the EPE map; the
same bits from run to run, for a sample alone and in its batch, with and without the map and at any alignment; the totals row; refusals
that write nothing; functional.flow_metrics; and scripts/eval_flownet.py end to end against run_flownet.py's .flo."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flow_metrics_ref as FR
from flownet2_amd import evaluate, flo, ops
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import COL, K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIRS = os.path.join(ROOT, "tests", "golden", "chairs")
SENTINEL = 0x5A

# name -> (shape, float offset of every blob inside its allocation, masks).  A thread owns four neighbouring pixels where H * W % 4 == 0
# (16-byte loads where every pointer allows, else 4-byte loads) and one pixel otherwise; a sample is cut into ceil(H W / 1024) <= 128
# workgroups of 256 threads; more than 65536 (sample, workgroup) items are taken in a loop.
CASES = {
    "1x2x1x1": ((1, 2, 1, 1), 0, True),
    "2x2x5x7": ((2, 2, 5, 7), 0, True),                   # a plane that is no multiple of 4
    "2x2x5x7_no_masks": ((2, 2, 5, 7), 0, False),
    "3x2x8x16": ((3, 2, 8, 16), 0, True),                 # the aligned 16-byte path
    "3x2x8x16_offset1": ((3, 2, 8, 16), 1, True),         # every pointer advanced by one float: four 4-byte loads, the same bits
    "2x2x67x131": ((2, 2, 67, 131), 0, True),             # one pixel per thread, 9 workgroups per sample, a ragged last one
    "2x2x36x60": ((2, 2, 36, 60), 0, True),               # four pixels per thread, 3 workgroups per sample, a ragged last one
    "1x2x365x364": ((1, 2, 365, 364), 0, True),           # 130 > 128 workgroups' worth: some threads take a second step
    "65537x2x1x1": ((65537, 2, 1, 1), 0, True),           # more work items than the grid: the workgroup-stride loop, the finalise loops
}
SAME_INPUTS = {"3x2x8x16_offset1": "3x2x8x16"}


def _dev(a, offset=0):
    """A device copy of float32 array `a` that starts `offset` floats into its (256-byte aligned) allocation."""
    if a is None:
        return None
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


@functools.lru_cache(maxsize=None)
def _inputs(name):
    name = SAME_INPUTS.get(name, name)
    shape, _, masks = CASES[name]
    case = FR.make_case(shape, seed=sorted(CASES).index(name), masks=masks)
    for a in case:
        if a is not None:
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _reference(name):
    """ref64 and its bound, computed once per case and shared."""
    return FR.bound(*_inputs(SAME_INPUTS.get(name, name)))


def _run_arrays(arrays, shape, offset=0, epe_map=False, outlier=FR.OUTLIER, bands=FR.BANDS):
    """One call in fresh allocations -> (results [N + 1, K] float64, epe map or None) on the host."""
    N, _, H, W = shape
    pred, gt, valid, occ = (_dev(a, offset) for a in arrays)
    ws_bytes, _ = FR.sizes(N, H, W)
    ws = torch.full((ws_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    results = torch.full(((N + 1) * K,), float("nan"), dtype=torch.float64, device="cuda")
    emap = _dev(np.full((N, 1, H, W), 7.0, np.float32), offset) if epe_map else None
    assert FR.call(pred, gt, valid, occ, shape, results, emap, ws, ws_bytes, outlier, bands) == FR.OK
    torch.cuda.synchronize()
    return results.cpu().numpy().reshape(N + 1, K), (emap.cpu().numpy() if epe_map else None)


@functools.lru_cache(maxsize=None)
def _run(name, epe_map=False):
    shape, offset, _ = CASES[name]
    return _run_arrays(_inputs(name), shape, offset, epe_map)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_against_ref64(name):
    B = _reference(name)
    ref, bnd = B["ref"], B["bound"]
    got, _ = _run(name)
    q = B["pixels"]
    N = ref.shape[0] - 1
    if N >= 2:
        assert ref[N - 1, COL["VALID"]] == 0 and not got[N - 1].any()                # the sample without a valid pixel: a row of zeros
    if q["counted"][0].size >= 30:
        assert ref[0, COL["NONFINITE"]] == 4 and (~q["counted"]).sum() >= 5
    assert np.array_equal(got[:, FR.COUNT_COLUMNS], ref[:, FR.COUNT_COLUMNS]), "counts differ from the reference"
    err = np.abs(got - ref)[:, FR.SUM_COLUMNS]
    worst = err / np.maximum(bnd[:, FR.SUM_COLUMNS], 1e-300)
    print(f"{name}: max |err| {err.max():.3e}, worst err / bound {worst.max():.3f} (column {FR.SUM_COLUMNS[int(worst.max(0).argmax())]})")
    assert np.isfinite(got).all() and np.all(err <= bnd[:, FR.SUM_COLUMNS]), f"error up to {worst.max():.3f} x its bound"
    if CASES[name][2] and N * q["counted"][0].size >= 100:
        assert all(ref[N, COL[c]] > 0 for c in ("OUTLIERS", "BAND_COUNT0", "BAND_COUNT1", "BAND_COUNT2", "OCC_COUNT"))


@pytest.mark.parametrize("name", list(CASES))
def test_bits_repeat_and_do_not_depend_on_batch_map_or_alignment(name):
    shape, offset, _ = CASES[name]
    got, _ = _run(name)
    again, _ = _run_arrays(_inputs(name), shape, offset)                             # other allocations
    assert np.array_equal(_bits(got), _bits(again))
    with_map, emap = _run(name, True)
    assert np.array_equal(_bits(got), _bits(with_map)), "asking for the epe map changed the results"
    if name in SAME_INPUTS:
        aligned, aligned_map = _run(SAME_INPUTS[name], True)
        assert np.array_equal(_bits(got), _bits(aligned)) and np.array_equal(_bits(emap), _bits(aligned_map))
    # the totals row: the fp64 sum of the sample rows in sample order, the max for EPE_MAX
    N = shape[0]
    total = np.zeros(K)
    for n in range(N):
        total = total + got[n]
    total[COL["EPE_MAX"]] = got[:N, COL["EPE_MAX"]].max()
    assert np.array_equal(_bits(got[N]), _bits(total))
    # each sample alone (at most four of them): the bits of its row in the batch
    for n in sorted({0, 1, N // 2, N - 1} & set(range(N))) if N > 1 else []:
        alone, _ = _run_arrays([a[n:n + 1] if a is not None else None for a in _inputs(name)], (1,) + shape[1:], offset)
        assert np.array_equal(_bits(alone[0]), _bits(got[n])) and np.array_equal(_bits(alone[1]), _bits(alone[0])), n


@pytest.mark.parametrize("name", list(CASES))
def test_epe_map(name):
    pred, gt, valid, occ = _inputs(name)
    _, emap = _run(name, True)
    want = FR.epe32(pred, gt, valid, occ)
    counted = _reference(name)["pixels"]["counted"][:, np.newaxis]
    assert emap.dtype == np.float32 and emap.shape == want.shape
    assert np.array_equal(np.isnan(emap), ~counted) and np.array_equal(np.isnan(want), ~counted)
    ulp = np.spacing(want[counted])                                                  # one ulp of sqrtf at the float32 restatement
    assert np.all(np.abs(emap[counted].astype(np.float64) - want[counted]) <= ulp)
    assert emap[counted].max() == _run(name)[0][-1, COL["EPE_MAX"]]                  # the map and the row hold the same float


def test_on_the_edges_with_exact_values():
    """Every operation is exact on these values, so float32 and float64 agree on the edge itself: epe == outlier_abs is no outlier (>),
    |gt| == band0 lies in band 1 and |gt| == band1 in band 2 (<)."""
    gt = np.array([[0, 0], [6, 8], [24, 32], [6, 8], [0.75, 1.0], [60, 80], [0, 0], [3, 4]], np.float32)             # |gt| = 0 10 40 10 1.25 100 0 5
    d = np.array([[3, 0], [0, 0], [0, 0], [0, -3], [1.5, 2.0], [3, 4], [0, 3.5], [0, 0]], np.float32)                # epe  = 3  0  0  3  2.5   5 3.5 0
    pred = gt + d
    shape = (1, 2, 2, 4)
    arrays = [np.ascontiguousarray(a.T.reshape(shape)) for a in (pred, gt)] + [None, None]
    got, emap = _run_arrays(arrays, shape, epe_map=True)
    ref = FR.ref64(*arrays)
    assert emap.ravel().tolist() == [3.0, 0.0, 0.0, 3.0, 2.5, 5.0, 3.5, 0.0]
    row = got[0]
    assert row[COL["VALID"]] == 8 and row[COL["EPE_SUM"]] == 17.0 and row[COL["EPE_SQ_SUM"]] == 9 + 9 + 6.25 + 25 + 12.25 and row[COL["EPE_MAX"]] == 5.0
    # outliers: 3 > 3 fails twice; 2.5 fails; 5 > 3 but 5 > 0.05 * 100 fails (the relative edge); 3.5 at |gt| = 0 is the one outlier
    assert row[COL["OUTLIERS"]] == 1
    assert [row[COL["BAND_COUNT%d" % b]] for b in range(3)] == [4, 2, 2]
    assert [row[COL["BAND_EPE_SUM%d" % b]] for b in range(3)] == [3 + 2.5 + 3.5, 3.0, 5.0]
    assert np.array_equal(got[:, FR.COUNT_COLUMNS], ref[:, FR.COUNT_COLUMNS])
    for c in ("EPE_SUM", "EPE_SQ_SUM", "EPE_MAX", "BAND_EPE_SUM0", "BAND_EPE_SUM1", "BAND_EPE_SUM2"):
        assert got[0, COL[c]] == ref[0, COL[c]], c
    # other thresholds are the call's: with outlier_abs 2.9 the three pixels of epe 3 and 3.5 at small |gt| count, 5 at |gt| = 100 still fails
    moved, _ = _run_arrays(arrays, shape, outlier=(2.9, 0.05), bands=(5.0, 10.0))
    assert moved[0, COL["OUTLIERS"]] == 3 and [moved[0, COL["BAND_COUNT%d" % b]] for b in range(3)] == [3, 1, 4]


def test_refused_calls_write_nothing():
    ws_bytes, _ = FR.sizes(2, 5, 7)
    mk = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    bufs = {"pred": mk(560), "gt": mk(560), "valid": mk(280), "occ": mk(280), "results": mk(3 * K * 8), "epe_map": mk(280), "ws": mk(ws_bytes)}
    cases = FR.refusals(bufs["pred"], bufs["gt"], bufs["valid"], bufs["occ"], bufs["results"], bufs["epe_map"], bufs["ws"], ws_bytes)
    assert len(cases) == 23
    for label, want, thunk in cases:
        assert thunk() == want, label
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == SENTINEL).all()), k


def test_functional_and_ops():
    name = "2x2x36x60"
    pred, gt, valid, occ = (torch.from_numpy(np.array(a)).cuda() for a in _inputs(name))
    got, _ = _run(name)
    results, emap = ops.flow_metrics(pred, gt, valid, occ)
    assert emap is None and results.dtype == torch.float64 and np.array_equal(_bits(results.cpu().numpy()), _bits(got))
    assert tuple(results.shape) == (3, K)
    m = Fn.flow_metrics(pred, gt, valid, occ, epe_map=True)
    assert isinstance(m, evaluate.FlowMetrics) and len(m) == 2 and np.array_equal(_bits(m.rows), _bits(got[:2]))
    assert m.epe_map.shape == (2, 1, 36, 60) and np.array_equal(_bits(m.epe_map.cpu().numpy()), _bits(_run(name, True)[1]))
    s = m.summary()
    assert s["samples"] == 2 and s["samples_without_ground_truth"] == 1 and s["nonfinite"] == 4 and s["pixels"] == got[2, COL["VALID"]]
    assert s["epe"] == s["epe_pixel"] == got[0, COL["EPE_SUM"]] / got[0, COL["VALID"]]          # one sample has every counted pixel
    other = Fn.flow_metrics(pred, gt, valid, occ, outlier=(1.0, 0.0), bands=(1.0, 2.0))
    assert other.summary()["fl_all"] > s["fl_all"] and other.column("BAND_COUNT2").sum() > m.column("BAND_COUNT2").sum()
    # a metric, not a loss
    with pytest.raises(RuntimeError, match="not differentiable"):
        Fn.flow_metrics(pred.clone().requires_grad_(True), gt)
    with torch.no_grad():
        assert np.array_equal(Fn.flow_metrics(pred.clone().requires_grad_(True), gt, valid, occ).rows, m.rows)
    with pytest.raises(ValueError, match="CUDA"):
        Fn.flow_metrics(pred.cpu(), gt.cpu())                                        # no CPU path, no fall-back
    with pytest.raises(ValueError, match=r"must both be \[N,2,H,W\]"):
        Fn.flow_metrics(pred[:, :1], gt[:, :1])
    with pytest.raises(ValueError, match="valid"):
        Fn.flow_metrics(pred, gt, valid[:1])


def test_eval_script_end_to_end(tmp_path):
    """scripts/eval_flownet.py --net S with seeded weights on the FlyingChairs pair, named three times: the summary's epe is the float64 EPE
    of the .flo that run_flownet.py writes for the pair against the ground-truth .flo, within the kernel's bound for that prediction; the JSON
    has the same bytes for --batch 1, 2 and 3."""
    i0, i1 = (os.path.join(CHAIRS, "0000000-%s.png" % k) for k in ("img0", "img1"))
    gt_path = str(tmp_path / "gt.flo")
    flo.write_flo(gt_path, np.load(os.path.join(CHAIRS, "0000000-gt.npz"))["flow"])
    lst = tmp_path / "list.txt"
    lst.write_text(f"{i0} {i1} {gt_path}\n" * 3)
    run = lambda script, *args: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), *args], capture_output=True, text=True, timeout=600)
    docs = {}
    for batch in (1, 2, 3):
        out = str(tmp_path / f"b{batch}.json")
        extra = ["--epe-maps", str(tmp_path / "maps")] if batch == 2 else []
        r = run("eval_flownet.py", "--net", "S", "--batch", str(batch), "--json", out, *extra, str(lst))
        assert r.returncode == 0, r.stderr[-2000:]
        docs[batch] = open(out, "rb").read()
        assert json.loads(r.stdout.strip().splitlines()[-1]) == json.loads(docs[batch])["summary"]
    assert docs[1] == docs[2] == docs[3]
    single = str(tmp_path / "single.flo")
    r = run("run_flownet.py", "--net", "S", i0, i1, single)
    assert r.returncode == 0, r.stderr[-2000:]
    pred = flo.read_flo(single).transpose(2, 0, 1)[np.newaxis]
    gt = flo.read_flo(gt_path).transpose(2, 0, 1)[np.newaxis]
    B = FR.bound(pred, gt)
    doc = json.loads(docs[1])
    rows = np.array(doc["rows"])
    assert rows.shape == (3, K) and np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2])
    assert np.array_equal(rows[0, FR.COUNT_COLUMNS], B["ref"][0, FR.COUNT_COLUMNS]) and rows[0, COL["VALID"]] == 384 * 512
    assert np.all(np.abs(rows[0] - B["ref"][0]) <= B["bound"][0])
    want = float(np.sqrt(((pred.astype(np.float64) - gt) ** 2).sum(1)).mean())       # the EPE a user computes from the two .flo files
    s = doc["summary"]
    print(f"epe {s['epe']!r} against {want!r}, bound {B['bound'][0, COL['EPE_SUM']] / (384 * 512):.3e}")
    assert abs(s["epe"] - want) <= B["bound"][0, COL["EPE_SUM"]] / (384 * 512) and s["epe"] == s["epe_pixel"]
    assert s["samples"] == 3 and s["pixels"] == 3 * 384 * 512 and s["nonfinite"] == 0 and s["samples_without_ground_truth"] == 0
    emap = np.load(str(tmp_path / "maps" / "000001.npy"))
    assert emap.shape == (384, 512) and sorted(os.listdir(tmp_path / "maps")) == ["000000.npy", "000001.npy", "000002.npy"]
    assert np.all(np.abs(emap - FR.epe32(pred, gt)[0, 0]) <= np.spacing(FR.epe32(pred, gt)[0, 0]))


def _small_list(tmp_path):
    """Two pairs of 96 x 136 images with random ground truth (a NaN in it) -> the list file.  96 x 136 is the size at which the runners'
    own guarantees are pinned (tests/test_prototxt.py: the prototxt net gives the built-in graph's bytes; tests/test_gpu_parity.py: a pair's
    bytes do not depend on its batch); what the evaluator adds on top -- rows that do not depend on the batch -- is tested at every size
    above."""
    from PIL import Image
    rng = np.random.default_rng(4)
    lines = []
    for k in range(2):
        a = rng.integers(0, 256, (96, 136, 3), dtype=np.uint8)
        names = [str(tmp_path / f"{k}_{n}") for n in ("a.ppm", "b.ppm", "gt.npz")]
        Image.fromarray(a).save(names[0]); Image.fromarray(np.roll(a, (1, 2), (0, 1))).save(names[1])
        gt = (rng.standard_normal((2, 96, 136)) * 4).astype(np.float32)
        gt[:, 3, 5] = np.nan
        np.savez(names[2], flow=gt)
        lines.append(" ".join(names))
    lst = tmp_path / "small.txt"
    lst.write_text("\n".join(lines) + "\n")
    return str(lst)


def _eval(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_flownet.py"), *args], capture_output=True, text=True, timeout=600)


def test_eval_script_prototxt_form(tmp_path):
    """`model deploy.prototxt.template list`, run_flownet.py's first argument form (the net is built from the template for every group), gives
    the bytes of the built-in graph's JSON for the same seeded weights."""
    from flownet2_amd import templates
    lst = _small_list(tmp_path)
    outs = [str(tmp_path / n) for n in ("proto.json", "builtin.json")]
    r = _eval("seed:S", templates.template_path("S"), lst, "--batch", "2", "--json", outs[0])
    assert r.returncode == 0, r.stderr[-2000:]
    r = _eval("--net", "S", lst, "--batch", "2", "--json", outs[1])
    assert r.returncode == 0, r.stderr[-2000:]
    proto, builtin = (open(o, "rb").read() for o in outs)
    assert proto == builtin
    s = json.loads(proto)["summary"]
    assert s["samples"] == 2 and s["pixels"] == 2 * (96 * 136 - 1) and s["nonfinite"] == 0 and s["epe"] > 0 and s["epe_unmatched"] is None


def test_eval_script_exit_status_on_nonfinite_predictions(tmp_path):
    """Weights with a NaN give NaN flow: every valid pixel is counted in `nonfinite`, none in a sum, and the script exits 1 unless
    --allow-nonfinite is given."""
    from flownet2_amd import nets
    lst = _small_list(tmp_path)
    P = nets.init_params("S", 0)
    name = next(iter(P))
    w = P[name].numpy().copy()
    w.flat[0] = np.nan
    weights = str(tmp_path / "nan.npz")
    np.savez(weights, **{name: w})
    r = _eval("--net", "S", "--weights", weights, lst)
    assert r.returncode == 1 and "NaN or Inf prediction" in r.stderr, r.stderr[-2000:]
    s = json.loads(r.stdout.strip().splitlines()[-1])
    assert s["nonfinite"] == 2 * (96 * 136 - 1) and s["pixels"] == 0 and s["epe"] is None and s["samples_without_ground_truth"] == 0
    r = _eval("--net", "S", "--weights", weights, "--allow-nonfinite", lst)
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1]) == s, r.stderr[-2000:]
