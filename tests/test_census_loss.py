"""The census-loss kernels (csrc/census_loss.hip) through the C ABI of include/flownet2_hip_census_loss.h: with gamma = 0.5 the planes G, Wg
and pd, every count and fw_diff / bw_diff equal to the float32 restatement (census_loss_ref.ref32) bit for bit, the fp64 sums within
n 2^-53 sum|v| of the exact sums of its per-pixel values and the loss equal to its formula on the device's own totals; the same bits alone
and in a batch, with and without occ, loss and saved, at any alignment and from run to run; with gamma = 0.45 the counts equal and the sums,
the loss and the gradients within the running bound of the float64 restatement; and what one NaN removes."""
import functools

import numpy as np
import pytest
import torch

import census_loss_ref as R
from flownet2_amd.evaluate import CENSUS_LOSS_COL as COL, CENSUS_LOSS_K as K

pytestmark = pytest.mark.gpu

F = np.float32
# the tile of the stencil pass is 32 x 8 pixels with a halo of `radius`; a (direction, sample) is cut into min(tiles, 128) workgroups
SHAPES = {
    "1x1x1x1": (1, 1, 1, 1),                              # no pairs
    "1x1x3x5": (1, 1, 3, 5),                              # smaller than the patch
    "3x1x7x67": (3, 1, 7, 67),                            # W % 4 != 0, a ragged tile
    "2x3x16x64": (2, 3, 16, 64),
    "1x3x37x70": (1, 3, 37, 70),                          # several tiles along both axes, both ragged
}
KINDS = ("small", "large", "nonfinite")
RADII = (1, 2, 3)
KEYS = ("img0", "img1", "fw", "bw", "occ_fw", "occ_bw")
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """The six input arrays of a case (read-only), seeded by the shape and the kind."""
    seed = 1 + sorted(SHAPES).index(name) * 10 + KINDS.index(kind)
    arrays = R.make_inputs(SHAPES[name], kind, seed)
    for t in arrays:
        t.setflags(write=False)
    return dict(zip(KEYS, arrays))


def _dev(a, offset=0):
    """A device copy of float32 array `a` that starts `offset` floats into its (256-byte aligned) allocation."""
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def run(case, p, offset=0, two=True, occ=True, loss=True, saved=True, grad=True, total_diff=None):
    """One forward (and backward) call in fresh allocations -> dict(rows [2, N + 1, K], loss float32 or None, planes [2, N, 3, H, W] or
    None, diff [fw_diff, bw_diff])."""
    shape = case["img0"].shape
    N, Cc, H, W = shape
    use = {k: case[k] for k in KEYS}
    if not two:
        use["bw"] = use["occ_bw"] = None
    if not occ:
        use["occ_fw"] = use["occ_bw"] = None
    dev = [None if use[k] is None else _dev(np.asarray(use[k]), offset) for k in KEYS]
    ws_bytes, saved_floats, k = R.sizes(N, H, W, p["radius"])
    assert k == K and saved_floats == 2 * N * 3 * H * W
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    results = torch.full((2 * (N + 1) * K,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda") if loss else None
    planes = _dev(np.full((2, N, 3, H, W), SENTINEL, F), offset) if saved else None
    assert R.forward(*dev, shape, p, results, out, planes, ws, ws_bytes) == R.OK
    diffs = []
    if grad and saved:
        diffs = [_dev(np.full((N, 2, H, W), SENTINEL, F), offset) for _ in range(2 if two else 1)]
        g = None if total_diff is None else torch.tensor([total_diff], dtype=torch.float32, device="cuda")
        assert R.backward(*dev[:4], shape, p, results, planes, g, diffs[0], diffs[1] if two else None) == R.OK
    torch.cuda.synchronize()
    return dict(rows=results.cpu().numpy().reshape(2, N + 1, K), loss=None if out is None else out.cpu().numpy()[0],
                planes=None if planes is None else planes.cpu().numpy(), diff=[d.cpu().numpy() for d in diffs])


def _ref(case, p, two=True, occ=True, total_diff=1.0, which=R.ref32, **kw):
    return which(case["img0"], case["img1"], case["fw"], case["bw"] if two else None, case["occ_fw"] if occ else None,
                 case["occ_bw"] if occ and two else None, p, total_diff, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want):
    """The same bits; a NaN (an undefined grey value) equals any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(got)
    return bool(np.array_equal(nan, np.isnan(want)) and np.array_equal(_bits(np.where(nan, 0, got).astype(got.dtype)),
                                                                       _bits(np.where(nan, 0, want).astype(got.dtype))))


def _loss_of(rows, p, dirs):
    L = 0.0
    for d in range(dirs):
        t = rows[d, -1]
        L = L + (float(F(p["data_weight"])) * t[COL["DATA_SUM"]]) / max(t[COL["COUNTED"]], 1.0)
    return F(L)


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_planes_counts_and_gradients_equal_the_float32_restatement_bit_for_bit(name, kind, radius):
    """Both directions with the occlusion planes, then the forward direction alone without them."""
    p = R.params(radius=radius, data_weight=0.75, **R.EXACT)
    case = _case(name, kind)
    N, Cc, H, W = SHAPES[name]
    for two, occ in ((True, True), (False, False)):
        got = run(case, p, two=two, occ=occ, total_diff=0.75)
        want = _ref(case, p, two=two, occ=occ, total_diff=0.75, rows=got["rows"])
        dirs = 2 if two else 1
        if kind != "nonfinite":
            assert R.not_counted_share(want["rows"][:dirs]) <= 1 / 3               # the cap on what an unpoisoned case may lose
        assert np.isfinite(got["rows"]).all()
        assert np.array_equal(got["rows"][:, :, R.COUNT_COLUMNS], want["rows"][:, :, R.COUNT_COLUMNS]), "counts differ from the restatement"
        rows = got["rows"][:dirs, :, R.COUNT_COLUMNS[:5]]
        assert np.array_equal(rows[..., 0], rows[..., 1:].sum(-1))                  # PIXELS = COUNTED + OCCLUDED + OUTSIDE + NONFINITE
        for d in range(dirs):
            for j, plane in enumerate(("G", "Wg", "pd")):
                g, w = got["planes"][d][:, j], want["planes"][d][:, j]
                assert _same(g, w), f"direction {d}, plane {plane}: {(~np.isclose(g, w, rtol=0, atol=0, equal_nan=True)).sum()} of {g.size} differ"
            g, w = got["diff"][d], want["diff"][d]
            assert np.isfinite(g).all() and _same(g, w), f"direction {d}: {(_bits(g) != _bits(w)).sum()} of {g.size} gradient elements differ"
        # the fp64 sums: the restatement's per-pixel float32 values, added in any order
        n = np.array([H * W] * N + [N * H * W], np.float64)[None, :, None]
        err = np.abs(got["rows"] - want["rows"])[:, :, R.SUM_COLUMNS]
        assert np.all(err <= (n * 2.0 ** -53 * want["sum_abs"])[:, :, R.SUM_COLUMNS]), f"sums: {err.max():.3e}"
        assert _same(got["loss"], _loss_of(got["rows"], p, dirs)), f"loss {got['loss']!r}"
        if not two:
            assert not got["rows"][1].any() and (got["planes"][1] == SENTINEL).all()      # a direction that is not run: zeros, not written
    if kind == "large" and min(H, W) >= 4:
        assert got["rows"][0, -1, COL["OUTSIDE"]] > 0
    if kind == "nonfinite":
        assert got["rows"][0, -1, COL["NONFINITE"]] > 0


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", list(SHAPES))
def test_absent_occ_loss_and_saved_alignment_and_a_second_run_change_no_bit(name, radius):
    case = dict(_case(name, "small"))
    p = R.params(radius=radius)
    full = run(case, p)
    everything = lambda a, b: _same(a["rows"], b["rows"]) and _same(a["planes"], b["planes"]) and all(_same(x, y) for x, y in zip(a["diff"], b["diff"]))
    assert everything(full, run(case, p)) and _same(full["loss"], run(case, p)["loss"])                  # from run to run
    assert everything(full, run(case, p, loss=False))
    rows_only = run(case, p, saved=False)
    assert _same(full["rows"], rows_only["rows"]) and _same(full["loss"], rows_only["loss"])
    moved = run(case, p, offset=1)                                                  # every float blob moved by one float
    assert everything(full, moved) and _same(full["loss"], moved["loss"])
    zeros = np.zeros_like(case["occ_fw"])
    with_zeros, absent = run(dict(case, occ_fw=zeros, occ_bw=zeros), p), run(case, p, occ=False)
    assert everything(with_zeros, absent) and _same(with_zeros["loss"], absent["loss"])


@pytest.mark.parametrize("name", ["3x1x7x67", "2x3x16x64", "1x3x37x70"])
def test_a_sample_has_the_same_bits_alone_and_in_any_batch(name):
    base, other = _case(name, "small"), _case(name, "nonfinite")
    one = {k: v[:1] for k, v in base.items()}
    first = {k: np.concatenate([base[k][:1], other[k][:1], other[k][:1]]) for k in KEYS}
    third = {k: np.concatenate([other[k][:1], other[k][:1], base[k][:1]]) for k in KEYS}
    p = R.params()
    alone, in_first, in_third = (run(c, p) for c in (one, first, third))
    for d in range(2):
        assert _same(alone["rows"][d, 0], in_first["rows"][d, 0]) and _same(alone["rows"][d, 0], in_third["rows"][d, 2])
        assert _same(alone["rows"][d, 0], alone["rows"][d, 1])                      # the totals row of a batch of one
        assert _same(alone["planes"][d, 0], in_first["planes"][d, 0]) and _same(alone["planes"][d, 0], in_third["planes"][d, 2])


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_powf_form_within_the_running_bound_of_the_float64_restatement(name, kind, radius):
    """gamma = 0.45: powf is not correctly rounded, so the comparison is with the float64 restatement and its bound, powf's allowance
    that of unsup_loss_ref._pow."""
    p = R.params(radius=radius)
    case = _case(name, kind)
    got = run(case, p)
    want = _ref(case, p, which=R.ref64)
    assert np.array_equal(got["rows"][:, :, R.COUNT_COLUMNS], want["rows"][:, :, R.COUNT_COLUMNS]), "counts differ from the restatement"
    err = np.abs(got["rows"] - want["rows"])[:, :, R.SUM_COLUMNS]
    bnd = want["rows_bound"][:, :, R.SUM_COLUMNS]
    lerr = abs(float(got["loss"]) - want["loss"])
    worst = max(float((err / np.maximum(bnd, 1e-300)).max()), lerr / want["loss_bound"])
    assert np.isfinite(bnd).all() and np.all(err <= bnd) and lerr <= want["loss_bound"]
    for d in range(2):
        e, b = np.abs(got["diff"][d] - want["diff"][d]), want["diff_bound"][d]
        worst = max(worst, float((e / np.maximum(b, 1e-300)).max()))
        assert np.isfinite(b).all() and np.all(e <= b), f"direction {d}: worst gradient error / bound {(e / np.maximum(b, 1e-300)).max():.3f}"
    print(f"{name} {kind} radius {radius}: worst error / bound {worst:.4f}")


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("where", ["flow", "image", "occ"])
def test_a_nan_removes_its_own_term_and_exactly_the_pairs_that_read_it(where, radius):
    """Against the run without the NaN, the forward direction alone: the counts move by what the header says, and no gradient element more
    than 2 * radius away changes a bit once the normaliser is held fixed -- data_weight is set per run to COUNTED * 2^-12, so kd is 2^-12 in
    both.  (Twice the radius, not once: the gradient at r holds pd(r + q) of every pixel of r's patch, and pd(r + q) = psi'(dist(r + q))
    moves when a pair of r + q's own patch is removed; tests/test_census_loss_host.py shows on the restatement that a pixel radius + 1
    away does change.)"""
    name = "2x3x16x64"
    N, Cc, H, W = SHAPES[name]
    clean = {k: np.array(v) for k, v in _case(name, "small").items()}
    n, y, x = 1, 6, 21
    clean["occ_fw"][n, 0, y - 1:y + 2, x - 1:x + 2] = 0                             # the pixel and its neighbours are not occluded
    clean["fw"][n, :, y - 1:y + 2, x - 1:x + 2] = F(0.25)                           # and their targets are inside
    bad = {k: v.copy() for k, v in clean.items()}
    {"flow": bad["fw"][n, 1], "image": bad["img0"][n, 2], "occ": bad["occ_fw"][n, 0]}[where][y, x] = np.nan
    base = dict(radius=radius, **R.EXACT)
    dec = R.decide(clean["img0"], clean["img1"], clean["fw"], clean["occ_fw"], R.params(**base))
    counted = dec["cls"] == 0
    assert counted[n, y - 1:y + 2, x - 1:x + 2].all()
    own = sum(int(ex[n, y, x]) for ex in dec["exists"].values())
    readers = sum(int(ex[n, y - dy, x - dx] and counted[n, y - dy, x - dx]) for (dx, dy), ex in dec["exists"].items())
    assert own > 0 and readers > 0
    runs = []
    for case in (clean, bad):
        c = run(case, R.params(**base), two=False, grad=False)["rows"][0, -1, COL["COUNTED"]]
        runs.append(run(case, R.params(data_weight=c * 2.0 ** -12, **base), two=False))
    a, b = runs
    ra, rb = a["rows"][0], b["rows"][0]
    column = {"flow": "NONFINITE", "image": "NONFINITE", "occ": "OCCLUDED"}[where]
    assert rb[n, COL[column]] == ra[n, COL[column]] + 1 and rb[n, COL["COUNTED"]] == ra[n, COL["COUNTED"]] - 1
    assert ra[n, COL["PAIRS"]] - rb[n, COL["PAIRS"]] == own + (0 if where == "occ" else readers)
    assert _same(ra[0], rb[0])                                                      # the other sample's row: untouched
    changed = _bits(a["diff"][0]) != _bits(b["diff"][0])
    far = np.ones((H, W), bool)
    far[max(y - 2 * radius, 0):y + 2 * radius + 1, max(x - 2 * radius, 0):x + 2 * radius + 1] = False
    assert not changed[0].any() and not changed[n][:, far].any(), f"{changed[n][:, far].sum()} gradient elements changed away from the NaN"
    assert changed[n][:, ~far].any()
    at_pixel = b["diff"][0][n, :, y, x]
    if where == "occ":
        assert at_pixel.any() and b["planes"][0][n, 2, y, x] == 0 and not np.isnan(b["planes"][0][n, 1, y, x])      # occluded, yet a gradient
    else:
        assert not _bits(np.abs(at_pixel)).any()                                    # no pair holds the pixel: nothing is left there
        assert np.isnan(b["planes"][0][n, 0 if where == "image" else 1, y, x])


def test_zero_flow_on_equal_images_gives_no_distance_and_no_gradient():
    N, Cc, H, W = SHAPES["1x3x37x70"]
    img = np.array(_case("1x3x37x70", "small")["img0"])
    zero = np.zeros((N, 2, H, W), F)
    p = R.params(**R.EXACT)
    got = run(dict(img0=img, img1=img, fw=zero, bw=zero, occ_fw=None, occ_bw=None), p, occ=False)
    eps = F(p["charbonnier"][0])
    for d in range(2):
        row = got["rows"][d, 0]
        assert row[COL["COUNTED"]] == H * W and row[COL["DIST_SUM"]] == 0 and row[COL["DATA_SUM"]] == H * W * float(np.sqrt(eps * eps))
        assert row[COL["PAIRS"]] == sum((H - abs(dy)) * (W - abs(dx)) for dx, dy in R.offsets(3))
        assert not _bits(np.abs(got["diff"][d])).any() and not _bits(got["planes"][d][:, 2]).any()
