"""The unsupervised-loss kernels (csrc/unsup_loss.hip) through the C ABI of include/flownet2_hip_unsup_loss.h: with gamma = 0.5 and no edge
weight the rows, the loss and fw_diff / bw_diff equal to the float32 restatement (unsup_loss_ref.ref32) bit for bit; with gamma = 0.45 and
edge weight 10 the counts equal and the sums and gradients within the operation-count bound of the float64 restatement; the data gradient
against the composition flow_warp -> psi -> masked mean through _FlowWarp's own backward kernel; zero flow, a shift of two, clamped taps,
what a NaN removes, the same bits alone and in a batch and at any alignment; descent on a small problem; and the Python layers."""
import functools

import numpy as np
import pytest
import torch

import unsup_loss_ref as R
from flownet2_amd import functional as Fn
from flownet2_amd import nets
from flownet2_amd.evaluate import UNSUP_LOSS_COL as COL, UNSUP_LOSS_K as K

pytestmark = pytest.mark.gpu

F = np.float32
# name -> (shape [N,C,H,W], float offset of every float blob inside its allocation).  A thread owns four neighbouring pixels of a row where
# W % 4 == 0 (16-byte accesses where every pointer allows, else 4-byte ones) and one pixel otherwise; a (direction, sample) is cut into
# ceil(H W / 1024) <= 128 workgroups of 256 threads.
SHAPES = {
    "2x3x5x7": ((2, 3, 5, 7), 0),                         # one pixel per thread
    "3x1x7x67": ((3, 1, 7, 67), 0),                       # a row longer than a wave, not a multiple of 4
    "2x3x16x64": ((2, 3, 16, 64), 0),                     # four pixels per thread
    "2x3x16x64_offset1": ((2, 3, 16, 64), 1),             # every pointer moved by one float: the 4-byte path
    "2x3x36x60": ((2, 3, 36, 60), 0),                     # three workgroups per sample
    "1x2x1x9": ((1, 2, 1, 9), 0),                         # an axis without smoothness terms
    "1x2x9x1": ((1, 2, 9, 1), 0),
}
KINDS = ("small", "large", "nonfinite")
EXACT = R.params(**R.EXACT)
KEYS = ("img0", "img1", "fw", "bw", "occ_fw", "occ_bw")


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """The six input arrays of a case (read-only), seeded by the shape and the kind."""
    shape = SHAPES[name][0]
    seed = 1 + sorted(SHAPES).index(name.replace("_offset1", "")) * 10 + KINDS.index(kind)
    img0, img1 = R.make_images(shape, seed)
    fw, bw = R.make_flows(shape, seed, "large" if kind == "large" else "small")
    occ_fw, occ_bw = R.make_occ(shape, seed)
    arrays = [img0, img1, fw, bw, occ_fw, occ_bw]
    if kind == "nonfinite":
        R.poison(arrays, seed)
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


def run(case, p, offset=0, two=True, occ=True, loss=True, grad=True, total_diff=None):
    """One forward (and backward) call in fresh allocations -> dict(rows [2, N + 1, K], loss float32 or None, diff [fw_diff, bw_diff])."""
    shape = case["img0"].shape
    N, Cc, H, W = shape
    use = {k: case[k] for k in KEYS}
    if not two:
        use["bw"] = use["occ_bw"] = None
    if not occ:
        use["occ_fw"] = use["occ_bw"] = None
    dev = [None if use[k] is None else _dev(np.asarray(use[k]), offset) for k in KEYS]
    ws_bytes, k = R.sizes(N, H, W)
    assert k == K
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    results = torch.full((2 * (N + 1) * K,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda") if loss else None
    assert R.forward(*dev, shape, p, results, out, ws, ws_bytes) == R.OK
    diffs = []
    if grad:
        diffs = [_dev(np.full((N, 2, H, W), 7.0, F), offset) for _ in range(2 if two else 1)]
        g = None if total_diff is None else torch.tensor([total_diff], dtype=torch.float32, device="cuda")
        assert R.backward(*dev, shape, p, results, g, diffs[0], diffs[1] if two else None) == R.OK
    torch.cuda.synchronize()
    return dict(rows=results.cpu().numpy().reshape(2, N + 1, K), loss=None if out is None else out.cpu().numpy()[0],
                diff=[d.cpu().numpy() for d in diffs])


def _ref(case, p, two=True, occ=True, total_diff=1.0, which=R.ref32):
    return which(case["img0"], case["img1"], case["fw"], case["bw"] if two else None, case["occ_fw"] if occ else None,
                 case["occ_bw"] if occ and two else None, p, total_diff)


@functools.lru_cache(maxsize=None)
def _run_default(name, kind):
    return run(_case(name, kind), R.params(), offset=SHAPES[name][1])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want):
    return bool(np.array_equal(_bits(got), _bits(want)))


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [True, False], ids=["two_directions", "one_direction"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_rows_loss_and_gradients_equal_the_float32_restatement_bit_for_bit(name, kind, order, two):
    p = R.params(smooth_order=order, **R.EXACT)
    case = _case(name, kind)
    got = run(case, p, offset=SHAPES[name][1], two=two, total_diff=0.75)
    want = _ref(case, p, two=two, total_diff=0.75)
    assert np.isfinite(got["rows"]).all()
    assert np.array_equal(got["rows"][:, :, R.COUNT_COLUMNS], want["rows"][:, :, R.COUNT_COLUMNS]), "counts differ from the restatement"
    assert _same(got["rows"], want["rows"]), f"sums differ: {got['rows'][:, -1, R.SUM_COLUMNS]} against {want['rows'][:, -1, R.SUM_COLUMNS]}"
    assert _same(got["loss"], want["loss"]), f"loss {got['loss']!r} against {want['loss']!r}"
    assert len(got["diff"]) == len(want["diff"]) == (2 if two else 1)
    for d, (g, w) in enumerate(zip(got["diff"], want["diff"])):
        assert np.isfinite(g).all() and not (g == 7.0).all()
        assert _same(g, w), f"direction {d}: {(_bits(g) != _bits(w)).sum()} of {g.size} gradient elements differ, worst {np.abs(g - w).max():.3e}"
    if not two:
        assert not got["rows"][1].any()                                             # the rows of the direction not given: zeros
    if kind == "large":
        assert got["rows"][0, -1, COL["OUTSIDE"]] > 0
    if kind == "nonfinite":
        assert got["rows"][0, -1, COL["NONFINITE"]] > 0


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_powf_and_expf_forms_within_the_operation_count_bound(name, kind, order):
    """gamma = 0.45, edge_weight = 10: powf and expf are not correctly rounded, so the comparison is with the float64 restatement and its
    running error bound (unsup_loss_ref's docstring)."""
    p = R.params(smooth_order=order)
    case = _case(name, kind)
    got = run(case, p, offset=SHAPES[name][1]) if order != 2 else _run_default(name, kind)
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
    print(f"{name} {kind} order {order}: worst error / bound {worst:.4f}")


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small", "large"])
@pytest.mark.parametrize("name", ["2x3x5x7", "3x1x7x67", "2x3x16x64", "2x3x36x60"])
def test_data_gradient_against_the_composition_through_flow_warp(name, kind):
    """Independent of the restatement: smooth_weight = 0, and per direction flow_warp(Io, a) -> psi -> sum over the pixels that are inside
    and not occluded / their count -> backward(), which runs _FlowWarp's own backward kernel.  Both gradients carry out the operations
    the bound of ref64 counts (the composition in another association), so they lie within that bound of each other."""
    p = R.params(smooth_weight=0.0)
    case = _case(name, kind)
    got = run(case, p)
    want = _ref(case, p, which=R.ref64)
    (eps, gam), (N, Cc, H, W) = p["charbonnier"], case["img0"].shape
    for d, (Ia, Io, a, occ) in enumerate((("img0", "img1", "fw", "occ_fw"), ("img1", "img0", "bw", "occ_bw"))):
        Ia, Io, occ = (torch.from_numpy(np.array(case[k])).cuda() for k in (Ia, Io, occ))
        a = torch.from_numpy(np.array(case[a])).cuda().requires_grad_(True)
        x2 = torch.arange(W, dtype=torch.float32, device="cuda")[None, None, :] + a.detach()[:, 0]
        y2 = torch.arange(H, dtype=torch.float32, device="cuda")[None, :, None] + a.detach()[:, 1]
        mask = ((x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H) & (occ[:, 0] == 0)).float()
        diff = Ia - Fn.flow_warp(Io, a)
        psi = (diff * diff + eps * eps) ** gam
        loss = (psi.sum(1) * mask).sum() / mask.sum().clamp(min=1)
        loss.backward()
        comp = a.grad.cpu().numpy()
        assert int(mask.sum()) == got["rows"][d, -1, COL["COUNTED"]] > 0
        e, b = np.abs(got["diff"][d] - comp), want["diff_bound"][d]
        print(f"{name} {kind} direction {d}: worst |kernel - composition| / bound {(e / np.maximum(b, 1e-300)).max():.3f}, largest gradient {np.abs(comp).max():.3e}")
        assert np.abs(comp).max() > 0 and np.all(e <= b)


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_flow_on_equal_images_and_a_constant_flow(name, order):
    shape, offset = SHAPES[name]
    N, Cc, H, W = shape
    img = np.array(_case(name, "small")["img0"])
    zero = np.zeros((N, 2, H, W), F)
    case = dict(img0=img, img1=img, fw=zero, bw=zero, occ_fw=None, occ_bw=None)
    p = R.params(smooth_order=order, **R.EXACT)
    got = run(case, p, offset=offset, occ=False)
    eps = F(p["charbonnier"][0])
    psi0 = np.sqrt(eps * eps)                                                       # sqrtf(0 * 0 + eps * eps), correctly rounded
    e = F(0)
    for _ in range(Cc):
        e = e + psi0                                                                # the per-pixel sum over the channels, in float32
    for d in range(2):
        rows = got["rows"][d]
        assert np.array_equal(rows[:, COL["COUNTED"]], rows[:, COL["PIXELS"]]) and rows[-1, COL["PIXELS"]] == N * H * W
        assert np.array_equal(rows[:, COL["DATA_SUM"]], rows[:, COL["COUNTED"]] * float(e))      # a multiple of e below 2^53: every sum exact
        assert np.array_equal(rows[:, COL["SMOOTH_SUM"]], rows[:, COL["SMOOTH_TERMS"]] * float(F(2) * psi0))      # s = 0: psi(0) + psi(0)
        assert not _bits(np.abs(got["diff"][d])).any()                              # zero, whatever its sign
    const = np.broadcast_to(np.array([1.25, -0.5], F)[None, :, None, None], (N, 2, H, W)).copy()
    only_smooth = run(dict(case, fw=const, bw=const), R.params(smooth_order=order, data_weight=0.0, **R.EXACT), offset=offset, occ=False)
    for d in range(2):
        assert not _bits(np.abs(only_smooth["diff"][d])).any()
        terms = (W - order) * H * (W > order) + (H - order) * W * (H > order)
        assert np.array_equal(only_smooth["rows"][d, :N, COL["SMOOTH_TERMS"]], np.full(N, terms))


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_shift_of_two_leaves_exactly_two_columns_outside(name):
    shape, offset = SHAPES[name]
    N, Cc, H, W = shape
    base = _case(name, "small")
    fw, bw = np.zeros((N, 2, H, W), F), np.zeros((N, 2, H, W), F)
    fw[:, 0], bw[:, 0] = 2.0, -2.0
    got = run(dict(base, fw=fw, bw=bw), EXACT, offset=offset, occ=False)
    for d in range(2):
        assert np.array_equal(got["rows"][d, :N, COL["OUTSIDE"]], np.full(N, H * min(2, W)))
        assert np.array_equal(got["rows"][d, :N, COL["COUNTED"]], np.full(N, H * max(W - 2, 0)))
    only_data = run(dict(base, fw=fw, bw=bw), R.params(smooth_weight=0.0, **R.EXACT), offset=offset, occ=False)
    for d, outside in enumerate((np.arange(W) >= W - 2, np.arange(W) < 2)):
        assert not _bits(np.abs(only_data["diff"][d][..., outside])).any()          # no data gradient where the target is outside


def test_targets_on_the_last_row_and_column_clamp_their_taps():
    """x2 = W - 1 and y2 = H - 1 exactly on even rows, x2 = W - 0.25 on odd rows: inside, the right / bottom tap clamped onto the last
    column / row, where the images carry values of their own."""
    name = "3x1x7x67"
    N, Cc, H, W = SHAPES[name][0]
    base = _case(name, "small")
    x, y = np.arange(W, dtype=F)[None, :], np.arange(H, dtype=F)[:, None]
    odd = (np.arange(H) % 2 == 1)[:, None]
    fw = np.zeros((N, 2, H, W), F)
    fw[:, 0] = np.where(odd, F(W - 0.25) - x, F(W - 1) - x)
    fw[:, 1] = np.where(odd, F(0), F(H - 1) - y)
    bw = np.array(base["bw"])
    bw[:, 0, ::3] = F(0.25) - x
    bw[:, 1, ::3] = 0
    img0, img1 = np.array(base["img0"]), np.array(base["img1"])
    img1[:, :, H - 1, :] += F(0.5)
    img1[:, :, :, W - 1] -= F(0.25)
    img0[:, :, 0, :] += F(0.125)
    case = dict(base, img0=img0, img1=img1, fw=fw, bw=bw)
    got = run(case, EXACT, occ=False)
    want = _ref(case, EXACT, occ=False)
    assert not got["rows"][0, :, COL["OUTSIDE"]].any() and got["rows"][0, -1, COL["COUNTED"]] == N * H * W
    assert _same(got["rows"], want["rows"]) and _same(got["loss"], want["loss"])
    assert all(_same(g, w) for g, w in zip(got["diff"], want["diff"]))


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("where", ["flow", "image", "occ"])
def test_a_nan_removes_its_pixel_and_the_terms_that_touch_it(where, order):
    """Against the run without the NaN: the counts move by what the header says, and no other gradient element changes a bit once the
    normalisers are taken out -- data_weight and smooth_weight are set per run so that kd and ks are the same float in both (weights
    proportional to the counts: weight / count = 2^-12 exactly)."""
    name = "2x3x16x64"
    N, Cc, H, W = SHAPES[name][0]
    clean = {k: np.array(v) for k, v in _case(name, "small").items()}
    n, y, x = 1, 5, 21
    bad = {k: v.copy() for k, v in clean.items()}
    {"flow": bad["fw"][n, 1], "image": bad["img0"][n, 2], "occ": bad["occ_fw"][n, 0]}[where][y, x] = np.nan
    clean["occ_fw"][n, 0, y, x] = 0                                                 # the pixel is counted in the clean run
    if where != "occ":
        bad["occ_fw"][n, 0, y, x] = 0
    edge = 10.0 if where == "image" else 0.0                                        # an image value reaches the smoothness terms through the edge weight only
    base = dict(charbonnier=(1e-3, 0.5), smooth_charbonnier=(1e-3, 0.5), edge_weight=edge, smooth_order=order)
    runs = []
    for case in (clean, bad):
        counts = run(case, R.params(**base), two=False, grad=False)["rows"][0, -1]
        p = R.params(data_weight=counts[COL["COUNTED"]] * 2.0 ** -12, smooth_weight=counts[COL["SMOOTH_TERMS"]] * 2.0 ** -12, **base)
        runs.append(run(case, p, two=False))
    a, b = runs
    ra, rb = a["rows"][0], b["rows"][0]
    column = {"flow": "NONFINITE", "image": "NONFINITE", "occ": "OCCLUDED"}[where]
    assert rb[n, COL[column]] == ra[n, COL[column]] + 1 and rb[n, COL["COUNTED"]] == ra[n, COL["COUNTED"]] - 1
    # the terms that read the value, both axes.  flow(p): order 1 the terms owned by p and p - step, order 2 those owned by p - step, p and
    # p + step.  Ia(p), through the edge weight: order 1 the terms owned by p - step (as p+) and p (as q), order 2 those owned by p - step
    # (as p+) and p + step (as p-).  occ: none.
    touching = {"flow": 2 * (order + 1), "image": 4, "occ": 0}[where]
    assert ra[n, COL["SMOOTH_TERMS"]] - rb[n, COL["SMOOTH_TERMS"]] == touching
    assert _same(ra[0], rb[0])                                                      # the other sample's row: untouched
    # a dropped term owned by a pixel one step away reaches `order` pixels from p along its axis
    reach = 0 if where == "occ" else order
    changed = _bits(a["diff"][0]) != _bits(b["diff"][0])
    far = np.ones((H, W), bool)
    far[max(y - reach, 0):y + reach + 1, x] = False
    far[y, max(x - reach, 0):x + reach + 1] = False
    assert not changed[0].any() and not changed[n][:, far].any(), f"{changed[n][:, far].sum()} gradient elements changed away from the NaN"
    assert changed[n][:, y, x].any()
    if where == "flow":
        assert not _bits(np.abs(b["diff"][0][n, :, y, x])).any()                    # nothing is left at the pixel itself


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x1x7x67", "2x3x36x60", "2x3x16x64_offset1"])
def test_a_sample_has_the_same_bits_alone_and_in_any_batch(name):
    offset = SHAPES[name][1]
    base, other = _case(name, "small"), _case(name, "nonfinite")
    one = {k: v[:1] for k, v in base.items()}
    first = {k: np.concatenate([base[k][:1], other[k][:1], other[k][:1]]) for k in KEYS}
    third = {k: np.concatenate([other[k][:1], other[k][:1], base[k][:1]]) for k in KEYS}
    p = R.params()
    alone, in_first, in_third = (run(c, p, offset=offset, grad=False)["rows"] for c in (one, first, third))
    for d in range(2):
        assert _same(alone[d, 0], in_first[d, 0]) and _same(alone[d, 0], in_third[d, 2])
        assert _same(alone[d, 0], alone[d, 1])                                      # the totals row of a batch of one
    assert _same(alone, run(one, p, offset=offset, grad=False)["rows"])             # and from run to run


@pytest.mark.parametrize("name", list(SHAPES))
def test_absent_occ_absent_loss_and_alignment_change_no_bit(name):
    shape, offset = SHAPES[name]
    case = dict(_case(name, "small"))
    full = _run_default(name, "small")
    without_loss = run(case, R.params(), offset=offset, loss=False)
    assert _same(full["rows"], without_loss["rows"]) and all(_same(a, b) for a, b in zip(full["diff"], without_loss["diff"]))
    zeros = np.zeros_like(case["occ_fw"])
    with_zeros = run(dict(case, occ_fw=zeros, occ_bw=zeros), R.params(), offset=offset)
    absent = run(case, R.params(), offset=offset, occ=False)
    assert _same(with_zeros["rows"], absent["rows"]) and _same(with_zeros["loss"], absent["loss"])
    assert all(_same(a, b) for a, b in zip(with_zeros["diff"], absent["diff"]))
    if name.endswith("_offset1"):
        aligned = _run_default(name.replace("_offset1", ""), "small")
        assert _same(full["rows"], aligned["rows"]) and _same(full["loss"], aligned["loss"])
        assert all(_same(a, b) for a, b in zip(full["diff"], aligned["diff"]))


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------
def descent_images():
    """img0 and img1 = img0 translated by 2 px along x: smooth sinusoids [1,1,16,32]; the true forward flow is (+2, 0)."""
    H, W = 16, 32
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f = lambda x, y: 0.5 + 0.25 * np.sin(2 * np.pi * x / 16 + 0.3) * np.cos(2 * np.pi * y / 32) + 0.2 * np.sin(2 * np.pi * (x / 32 + y / 16) + 1.0)
    return f(x, y)[None, None].astype(F), f(x - 2, y)[None, None].astype(F)


DESCENT = dict(step=500.0, steps=40, params=R.params(smooth_weight=0.1))


def test_descent_on_a_translated_image():
    """40 plain gradient steps of size 500 on the forward flow, a leaf tensor starting from zero (defaults but smooth_weight = 0.1; the
    gradient is that of a mean over 512 pixels, hence the step size).  The float64 restatement on the CPU, same inputs and step size
    (run before the kernel was): loss 0.112937 -> 0.059923, EPE against (2, 0) over the counted pixels 2.0 -> 1.271790.  Both conditions
    hold there; the kernel must meet them too."""
    img0, img1 = descent_images()
    i0, i1 = torch.from_numpy(img0).cuda(), torch.from_numpy(img1).cuda()
    fw = torch.zeros((1, 2, 16, 32), device="cuda", requires_grad=True)
    kw = {k: v for k, v in DESCENT["params"].items()}

    def measure():
        rep = Fn.unsupervised_loss_report(i0, i1, fw.detach(), **kw)
        dec = R.decide(img0, img1, fw.detach().cpu().numpy(), None, DESCENT["params"])
        counted = torch.from_numpy(dec["cls"][0] == 0).cuda()
        assert int(counted.sum()) == rep.rows_fw[0, COL["COUNTED"]]
        epe = ((fw.detach()[0, 0] - 2) ** 2 + fw.detach()[0, 1] ** 2).sqrt()[counted].mean()
        return rep.loss, float(epe)

    before = measure()
    for _ in range(DESCENT["steps"]):
        fw.grad = None
        Fn.unsupervised_loss(i0, i1, fw, **kw).backward()
        with torch.no_grad():
            fw -= DESCENT["step"] * fw.grad
    after = measure()
    print(f"descent: loss {before[0]:.6f} -> {after[0]:.6f}, EPE {before[1]:.6f} -> {after[1]:.6f}")
    assert before[1] == 2.0 and after[0] < before[0] and after[1] < before[1]


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------
def test_functional_fills_the_gradients_with_the_kernels_arrays():
    name = "2x3x36x60"
    case = _case(name, "small")
    p = R.params()
    raw = run(case, p, total_diff=1.0)
    t = {k: torch.from_numpy(np.array(v)).cuda() for k, v in case.items()}
    fw, bw = t["fw"].requires_grad_(True), t["bw"].requires_grad_(True)
    loss = Fn.unsupervised_loss(t["img0"], t["img1"], fw, bw, t["occ_fw"], t["occ_bw"])
    assert loss.dim() == 0 and loss.is_cuda and _same(loss.detach().cpu().numpy(), raw["loss"])
    loss.backward()
    assert _same(fw.grad.cpu().numpy(), raw["diff"][0]) and _same(bw.grad.cpu().numpy(), raw["diff"][1])
    fw.grad = bw.grad = None
    (3.0 * Fn.unsupervised_loss(t["img0"], t["img1"], fw, bw, t["occ_fw"], t["occ_bw"])).backward()      # the upstream gradient, on the device
    scaled = run(case, p, total_diff=3.0)
    assert _same(fw.grad.cpu().numpy(), scaled["diff"][0]) and _same(bw.grad.cpu().numpy(), scaled["diff"][1])
    one = Fn.unsupervised_loss(t["img0"], t["img1"], fw.detach().requires_grad_(True), None, t["occ_fw"])
    assert _same(one.detach().cpu().numpy(), run(case, p, two=False, grad=False)["loss"])
    with pytest.raises(RuntimeError, match="gets no gradient"):
        Fn.unsupervised_loss(t["img0"].clone().requires_grad_(True), t["img1"], fw)
    with pytest.raises(ValueError, match="must be"):
        Fn.unsupervised_loss(t["img0"], t["img1"], fw[:, :, :-1])

    rep = Fn.unsupervised_loss_report(t["img0"], t["img1"], fw, bw, t["occ_fw"], t["occ_bw"])
    assert len(rep) == 2 and _same(rep.rows_fw, raw["rows"][0, :-1]) and _same(rep.rows_bw, raw["rows"][1, :-1]) and rep.loss == float(raw["loss"])
    s, tot = rep.summary(), raw["rows"][:, -1]
    for d, key in enumerate(("fw", "bw")):
        assert s[key]["data_mean"] == tot[d, COL["DATA_SUM"]] / tot[d, COL["COUNTED"]]
        assert s[key]["smooth_mean"] == tot[d, COL["SMOOTH_SUM"]] / tot[d, COL["SMOOTH_TERMS"]]
        for share, col in (("counted", "COUNTED"), ("occluded", "OCCLUDED"), ("outside", "OUTSIDE"), ("nonfinite", "NONFINITE")):
            assert s[key][share] == tot[d, COL[col]] / tot[d, COL["PIXELS"]]
        assert s[key]["counted"] + s[key]["occluded"] + s[key]["outside"] + s[key]["nonfinite"] == pytest.approx(1.0)
    assert 0 < s["fw"]["occluded"] < 0.5 and s["samples"] == 2 and s["loss"] == rep.loss


def test_nets_unsupervised_loss_is_the_weighted_sum_of_the_per_scale_calls():
    """A two-scale stub pyramid: per scale the images brought down with downsample, flow_mult = FLOW_SCALE w_s / W, the occlusion planes
    from flow_consistency on the detached, rescaled flows; the result is the weighted sum in list order, bit for bit."""
    N, H, W = 2, 32, 64
    img0, img1 = (torch.from_numpy(t).cuda() for t in R.make_images((N, 3, H, W), 5))
    rng = np.random.default_rng(9)
    sizes = {3: (8, 16), 2: (16, 32)}                                               # scale -> (h, w); LOSS_WEIGHTS lists scale 3 before scale 2
    flows_fw = {s: torch.from_numpy(rng.normal(0, 0.02, (N, 2, h, w)).astype(F)).cuda().requires_grad_(True) for s, (h, w) in sizes.items()}
    flows_bw = {s: torch.from_numpy(rng.normal(0, 0.02, (N, 2, h, w)).astype(F)).cuda().requires_grad_(True) for s, (h, w) in sizes.items()}
    assert [s for s in nets.LOSS_WEIGHTS if s in sizes] == [3, 2] and nets.backend_of(Fn).has_unsupervised_loss
    for occ in ("consistency", None):
        total = nets.unsupervised_loss(flows_fw, flows_bw, img0, img1, Fn, occ=occ, smooth_order=1)
        want = None
        for s in (3, 2):
            (h, w), f, b, lw = sizes[s], flows_fw[s], flows_bw[s], nets.LOSS_WEIGHTS[s]
            mult = nets.FLOW_SCALE * w / W
            i0, i1 = Fn.downsample(img0, h, w), Fn.downsample(img1, h, w)
            of = ob = None
            if occ:
                c = Fn.flow_consistency(f.detach() * mult, b.detach() * mult)
                of, ob = c.occ_fw, c.occ_bw
            term = Fn.unsupervised_loss(i0, i1, f, b, of, ob, smooth_order=1, flow_mult=mult) * lw
            want = term if want is None else want + term
        assert total.dim() == 0 and _same(total.detach().cpu().numpy(), want.detach().cpu().numpy())
    total.backward()
    assert all(f.grad is not None and bool(f.grad.abs().sum() > 0) for f in list(flows_fw.values()) + list(flows_bw.values()))
