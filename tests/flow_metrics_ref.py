"""Flow-metrics references for the tests: the arithmetic of include/flownet2_hip_flow_metrics.h in NumPy float64 (ref64: the rows) and
op by op in float32 (epe32: the EPE map), an error bound per column from the operation count (bound), seeded inputs (make_case) and the
raw C ABI calls.  No file of the reference tree is read, and no tolerance here comes from the kernel's output.

The bound, with U = 2^-24 (every fp32 operation: half an ulp, relative U) and R = 2 U E_POW for sqrtf and atan2f -- the ulp figure the
LpqLoss tests use for powf (lpq_ref.E_POW = 2.64 ulp; ROCm's device-math accuracy table is not installed beside the toolchain).  Starred
values are ref64's.  Inputs are float32 and exact.

  du = pu - gu                 1 rounding, relative to du* itself                                        e_d = U
  s = du du + dv dv            per term (1 + e_d)^2 (1 + U), then the addition of non-negative terms     e_s = (1 + U)^4 - 1
  epe = sqrtf(s)               the square root halves e_s; R on top                                      e_e = (1 - e_s)^-1/2 (1 + R) - 1
  mag = sqrtf(gu gu + gv gv)   exact inputs: two roundings under the root                                e_m = (1 - ((1 + U)^2 - 1))^-1/2 (1 + R) - 1
  EPE_SUM, BAND_EPE_SUM*, OCC_EPE_SUM   sum of e_e epe* over the pixels of the column                    (the classifications are exact, see below)
  EPE_SQ_SUM                   sum of e_s s*
  EPE_MAX                      |max a - max b| <= max |a - b|:                                           max of e_e epe*
  the fp64 additions: n of them, relative 2^-53 each on non-negative terms                               + n 2^-53 (sum*)
  angular error  ae = atan2f(y, x), y = sqrtf((cx cx + cy cy) + cz cz), x = (1 + pu gu) + pv gv:
    cx = pv - gv, cy = gu - pu        relative U each
    cz = pu gv - pv gu                two products and a difference that may cancel:  A = |pu gv| + |pv gu|,
                                      d_cz = U A + U (|cz*| + U A)                      -- the cancellation term 2^-24 (|pu gv| + |pv gu|)
    the vector c = (cx, cy, cz)       |c~ - c*| <= d_c = U hypot(cx*, cy*) + d_cz, so | |c~| - |c*| | <= d_c
    y from c~                         three roundings under the root, the root, R:  e_y = (1 - ((1 + U)^3 - 1))^-1/2 (1 + R) - 1
                                      d_y = d_c (1 + e_y) + |c*| e_y
    x                                 t1 = pu gu, t2 = 1 + t1, t3 = pv gv, x = t2 + t3:
                                      d_x = (U |t1*| + U (|1 + t1*| + U |t1*|) + U |t3*|) (1 + U) + U |x*|
    atan2 of a perturbed point        |grad atan2| = 1 / r, r = hypot(y, x); r* = |(pu, pv, 1)| |(gu, gv, 1)| >= 1, y >= 0 on both sides (no
                                      branch cut between them):  d_t = h / (r* - h), h = hypot(d_y, d_x)
    atan2f itself                     d_ae = d_t + R (ae* + d_t)
  AE_SUM                       sum of d_ae

Counts (VALID, NONFINITE, OUTLIERS, BAND_COUNT*, OCC_COUNT) must be EQUAL: validity and finiteness are decided on the inputs' bits, and
make_case asserts on the CPU that no counted pixel has epe within relative 1e-5 of outlier_abs or of outlier_rel mag, nor mag within
relative 1e-5 of a band edge -- thirty times e_e, e_m or the rounding of outlier_rel mag -- so float32 and float64 classify alike."""
import ctypes as C

import numpy as np

import lpq_ref as LR
from flownet2_amd import _lib
from flownet2_amd.evaluate import COL, K

U = LR.U
R = 2.0 * U * LR.E_POW
TINY = 8 * 2.0 ** -150
MARGIN = 1e-5
OK, INVALID, WORKSPACE = 0, -1, -3
OUTLIER, BANDS = (3.0, 0.05), (10.0, 40.0)


def _f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def per_pixel(pred, gt, valid=None, occ=None, outlier=OUTLIER, bands=BANDS):
    """The header's per-pixel quantities in float64: dict of [N,H,W] arrays."""
    p, g = _f64(pred), _f64(gt)
    oa, orl, b0, b1 = (np.float64(np.float32(x)) for x in (*outlier, *bands))
    pu, pv, gu, gv = p[:, 0], p[:, 1], g[:, 0], g[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = ~np.isnan(gu) & ~np.isnan(gv) & (np.abs(gu) <= np.float64(np.float32(1e9))) & (np.abs(gv) <= np.float64(np.float32(1e9)))
        if valid is not None:
            ok &= np.asarray(valid)[:, 0] != 0
        nonfinite = ok & ~(np.isfinite(pu) & np.isfinite(pv))
        counted = ok & ~nonfinite
        z = lambda a: np.where(counted, a, 0.0)
        pu, pv, gu, gv = z(pu), z(pv), z(gu), z(gv)
        du, dv = pu - gu, pv - gv
        s = du * du + dv * dv
        epe = np.sqrt(s)
        mag = np.sqrt(gu * gu + gv * gv)
        cx, cy, cz = pv - gv, gu - pu, pu * gv - pv * gu
        y, x = np.sqrt(cx * cx + cy * cy + cz * cz), 1.0 + pu * gu + pv * gv
        ae = np.arctan2(y, x)
    band = np.where(mag < b0, 0, np.where(mag < b1, 1, 2))
    occluded = counted & (np.asarray(occ)[:, 0] != 0) if occ is not None else np.zeros_like(counted)
    return dict(pu=pu, pv=pv, gu=gu, gv=gv, counted=counted, nonfinite=nonfinite, s=s, epe=epe, mag=mag, ae=ae, cx=cx, cy=cy, cz=cz, y=y, x=x,
                band=band, outlier=counted & (epe > oa) & (epe > orl * mag), occluded=occluded, thresholds=(oa, orl, b0, b1))


def _rows(q, weight_epe, weight_s, weight_ae, count):
    """[N + 1, K]: per-pixel weights summed per column; `count`: fill the count columns (the reference) or leave them 0 (the bound)."""
    c = q["counted"]
    N = c.shape[0]
    rows = np.zeros((N + 1, K), np.float64)
    tot = lambda a, m: np.where(m, a, 0.0).reshape(N, -1).sum(1)
    rows[:N, COL["EPE_SUM"]] = tot(weight_epe, c)
    rows[:N, COL["EPE_SQ_SUM"]] = tot(weight_s, c)
    rows[:N, COL["EPE_MAX"]] = np.where(c, weight_epe, 0.0).reshape(N, -1).max(1)
    rows[:N, COL["AE_SUM"]] = tot(weight_ae, c)
    for b in range(3):
        rows[:N, COL["BAND_EPE_SUM%d" % b]] = tot(weight_epe, c & (q["band"] == b))
    rows[:N, COL["OCC_EPE_SUM"]] = tot(weight_epe, q["occluded"])
    if count:
        n = lambda m: m.reshape(N, -1).sum(1).astype(np.float64)
        rows[:N, COL["VALID"]], rows[:N, COL["NONFINITE"]], rows[:N, COL["OUTLIERS"]] = n(c), n(q["nonfinite"]), n(q["outlier"])
        for b in range(3):
            rows[:N, COL["BAND_COUNT%d" % b]] = n(c & (q["band"] == b))
        rows[:N, COL["OCC_COUNT"]] = n(q["occluded"])
    rows[N] = rows[:N].sum(0)
    rows[N, COL["EPE_MAX"]] = rows[:N, COL["EPE_MAX"]].max()
    return rows


COUNT_COLUMNS = [COL[n] for n in ("VALID", "NONFINITE", "OUTLIERS", "BAND_COUNT0", "BAND_COUNT1", "BAND_COUNT2", "OCC_COUNT")]
SUM_COLUMNS = [i for i in range(K) if i not in COUNT_COLUMNS]


def ref64(pred, gt, valid=None, occ=None, outlier=OUTLIER, bands=BANDS):
    """The results rows [N + 1, K] in float64 (the sample rows and the totals row)."""
    q = per_pixel(pred, gt, valid, occ, outlier, bands)
    return _rows(q, q["epe"], q["s"], q["ae"], True)


def bound(pred, gt, valid=None, occ=None, outlier=OUTLIER, bands=BANDS):
    """{"ref": ref64's rows, "bound": [N + 1, K] bounds on |computed - ref| (0 in the count columns: they must be equal)} -- the derivation is
    this module's docstring."""
    q = per_pixel(pred, gt, valid, occ, outlier, bands)
    e_s = (1 + U) ** 4 - 1
    e_e = (1 - e_s) ** -0.5 * (1 + R) - 1
    A = np.abs(q["pu"] * q["gv"]) + np.abs(q["pv"] * q["gu"])
    d_cz = U * A + U * (np.abs(q["cz"]) + U * A)
    d_c = U * np.hypot(q["cx"], q["cy"]) + d_cz
    e_y = (1 - ((1 + U) ** 3 - 1)) ** -0.5 * (1 + R) - 1
    d_y = d_c * (1 + e_y) + q["y"] * e_y
    t1, t3 = q["pu"] * q["gu"], q["pv"] * q["gv"]
    d_x = (U * np.abs(t1) + U * (np.abs(1 + t1) + U * np.abs(t1)) + U * np.abs(t3)) * (1 + U) + U * np.abs(q["x"])
    h, r = np.hypot(d_y, d_x), np.hypot(q["y"], q["x"])
    assert np.all(r[q["counted"]] >= 1 - 1e-12) and np.all(h < 0.5)
    d_t = h / (r - h)
    d_ae = d_t + R * (q["ae"] + d_t) + TINY
    ref = _rows(q, q["epe"], q["s"], q["ae"], True)
    B = _rows(q, e_e * q["epe"] + TINY, e_s * q["s"] + TINY, d_ae, False)
    npix = q["counted"][0].size
    B[:, SUM_COLUMNS] += npix * 2.0 ** -53 * np.abs(ref[:, SUM_COLUMNS])
    B[-1, SUM_COLUMNS] += q["counted"].size * 2.0 ** -53 * np.abs(ref[-1, SUM_COLUMNS])
    B[:, COL["EPE_MAX"]] = ref[:, COL["EPE_MAX"]] * e_e + TINY                    # max |a - b| over the pixels is at most e_e times the largest epe*
    return {"ref": ref, "bound": B, "pixels": q}


def epe32(pred, gt, valid=None, occ=None):
    """The EPE map op by op in float32 [N,1,H,W] (np.sqrt is correctly rounded), NaN where the pixel is not counted."""
    q = per_pixel(pred, gt, valid, occ)
    p, g = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        du, dv = p[:, 0] - g[:, 0], p[:, 1] - g[:, 1]
        e = np.sqrt(du * du + dv * dv)
    assert e.dtype == np.float32
    return np.where(q["counted"], e, np.float32(np.nan))[:, np.newaxis].astype(np.float32)


def clear_of_edges(pred, gt, valid=None, occ=None, outlier=OUTLIER, bands=BANDS):
    """The condition under which float32 and float64 classify every counted pixel alike (module docstring)."""
    q = per_pixel(pred, gt, valid, occ, outlier, bands)
    oa, orl, b0, b1 = q["thresholds"]
    c, epe, mag = q["counted"], q["epe"], q["mag"]
    far = lambda a, t: np.abs(a - t) > MARGIN * np.maximum(np.abs(a), np.abs(t))
    return bool(np.all(far(epe, oa)[c]) and np.all((far(epe, orl * mag) | ((epe == 0) & (mag == 0)))[c]) and np.all(far(mag, b0)[c])
                and np.all(far(mag, b1)[c]))


def _draw(shape, seed, masks):
    rng = np.random.default_rng(seed)
    N, _, H, W = shape
    plane = (N, H, W)
    mag = np.exp(rng.uniform(np.log(0.05), np.log(80.0), plane))                    # all three bands
    ang = rng.uniform(0, 2 * np.pi, plane)
    gt = np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1).astype(np.float32)
    err = np.exp(rng.uniform(np.log(1e-3), np.log(20.0), plane))                     # outliers and inliers
    ang = rng.uniform(0, 2 * np.pi, plane)
    pred = (gt + np.stack([err * np.cos(ang), err * np.sin(ang)], 1)).astype(np.float32)
    same = rng.random(plane) < 0.05
    pred = np.where(same[:, None], gt, pred)                                         # epe == 0, ae == 0
    flat = lambda a: a.reshape(N, -1)
    hw = H * W
    if hw >= 30:
        pick = rng.permutation(hw)[:12]
        gu, gv, pu, pv = flat(gt[:, 0]), flat(gt[:, 1]), flat(pred[:, 0]), flat(pred[:, 1])
        gu[0, pick[0]] = np.nan                                                      # missing ground truth: one component, both, the .flo marker
        gu[0, pick[1]] = gv[0, pick[1]] = np.nan
        gv[0, pick[2]] = 1e10
        gu[0, pick[3]] = -1e10
        pu[0, pick[2]] = np.nan                                                      # a NaN prediction where there is no ground truth: not counted at all
        pu[0, pick[4]] = np.inf                                                      # non-finite predictions at valid pixels
        pv[0, pick[5]] = -np.inf
        pu[0, pick[6]] = pv[0, pick[6]] = np.nan
        pv[0, pick[7]] = np.nan
        gt = np.stack([gu.reshape(plane), gv.reshape(plane)], 1)
        pred = np.stack([pu.reshape(plane), pv.reshape(plane)], 1)
    valid = occ = None
    if masks:
        valid = (rng.random((N, 1, H, W)) < 0.8).astype(np.float32) * rng.choice([1.0, 2.5, -1.0], (N, 1, H, W)).astype(np.float32)
        occ = (rng.random((N, 1, H, W)) < 0.3).astype(np.float32) * rng.choice([1.0, 255.0], (N, 1, H, W)).astype(np.float32)
        if hw >= 30:
            valid.reshape(N, -1)[0, pick[4:8]] = 1.0                                 # the non-finite predictions sit at valid pixels
            valid.reshape(N, -1)[0, pick[8]] = 0.0
        elif N == 1:
            valid[:] = 1.0
    if N >= 2:
        if masks:
            valid[-1] = 0.0                                                          # the last sample has no valid pixel
        else:
            gt[-1, 0] = np.nan
    return pred.astype(np.float32), gt.astype(np.float32), valid, occ


def make_case(shape, seed, masks=True):
    """(pred, gt, valid, occ) float32: ground truth of 0.05 .. 80 px in every direction, errors of 1e-3 .. 20 px and exact zeros; where the
    plane has 30 pixels or more NaN and 1e10 ground truth, +-Inf and NaN predictions; with N >= 2 a last sample without a valid pixel;
    masks with non-zero values other than 1.  A draw that has a counted pixel on an edge (clear_of_edges) is drawn again with another seed."""
    for k in range(50):
        case = _draw(shape, seed + 1000 * k, masks)
        if clear_of_edges(*case):
            return case
    raise AssertionError(f"no draw of {shape} clear of the classification edges")


# ---- the raw C ABI -----------------------------------------------------------------------------------------------------------------
def f(x):
    return C.c_float(float(x))


def ptr(t):
    """Device (torch) tensor, ctypes buffer, int address or None -> c_void_p."""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, int):
        return C.c_void_p(t)
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(C.addressof(t))


def sizes(N, H, W):
    nbytes, k = C.c_size_t(), C.c_int()
    assert _lib.lib().fn2_flow_metrics_sizes(int(N), int(H), int(W), C.byref(nbytes), C.byref(k)) == OK
    return nbytes.value, k.value


def call(pred, gt, valid, occ, shape, results, epe_map, ws, ws_bytes, outlier=OUTLIER, bands=BANDS, stream=None):
    N, _, H, W = shape
    return _lib.lib().fn2_flow_metrics(ptr(pred), ptr(gt), ptr(valid), ptr(occ), int(N), int(H), int(W), f(outlier[0]), f(outlier[1]), f(bands[0]),
                                       f(bands[1]), ptr(results), ptr(epe_map), ptr(ws), int(ws_bytes), stream)


def refusals(pred, gt, valid, occ, results, epe_map, ws, ws_bytes):
    """(label, expected status, thunk) for every call the header says is refused on the host, for shape [2,2,5,7].  The pointers may be
    device tensors or any non-null host addresses: a refusal dereferences none of them."""
    S, nan = (2, 2, 5, 7), float("nan")
    out = []

    def add(label, want, pred_=pred, gt_=gt, results_=results, shape=S, outlier=OUTLIER, bands=BANDS, ws_=ws, nbytes=ws_bytes):
        out.append((label, want, lambda: call(pred_, gt_, valid, occ, shape, results_, epe_map, ws_, nbytes, outlier, bands)))

    add("pred NULL", INVALID, pred_=None)
    add("gt NULL", INVALID, gt_=None)
    add("results NULL", INVALID, results_=None)
    add("N = 0", INVALID, shape=(0, 2, 5, 7))
    add("N < 0", INVALID, shape=(-2, 2, 5, 7))
    add("H = 0", INVALID, shape=(2, 2, 0, 7))
    add("W < 0", INVALID, shape=(2, 2, 5, -7))
    add("2^31 elements", INVALID, shape=(1 << 10, 2, 1 << 10, 1 << 10))
    add("N 2 H W wraps to 0 in 64 bits", INVALID, shape=(1 << 22, 2, 1 << 21, 1 << 21))
    add("H W alone is 2^30", INVALID, shape=(1, 2, 1 << 15, 1 << 15))
    add("every extent the largest int", INVALID, shape=(2 ** 31 - 1, 2, 2 ** 31 - 1, 2 ** 31 - 1))
    add("outlier_abs NaN", INVALID, outlier=(nan, 0.05))
    add("outlier_abs < 0", INVALID, outlier=(-3.0, 0.05))
    add("outlier_rel NaN", INVALID, outlier=(3.0, nan))
    add("outlier_rel < 0", INVALID, outlier=(3.0, -0.05))
    add("band0 NaN", INVALID, bands=(nan, 40.0))
    add("band0 < 0", INVALID, bands=(-1.0, 40.0))
    add("band1 NaN", INVALID, bands=(10.0, nan))
    add("band1 < 0", INVALID, bands=(-20.0, -10.0))
    add("band0 == band1", INVALID, bands=(10.0, 10.0))
    add("band0 > band1", INVALID, bands=(40.0, 10.0))
    add("workspace NULL", WORKSPACE, ws_=None)
    add("workspace too small", WORKSPACE, nbytes=ws_bytes - 1)
    return out
