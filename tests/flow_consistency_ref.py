"""Forward-backward consistency references for the tests: the arithmetic of include/flownet2_hip_flow_consistency.h op by op in NumPy
float32 (ref32: the maps, which the kernel must equal bit for bit, and the rows), a float64 evaluation of ERR_SUM with an error bound from
the operation count (err_sum_bound), seeded inputs (make_case) and the raw C ABI calls.  No file of the reference tree is read, and no
tolerance here comes from the kernel's output.

ref32 rounds once per NumPy operation: every array is float32 and every scalar an np.float32, so a + b, a * b and np.sqrt (correctly
rounded) are the kernel's operations (which are compiled without contraction) in the kernel's association.

The bound on ERR_SUM, with U = 2^-24 (every fp32 operation: half an ulp, relative U; sqrtf is correctly rounded, so U as well).  Starred
values are the float64 evaluation's.  Inputs are float32 and exact.  x2 = float(x) + au and y2 are PART of the function (they choose the
taps, as in FlowWarp), so the float64 evaluation starts from the float32 x2, y2; al = x2 - ixL and be are then exact (x2 and ixL lie
within a factor of two of each other or ixL = 0), and so is which pixels have an err at all.

  b = ((wTL TL + wTR TR) + wBL BL) + wBR BR   a weight: two subtractions from 1 and a product (3 roundings), its product with the tap (1),
                                               up to three additions (3); the terms may differ in sign, so relative to the sum of their
                                               magnitudes:                                   d_b = ((1 + U)^7 - 1) sum w* |T|
  su = au + bu                                 d_su = d_b + U (|su*| + d_b)
  su su                                        d_p = (2 |su*| d_su + d_su^2) (1 + U) + U su*^2
  s = su su + sv sv                            d_s = (d_pu + d_pv) (1 + U) + U s*
  err = sqrtf(s)                               |sqrt(s) - sqrt(s*)| <= min(d_s / sqrt(s*), sqrt(d_s)) =: d_r;  d_e = d_r + U (err* + d_r)
  ERR_SUM                                      sum of d_e over the pixels that have an err
  the fp64 additions: n of them, relative 2^-53 each on non-negative terms                   + n 2^-53 (sum*)
A few multiples of the smallest subnormal (TINY) cover products that underflow."""
import ctypes as C

import numpy as np

from flownet2_amd import _lib
from flownet2_amd.evaluate import CONSISTENCY_COL as COL, CONSISTENCY_FLAGS as FLAG, CONSISTENCY_K as K

U = 2.0 ** -24
TINY = 16 * 2.0 ** -149
OK, INVALID, WORKSPACE = 0, -1, -3
ALPHA, BETA = (0.01, 0.5), (0.01, 0.002)
F = np.float32
LIMIT = F(1e9)


def _ok(t):
    with np.errstate(invalid="ignore"):
        return np.abs(t) <= LIMIT                                                   # False for NaN and +-Inf


def _taps(a, H, W):
    """What both evaluations share, decided in float32 on the own flow a [N,2,H,W]: fin (step 1), inside (step 3), the tap indices and the
    exact al, be (step 4; 0 where the pixel is not inside)."""
    au, av = a[:, 0], a[:, 1]
    fin = _ok(au) & _ok(av)
    with np.errstate(invalid="ignore", over="ignore"):
        x2 = np.arange(W, dtype=F)[None, None, :] + au
        y2 = np.arange(H, dtype=F)[None, :, None] + av
        inside = fin & (x2 >= 0) & (y2 >= 0) & (x2 < F(W)) & (y2 < F(H))
    x2, y2 = np.where(inside, x2, F(0)), np.where(inside, y2, F(0))
    ixL, iyT = x2.astype(np.int32), y2.astype(np.int32)                             # truncation of a value in [0, W)
    ixR, iyB = np.minimum(ixL + 1, W - 1), np.minimum(iyT + 1, H - 1)
    al, be = x2 - ixL.astype(F), y2 - iyT.astype(F)
    assert al.dtype == F and be.dtype == F and ixL.min() >= 0 and ixR.max() <= W - 1 and iyT.min() >= 0 and iyB.max() <= H - 1
    return fin, inside, (ixL, ixR, iyT, iyB), al, be


def _gather(o, c, iy, ix):
    return o[np.arange(o.shape[0])[:, None, None], c, iy, ix]


def direction32(a, o, alpha=ALPHA, beta=BETA):
    """One direction, a checked against o (both float32 [N,2,H,W]): dict of flags uint8 [N,1,H,W], occ, err float32 [N,1,H,W], warped
    float32 [N,2,H,W]."""
    a, o = np.ascontiguousarray(a, F), np.ascontiguousarray(o, F)
    N, _, H, W = a.shape
    a1, a2, b1, b2 = (F(v) for v in (*alpha, *beta))
    au, av = a[:, 0], a[:, 1]
    fin, inside, (ixL, ixR, iyT, iyB), al, be = _taps(a, H, W)
    xl, xr = np.maximum(np.arange(W) - 1, 0), np.minimum(np.arange(W) + 1, W - 1)
    yt, yb = np.maximum(np.arange(H) - 1, 0), np.minimum(np.arange(H) + 1, H - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        nb = [au[:, :, xl], au[:, :, xr], au[:, yt], au[:, yb], av[:, :, xl], av[:, :, xr], av[:, yt], av[:, yb]]
        nb_ok = np.logical_and.reduce([_ok(t) for t in nb])
        half = F(0.5)
        ux, uy, vx, vy = half * (nb[1] - nb[0]), half * (nb[3] - nb[2]), half * (nb[5] - nb[4]), half * (nb[7] - nb[6])
        g = ((ux * ux + uy * uy) + vx * vx) + vy * vy
        mag = au * au + av * av
        boundary = fin & nb_ok & (g > b1 * mag + b2)
        one = F(1)
        wTL, wTR, wBL, wBR = (one - al) * (one - be), al * (one - be), (one - al) * be, al * be
        b = []
        for c in (0, 1):
            TL, TR, BL, BR = _gather(o, c, iyT, ixL), _gather(o, c, iyT, ixR), _gather(o, c, iyB, ixL), _gather(o, c, iyB, ixR)
            b.append(((wTL * TL + wTR * TR) + wBL * BL) + wBR * BR)
        bu, bv = b
        full = inside & _ok(bu) & _ok(bv)
        su, sv = au + bu, av + bv
        s = su * su + sv * sv
        m = mag + (bu * bu + bv * bv)
        inconsistent = full & (s > a1 * m + a2)
        err = np.where(full, np.sqrt(s), F(np.nan))
    assert all(t.dtype == F for t in (g, mag, bu, bv, s, m, err))
    nonfinite = ~fin | (inside & ~full)
    outside = fin & ~inside
    flags = (nonfinite * FLAG["NONFINITE"] + outside * FLAG["OUTSIDE"] + inconsistent * FLAG["INCONSISTENT"] + boundary * FLAG["BOUNDARY"]).astype(np.uint8)
    occ = (nonfinite | outside | inconsistent).astype(F)
    warped = np.stack([np.where(inside, bu, F(np.nan)), np.where(inside, bv, F(np.nan))], 1).astype(F)
    return dict(flags=flags[:, None], occ=occ[:, None], err=err[:, None].astype(F), warped=warped)


def rows_of(flags, occ, err):
    """[N + 1, K] float64 rows from one direction's maps: exact counts, ERR_SUM as the float64 sum of the float32 err, ERR_MAX exact."""
    N = flags.shape[0]
    rows = np.zeros((N + 1, K), np.float64)
    fl, e = flags.reshape(N, -1), err.reshape(N, -1).astype(np.float64)
    rows[:N, COL["PIXELS"]] = fl.shape[1]
    for name in ("NONFINITE", "OUTSIDE", "INCONSISTENT", "BOUNDARY"):
        rows[:N, COL[name]] = ((fl & FLAG[name]) != 0).sum(1)
    rows[:N, COL["OCCLUDED"]] = (occ.reshape(N, -1) != 0).sum(1)
    has = ~np.isnan(e)
    rows[:N, COL["ERR_SUM"]] = np.where(has, e, 0.0).sum(1)
    rows[:N, COL["ERR_MAX"]] = np.where(has, e, 0.0).max(1)
    rows[N] = rows[:N].sum(0)
    rows[N, COL["ERR_MAX"]] = rows[:N, COL["ERR_MAX"]].max()
    return rows


COUNT_COLUMNS = [COL[n] for n in ("PIXELS", "NONFINITE", "OUTSIDE", "INCONSISTENT", "OCCLUDED", "BOUNDARY")]


def ref32(fw, bw, alpha=ALPHA, beta=BETA):
    """Both directions: [direction32(fw, bw), direction32(bw, fw)], each with its `rows` [N + 1, K]."""
    out = [direction32(fw, bw, alpha, beta), direction32(bw, fw, alpha, beta)]
    for d in out:
        d["rows"] = rows_of(d["flags"], d["occ"], d["err"])
    return out


def err_sum_bound(a, o):
    """One direction in float64 from the float32 x2, y2 (module docstring): (ERR_SUM* [N + 1], bound on |computed - ERR_SUM*| [N + 1]).
    Asserts that no sampled value lies within relative 1e-5 of the 1e9 limit, so both evaluations give the same pixels an err."""
    a, o = np.ascontiguousarray(a, F), np.ascontiguousarray(o, F)
    N, _, H, W = a.shape
    fin, inside, (ixL, ixR, iyT, iyB), al, be = _taps(a, H, W)
    al, be = al.astype(np.float64), be.astype(np.float64)
    o64 = np.where(np.isfinite(o), o, 0).astype(np.float64)
    bad = ~np.isfinite(o)
    w = [(1 - al) * (1 - be), al * (1 - be), (1 - al) * be, al * be]
    idx = [(iyT, ixL), (iyT, ixR), (iyB, ixL), (iyB, ixR)]
    tap_bad = np.zeros(inside.shape, bool)
    b, A = [], []
    for c in (0, 1):
        T = [_gather(o64, c, iy, ix) for iy, ix in idx]
        for iy, ix in idx:
            tap_bad |= _gather(bad, c, iy, ix)
        b.append(sum(wi * Ti for wi, Ti in zip(w, T)))
        A.append(sum(wi * np.abs(Ti) for wi, Ti in zip(w, T)))
    full = inside & ~tap_bad & (np.abs(b[0]) <= 1e9) & (np.abs(b[1]) <= 1e9)
    near = inside & ~tap_bad & ((np.abs(np.abs(b[0]) - 1e9) < 1e4) | (np.abs(np.abs(b[1]) - 1e9) < 1e4))
    assert not near.any(), "a sampled value on the 1e9 limit"
    e7 = (1 + U) ** 7 - 1
    a64 = np.where(fin[:, None], a, 0).astype(np.float64)
    d_p, s = [], 0.0
    for c in (0, 1):
        su = a64[:, c] + b[c]
        d_b = e7 * A[c] + TINY
        d_su = d_b + U * (np.abs(su) + d_b)
        d_p.append((2 * np.abs(su) * d_su + d_su ** 2) * (1 + U) + U * su ** 2 + TINY)
        s = s + su ** 2
    d_s = (d_p[0] + d_p[1]) * (1 + U) + U * s
    err = np.sqrt(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        d_r = np.minimum(np.where(s > 0, d_s / np.where(s > 0, err, 1.0), np.inf), np.sqrt(d_s))
    d_e = d_r + U * (err + d_r) + TINY
    tot = lambda v: np.where(full, v, 0.0).reshape(N, -1).sum(1)
    ref, bnd = tot(err), tot(d_e)
    bnd = bnd + H * W * 2.0 ** -53 * ref
    ref_all, bnd_all = np.append(ref, ref.sum()), np.append(bnd, bnd.sum() + N * 2.0 ** -53 * ref.sum())
    return ref_all, bnd_all, full


def make_case(shape, seed, occluder=True):
    """(fw, bw) float32 [N,2,H,W]: a smooth forward flow of a few pixels, the backward flow close to its negative (so most pixels are
    consistent, with sub-pixel targets everywhere), and a pasted rectangle that moves differently in the forward flow alone."""
    N, _, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fw = np.zeros(shape, np.float64)
    for n in range(N):
        for c in range(2):
            amp, fx, fy, ph = rng.uniform(0.5, 3.0), rng.uniform(0.02, 0.2), rng.uniform(0.02, 0.2), rng.uniform(0, 6.28, 2)
            fw[n, c] = amp * np.sin(fx * x + ph[0]) * np.cos(fy * y + ph[1]) + rng.uniform(-1.5, 1.5)
    bw = -fw + rng.normal(0, 0.05, shape)
    if occluder and H >= 3 and W >= 4:
        y0, x0, h, w = H // 4, W // 4, max(1, H // 3), max(1, W // 3)
        fw[:, 0, y0:y0 + h, x0:x0 + w] += 4.0
        fw[:, 1, y0:y0 + h, x0:x0 + w] -= 2.5
    return fw.astype(F), bw.astype(F)


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
    assert _lib.lib().fn2_flow_consistency_sizes(int(N), int(H), int(W), C.byref(nbytes), C.byref(k)) == OK
    return nbytes.value, k.value


def call(fw, bw, shape, results, ws, ws_bytes, alpha=ALPHA, beta=BETA, flags=(None, None), occ=(None, None), err=(None, None),
         warped=(None, None), stream=None):
    N, _, H, W = shape
    return _lib.lib().fn2_flow_consistency(ptr(fw), ptr(bw), int(N), int(H), int(W), f(alpha[0]), f(alpha[1]), f(beta[0]), f(beta[1]),
                                           ptr(results), ptr(flags[0]), ptr(flags[1]), ptr(occ[0]), ptr(occ[1]), ptr(err[0]), ptr(err[1]),
                                           ptr(warped[0]), ptr(warped[1]), ptr(ws), int(ws_bytes), stream)


def refusals(fw, bw, results, outs, ws, ws_bytes):
    """(label, expected status, the argument the error string must name, thunk) for every call the header says is refused on the host,
    for shape [2,2,5,7].  outs: dict of the optional output pairs.  The pointers may be device tensors or any non-null host addresses: a
    refusal dereferences none of them."""
    S, nan = (2, 2, 5, 7), float("nan")
    out = []

    def add(label, want, names, fw_=fw, bw_=bw, results_=results, shape=S, alpha=ALPHA, beta=BETA, ws_=ws, nbytes=ws_bytes):
        out.append((label, want, names, lambda: call(fw_, bw_, shape, results_, ws_, nbytes, alpha, beta, **outs)))

    add("fw NULL", INVALID, "fw", fw_=None)
    add("bw NULL", INVALID, "bw", bw_=None)
    add("results NULL", INVALID, "results", results_=None)
    add("N = 0", INVALID, "shape", shape=(0, 2, 5, 7))
    add("N < 0", INVALID, "shape", shape=(-2, 2, 5, 7))
    add("H = 0", INVALID, "shape", shape=(2, 2, 0, 7))
    add("W < 0", INVALID, "shape", shape=(2, 2, 5, -7))
    add("2^31 elements", INVALID, "2^31", shape=(1 << 10, 2, 1 << 10, 1 << 10))
    add("N 2 H W wraps to 0 in 64 bits", INVALID, "2^31", shape=(1 << 22, 2, 1 << 21, 1 << 21))
    add("H W alone is 2^30", INVALID, "2^31", shape=(1, 2, 1 << 15, 1 << 15))
    add("every extent the largest int", INVALID, "2^31", shape=(2 ** 31 - 1, 2, 2 ** 31 - 1, 2 ** 31 - 1))
    add("alpha1 NaN", INVALID, "alpha1", alpha=(nan, 0.5))
    add("alpha1 < 0", INVALID, "alpha1", alpha=(-0.01, 0.5))
    add("alpha2 NaN", INVALID, "alpha2", alpha=(0.01, nan))
    add("alpha2 < 0", INVALID, "alpha2", alpha=(0.01, -0.5))
    add("beta1 NaN", INVALID, "beta1", beta=(nan, 0.002))
    add("beta1 < 0", INVALID, "beta1", beta=(-0.01, 0.002))
    add("beta2 NaN", INVALID, "beta2", beta=(0.01, nan))
    add("beta2 < 0", INVALID, "beta2", beta=(0.01, -0.002))
    add("workspace NULL", WORKSPACE, "workspace", ws_=None)
    add("workspace too small", WORKSPACE, "workspace", nbytes=ws_bytes - 1)
    return out
