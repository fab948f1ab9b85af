"""Flow-visualisation references for the tests: the arithmetic of include/flownet2_hip_flow_visualize.h op by op in NumPy float32 (color32,
error_map32), the same functions evaluated in float64 with a bound on |out32 - out64| from the operation count (color_bounds,
error_bounds), what bytes those allow (color_allowed, error_allowed), seeded inputs and the raw C ABI calls.  No file of the reference tree
is read, and no tolerance here comes from the kernel's output.

The float32 restatements round once per NumPy operation: every array is float32 and every scalar an np.float32.  They are the kernel's
operations in the kernel's association, except that np.arctan2 and the device's atan2f (and, should it not be correctly rounded, sqrtf)
may differ in the last places; that is what the bounds are for.

The bounds, with U = 2^-24 (every fp32 operation: half an ulp, relative U) and R = 2 U E_POW for sqrtf and atan2f, the term
flow_metrics_ref.py uses (lpq_ref.E_POW).  Starred values are the float64 evaluation's.  Inputs are float32 and exact.

Colour coding, per pixel and channel:
  rad = sqrtf(u u + v v)       two exact-input products and an addition of non-negative terms under the root, halved by it, R on top:
                               e_r = (1 + ((1 + U)^2 - 1))^1/2 (1 + R) - 1
  maxrad                       |max a - max b| <= max |a - b|: relative e_r as well (exact, a float32 argument, under NORM_FIXED)
  rn = rad / maxrad            e_n = (1 + e_r) / (1 - e_r) (1 + U) - 1 (NORM_FIXED: (1 + e_r) (1 + U) - 1);  d_rn = e_n rn*
      d_rn = 0 where rad is 0 (0 / maxrad is 0) and at the maximum pixel: x / x is exactly 1 in float32 as in float64.  The maximum pixel
      is the same pixel on both sides where every other known pixel of the normalisation group has rn* < 1 - 4 e_r or holds the same
      {|u|, |v|} (the same radius to the bit); only there is d_rn set to 0.  ("delta is 0 at the sample's maximum pixel" is read as this:
      the pixel's rn, and with it its branch, is exact; its channels still carry the error of the angle unless they are saturated.)
      Under NORM_SAMPLE and NORM_BATCH rn <= 1 on both sides always (rad <= maxrad and a correctly rounded quotient), so the
      out-of-range branch is taken under NORM_FIXED only.
  t = atan2f(-v, -u)           d_t = R |t*|
  a = t / PI_F                 PI_F is not pi: E_PI = |PI_F - pi| / pi;  d_a = |a*| ((1 + R) (1 + U) / (1 - E_PI) - 1)
  s = a + 1                    d_s = d_a + U (|s*| + d_a)
  fk = (s 0.5) 54              the halving is exact;  d_fk = 54 d_s / 2 + U (fk* + 54 d_s / 2)
  k0, f, c                     c is a continuous piecewise-linear function of fk (at an integer fk both neighbouring segments give the node's
                               value, at fk = 54 the wrap gives entry 54 from both sides), f = fk - k0 is exact, so a k0 that differs from
                               k0* changes nothing beyond the slope:  with L the largest |w1 - w0| of the segment of fk* and, where fk* lies
                               within d_fk of a segment end, of that neighbour too:
                               d_c = L d_fk + U L + U (c* + L d_fk + U L), and d_c = 0 where L = 0 (w0 + f 0 is w0 exactly)
  m = 255 - c                  d_m = d_c + U (m* + d_c); 0 where d_c = 0 (integers)
  p = rn m                     d_p0 = rn* d_m + m* d_rn + d_rn d_m;  d_p = d_p0 + U (p* + d_p0); 0 where d_p0 = 0 and p* = 0
  out = 255 - p                delta = d_p + U (out* + d_p); 0 where d_p = 0 (then p is exactly 0)
  out = 0.75 c (rn > 1)        delta = 0.75 d_c + U (out* + 0.75 d_c); 0 where d_c = 0 (three quarters of an integer below 256 is exact)
So delta is 0 where rn = 0 (zero flow: white bit for bit) and for a channel with w0 = w1 = 255 well inside its segment (255 bit for bit).
A few multiples of the smallest subnormal (TINY) cover underflow wherever delta is not 0.

Error image: epe and mag as in flow_metrics_ref.py (e_e, e_m);  na = epe / abs_thresh: e_na = (1 + e_e) (1 + U) - 1;
nr = (epe / mag) / rel_thresh: e_nr = (1 + e_e) / (1 - e_m) (1 + U)^2 - 1;  n = fminf(na, nr) lies in
[min(na* - d_na, nr* - d_nr), min(na* + d_na, nr* + d_nr)].  The thresholds are float32 arguments and exact.  A pixel whose interval
holds a bin edge may take either neighbouring bin's colour; every other pixel must have its bin's colour, and black, the last bin of a
NaN prediction and the halving under occ are decided on the inputs' bits and exact."""
import ctypes as C

import numpy as np

import lpq_ref as LR
from flownet2_amd import _lib

U = LR.U
R = 2.0 * U * LR.E_POW
TINY = 16 * 2.0 ** -149
OK, INVALID, WORKSPACE = 0, -1, -3
F = np.float32
LIMIT = F(1e9)
PI_F = F(3.14159265358979323846)
E_PI = abs(float(PI_F) - np.pi) / np.pi
NORM = {n[len("FN2_FLOW_COLOR_NORM_"):]: v for n, v in _lib.FLOW_VISUALIZE_CONSTANTS.items()}      # SAMPLE, BATCH, FIXED
ABS_THRESH, REL_THRESH = 3.0, 0.05


def make_wheel():
    """[55, 3] integers, from the segment lengths and integer division."""
    w = []
    w += [(255, 255 * i // 15, 0) for i in range(15)]             # RY
    w += [(255 - 255 * i // 6, 255, 0) for i in range(6)]         # YG
    w += [(0, 255, 255 * i // 4) for i in range(4)]               # GC
    w += [(0, 255 - 255 * i // 11, 255) for i in range(11)]       # CB
    w += [(255 * i // 13, 0, 255) for i in range(13)]             # BM
    w += [(255, 0, 255 - 255 * i // 6) for i in range(6)]         # MR
    return np.array(w, np.int32)


WHEEL = make_wheel()
EDGES = np.array([0.0625, 0.125, 0.25, 0.5, 1, 2, 4, 8, 16], np.float64)
BIN_COLORS = np.array([(49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248), (254, 224, 144), (253, 174, 97),
                       (244, 109, 67), (215, 48, 39), (165, 0, 38)], np.uint8)


def _ok(t):
    with np.errstate(invalid="ignore"):
        return np.abs(t) <= LIMIT                                                   # False for NaN and +-Inf


def _known(flow):
    return _ok(flow[:, 0]) & _ok(flow[:, 1])


# ---- the colour coding -----------------------------------------------------------------------------------------------------------------
def maxrad32(flow, norm, max_flow=None):
    """The float32 [N] radius each sample is divided by."""
    flow = np.ascontiguousarray(flow, F)
    N = flow.shape[0]
    if norm == NORM["FIXED"]:
        return np.full(N, F(max_flow), F)
    known = _known(flow)
    u, v = np.where(known, flow[:, 0], F(0)), np.where(known, flow[:, 1], F(0))
    m = np.sqrt(u * u + v * v).reshape(N, -1).max(1)
    if norm == NORM["BATCH"]:
        m = np.full(N, m.max(), F)
    return np.where(m > 0, m, F(1)).astype(F)


def color32(flow, norm=0, max_flow=None):
    """(uint8 [N,H,W,3], float32 [N] maxrad) op by op in float32."""
    flow = np.ascontiguousarray(flow, F)
    known = _known(flow)
    u, v = np.where(known, flow[:, 0], F(0)), np.where(known, flow[:, 1], F(0))
    maxrad = maxrad32(flow, norm, max_flow)
    rn = np.sqrt(u * u + v * v) / maxrad[:, None, None]
    a = np.arctan2(-v, -u) / PI_F
    fk = ((a + F(1)) * F(0.5)) * F(54)
    k0 = np.clip(fk.astype(np.int32), 0, 54)
    k1 = (k0 + 1) % 55
    f = fk - k0.astype(F)
    assert rn.dtype == F and fk.dtype == F and f.dtype == F
    out = np.zeros(flow.shape[:1] + flow.shape[2:] + (3,), np.uint8)
    for ch in range(3):
        w0, w1 = WHEEL[k0, ch].astype(F), WHEEL[k1, ch].astype(F)
        c = w0 + f * (w1 - w0)
        o = np.where(rn <= F(1), F(255) - rn * (F(255) - c), F(0.75) * c)
        assert o.dtype == F
        out[..., ch] = np.where(known, o.astype(np.int32), 0).astype(np.uint8)
    return out, maxrad


def color_bounds(flow, norm=0, max_flow=None):
    """The float64 evaluation and the module docstring's bounds: dict of known [N,H,W], rn, d_rn [N,H,W], either (the branch rn <= 1 is not
    decided), and per branch out / delta [N,H,W,3] (`in`: rn <= 1, `over`: rn > 1), maxrad [N]."""
    flow = np.ascontiguousarray(flow, F)
    N = flow.shape[0]
    known = _known(flow)
    u = np.where(known, flow[:, 0], F(0)).astype(np.float64)
    v = np.where(known, flow[:, 1], F(0)).astype(np.float64)
    rad = np.sqrt(u * u + v * v)
    fixed = norm == NORM["FIXED"]
    e_r = np.sqrt(1 + ((1 + U) ** 2 - 1)) * (1 + R) - 1
    if fixed:
        maxrad = np.full(N, float(F(max_flow)))
        e_n = (1 + e_r) * (1 + U) - 1
    else:
        maxrad = rad.reshape(N, -1).max(1)
        if norm == NORM["BATCH"]:
            maxrad = np.full(N, maxrad.max())
        maxrad = np.where(maxrad > 0, maxrad, 1.0)
        e_n = (1 + e_r) / (1 - e_r) * (1 + U) - 1
    rn = rad / maxrad[:, None, None]
    d_rn = e_n * rn + np.where(rn > 0, TINY, 0.0)
    if not fixed:
        # the maximum pixel(s): exact where nothing else comes close, or what comes close is the same radius to the bit
        au, av = np.minimum(np.abs(u), np.abs(v)), np.maximum(np.abs(u), np.abs(v))
        groups = [slice(None)] if norm == NORM["BATCH"] else [slice(n, n + 1) for n in range(N)]
        for g in groups:
            top = known[g] & (rn[g] == 1.0)
            if not top.any():
                continue
            lo, hi = au[g][top], av[g][top]
            same = (au[g] == lo[0]) & (av[g] == hi[0])
            if np.all(lo == lo[0]) and np.all(hi == hi[0]) and not (known[g] & ~same & (rn[g] >= 1 - 4 * e_r)).any():
                d_rn[g] = np.where(same & known[g], 0.0, d_rn[g])
    with np.errstate(invalid="ignore"):
        t = np.arctan2(-v, -u)
    a = t / np.pi
    d_a = np.abs(a) * ((1 + R) * (1 + U) / (1 - E_PI) - 1)
    s = a + 1
    d_s = d_a + U * (np.abs(s) + d_a)
    fk = s * 0.5 * 54
    d_fk = 27 * d_s + U * (fk + 27 * d_s) + TINY
    k0 = np.clip(fk.astype(np.int64), 0, 54)
    k1 = (k0 + 1) % 55
    f = fk - k0
    near_lo, near_hi = f <= d_fk, f >= 1 - d_fk
    kb, ka = (k0 - 1) % 55, (k0 + 1) % 55                       # the segments before and after; past entry 54 the angle wraps to segment 0
    res = dict(known=known, rn=rn, d_rn=d_rn, maxrad=maxrad, either=known & (np.abs(rn - 1) <= d_rn) & (d_rn > 0))
    out_in, del_in, out_ov, del_ov = (np.zeros(rn.shape + (3,)) for _ in range(4))
    for ch in range(3):
        w = WHEEL[:, ch].astype(np.float64)
        slope = np.abs(w[(np.arange(55) + 1) % 55] - w)
        w0, w1 = w[k0], w[k1]
        L = np.maximum(slope[k0], np.maximum(np.where(near_lo, slope[kb], 0), np.where(near_hi, slope[ka], 0)))
        c = w0 + f * (w1 - w0)
        d_c = np.where(L > 0, L * d_fk + U * L + U * (c + L * d_fk + U * L) + TINY, 0.0)
        m = 255 - c
        d_m = np.where(d_c > 0, d_c + U * (m + d_c), 0.0)
        p = rn * m
        d_p0 = rn * d_m + m * d_rn + d_rn * d_m
        d_p = np.where((d_p0 == 0) & (p == 0), 0.0, d_p0 + U * (p + d_p0) + TINY)
        out_in[..., ch] = 255 - p
        del_in[..., ch] = np.where(d_p == 0, 0.0, d_p + U * (255 - p + d_p))
        out_ov[..., ch] = 0.75 * c
        del_ov[..., ch] = np.where(d_c == 0, 0.0, 0.75 * d_c + U * (0.75 * c + 0.75 * d_c) + TINY)
    res.update({"in": (out_in, del_in), "over": (out_ov, del_ov)})
    return res


def _byte_range(out, delta):
    lo = np.floor(np.maximum(out - delta, 0.0)).astype(np.int64)
    hi = np.floor(out + delta).astype(np.int64)
    return lo, np.maximum(hi, lo)


def color_allowed(flow, norm=0, max_flow=None):
    """What the bytes may be: (ranges: list of (lo, hi, applies) with byte in [lo, hi] allowed where applies; loose [N,H,W,3]: the values
    that are not pinned to one byte; bounds: color_bounds' dict).  A byte is right when it lies in one of the ranges that apply to it."""
    b = color_bounds(flow, norm, max_flow)
    known, rn, either = b["known"][..., None], b["rn"][..., None], b["either"][..., None]
    ranges, loose = [], np.zeros(b["in"][0].shape, bool)
    for key, takes in (("in", (rn <= 1) | either), ("over", (rn > 1) | either)):
        lo, hi = _byte_range(*b[key])
        applies = known & takes
        lo, hi = np.where(known, lo, 0), np.where(known, hi, 0)
        ranges.append((lo, hi, applies | ~known if key == "in" else applies))
        loose |= applies & (hi > lo)
    loose |= either
    return ranges, loose, b


def color_check(got, flow, norm=0, max_flow=None):
    """(number of wrong bytes, share of values left to a loose rule, the largest delta) of uint8 got [N,H,W,3]."""
    ranges, loose, b = color_allowed(flow, norm, max_flow)
    good = np.zeros(got.shape, bool)
    g = got.astype(np.int64)
    for lo, hi, applies in ranges:
        good |= applies & (g >= lo) & (g <= hi)
    delta = max(float(np.where(applies & b["known"][..., None], b[key][1], 0.0).max()) for key, (_, _, applies) in zip(("in", "over"), ranges))
    return int((~good).sum()), float(loose.mean()), delta


# ---- the error image -------------------------------------------------------------------------------------------------------------------
def _masks(pred, gt, valid, occ):
    use = _ok(gt[:, 0]) & _ok(gt[:, 1])
    if valid is not None:
        use &= np.asarray(valid)[:, 0] != 0
    fin = use & _ok(pred[:, 0]) & _ok(pred[:, 1])
    occluded = np.asarray(occ)[:, 0] != 0 if occ is not None else np.zeros(use.shape, bool)
    return use, fin, occluded


def _finish(bins, use, fin, occluded):
    rgb = BIN_COLORS[np.where(fin, bins, 9)]
    rgb = np.where(use[..., None], rgb, 0).astype(np.uint8)
    return np.where(occluded[..., None], (F(0.5) * rgb.astype(F)).astype(np.int32), rgb).astype(np.uint8)


def error_map32(pred, gt, valid=None, occ=None, abs_thresh=ABS_THRESH, rel_thresh=REL_THRESH):
    """uint8 [N,H,W,3] op by op in float32."""
    pred, gt = np.ascontiguousarray(pred, F), np.ascontiguousarray(gt, F)
    use, fin, occluded = _masks(pred, gt, valid, occ)
    z = lambda t: np.where(fin, t, F(0))
    pu, pv, gu, gv = z(pred[:, 0]), z(pred[:, 1]), z(gt[:, 0]), z(gt[:, 1])
    du, dv = pu - gu, pv - gv
    epe = np.sqrt(du * du + dv * dv)
    mag = np.sqrt(gu * gu + gv * gv)
    n = epe / F(abs_thresh)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(mag > 0, np.fmin(n, (epe / np.where(mag > 0, mag, F(1))) / F(rel_thresh)), n)
    assert n.dtype == F
    bins = (n[..., None] >= EDGES.astype(F)).sum(-1)
    return _finish(bins, use, fin, occluded)


def error_bounds(pred, gt, valid=None, occ=None, abs_thresh=ABS_THRESH, rel_thresh=REL_THRESH):
    """The float64 evaluation: dict of n [N,H,W], its interval (lo, hi), and the masks."""
    pred, gt = np.ascontiguousarray(pred, F), np.ascontiguousarray(gt, F)
    use, fin, occluded = _masks(pred, gt, valid, occ)
    z = lambda t: np.where(fin, t, F(0)).astype(np.float64)
    pu, pv, gu, gv = z(pred[:, 0]), z(pred[:, 1]), z(gt[:, 0]), z(gt[:, 1])
    at, rt = float(F(abs_thresh)), float(F(rel_thresh))
    du, dv = pu - gu, pv - gv
    epe = np.sqrt(du * du + dv * dv)
    mag = np.sqrt(gu * gu + gv * gv)
    e_s = (1 + U) ** 4 - 1
    e_e = (1 - e_s) ** -0.5 * (1 + R) - 1
    e_m = (1 - ((1 + U) ** 2 - 1)) ** -0.5 * (1 + R) - 1
    na = epe / at
    d_na = ((1 + e_e) * (1 + U) - 1) * na + np.where(na > 0, TINY, 0.0)
    has = mag > 0
    nr = np.where(has, epe / np.where(has, mag, 1.0) / rt, np.inf)
    d_nr = np.where(has, ((1 + e_e) / (1 - e_m) * (1 + U) ** 2 - 1) * np.where(has, nr, 0.0) + np.where(nr > 0, TINY, 0.0), 0.0)
    n = np.minimum(na, nr)
    lo = np.maximum(np.minimum(na - d_na, nr - d_nr), 0.0)
    hi = np.minimum(na + d_na, nr + d_nr)
    return dict(n=n, lo=lo, hi=hi, use=use, fin=fin, occluded=occluded)


def error_check(got, pred, gt, valid=None, occ=None, abs_thresh=ABS_THRESH, rel_thresh=REL_THRESH):
    """(number of wrong pixels, share of pixels left to the either-bin rule) of uint8 got [N,H,W,3]."""
    b = error_bounds(pred, gt, valid, occ, abs_thresh, rel_thresh)
    bin_lo, bin_hi = (b["lo"][..., None] >= EDGES).sum(-1), (b["hi"][..., None] >= EDGES).sum(-1)
    assert np.all(bin_hi - bin_lo <= 1), "an interval spans a whole bin"
    a, c = _finish(bin_lo, b["use"], b["fin"], b["occluded"]), _finish(bin_hi, b["use"], b["fin"], b["occluded"])
    good = (got == a).all(-1) | (got == c).all(-1)
    return int((~good).sum()), float((b["fin"] & (bin_hi != bin_lo)).mean())


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def smooth_flow(shape, seed, scale=1.0):
    """float32 [N,2,H,W]: per sample and channel a smooth wave of a few pixels plus noise, so that every direction and radius occurs."""
    N, _, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros(shape, np.float64)
    for n in range(N):
        for c in range(2):
            amp, fx, fy, ph = rng.uniform(1.0, 4.0), rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4), rng.uniform(0, 6.28, 2)
            out[n, c] = amp * np.sin(fx * x + ph[0]) * np.cos(fy * y + ph[1]) + rng.uniform(-1.0, 1.0)
    out += rng.normal(0, 0.3, shape)
    return (out * scale).astype(F)


def error_case(shape, seed):
    """(pred, gt, valid, occ): a smooth ground truth and a prediction whose error spans every bin; an eighth of the pixels with
    pred - gt = (m abs_thresh / 16, 0) for an integer m (float32 arithmetic is exact there), a few of those over gt = 0 (mag == 0: the
    absolute term alone); NaN / Inf / 1e10 in both; valid 0 and occ 1 on a share of the pixels."""
    N, _, H, W = shape
    rng = np.random.default_rng(seed)
    gt = smooth_flow(shape, seed + 1, scale=4.0)
    err = rng.normal(0, 1.0, shape) * np.exp(rng.uniform(-4, 4, (N, 1, H, W)))
    pred = (gt + err).astype(F)
    exact = rng.random((N, H, W)) < 0.125
    zero_gt = exact & (rng.random((N, H, W)) < 0.25)
    gt[:, 0][exact] = np.round(gt[:, 0][exact] * 4) / 4                                # quarter pixels: the sum below is exact
    gt[:, 1][exact] = np.round(gt[:, 1][exact] * 4) / 4
    gt[:, 0][zero_gt] = 0
    gt[:, 1][zero_gt] = 0
    m = rng.integers(0, 48, (N, H, W)).astype(F)
    pred[:, 0][exact] = (gt[:, 0] + m * F(ABS_THRESH / 16))[exact]
    pred[:, 1][exact] = gt[:, 1][exact]
    flat_p, flat_g = pred.reshape(-1), gt.reshape(-1)
    bad = [np.nan, np.inf, -np.inf, 1e10, -1e10]
    if flat_p.size >= 60:
        for k, pos in enumerate(rng.permutation(flat_p.size)[:10]):
            (flat_p if k % 2 else flat_g)[pos] = bad[k % 5]
    valid = (rng.random((N, 1, H, W)) < 0.9).astype(F)
    occ = (rng.random((N, 1, H, W)) < 0.2).astype(F)
    return pred, gt.astype(F), valid, occ


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
    nbytes = C.c_size_t()
    assert _lib.lib().fn2_flow_visualize_sizes(int(N), int(H), int(W), C.byref(nbytes)) == OK
    return nbytes.value


def chunks(H, W):
    return min(-(-H * W // 1024), 128)


def call_color(flow, shape, rgb, norm=0, max_flow=0.0, maxrad_out=None, ws=None, ws_bytes=0, stream=None):
    N, _, H, W = shape
    return _lib.lib().fn2_flow_color(ptr(flow), int(N), int(H), int(W), int(norm), f(max_flow), ptr(rgb), ptr(maxrad_out), ptr(ws),
                                     int(ws_bytes), stream)


def call_error(pred, gt, shape, rgb, valid=None, occ=None, abs_thresh=ABS_THRESH, rel_thresh=REL_THRESH, stream=None):
    N, _, H, W = shape
    return _lib.lib().fn2_flow_error_map(ptr(pred), ptr(gt), ptr(valid), ptr(occ), int(N), int(H), int(W), f(abs_thresh), f(rel_thresh),
                                         ptr(rgb), stream)


BAD_SHAPES = [("N = 0", (0, 2, 5, 7), "shape"), ("N < 0", (-2, 2, 5, 7), "shape"), ("H = 0", (2, 2, 0, 7), "shape"),
              ("W < 0", (2, 2, 5, -7), "shape"), ("2^31 elements", (1 << 10, 2, 1 << 10, 1 << 10), "2^31"),
              ("N 2 H W wraps to 0 in 64 bits", (1 << 22, 2, 1 << 21, 1 << 21), "2^31"), ("H W alone is 2^30", (1, 2, 1 << 15, 1 << 15), "2^31"),
              ("every extent the largest int", (2 ** 31 - 1, 2, 2 ** 31 - 1, 2 ** 31 - 1), "2^31")]


def refusals(flow, gt, valid, occ, rgb, maxrad_out, ws, ws_bytes):
    """(label, expected status, the prefix and the argument the error string must name, thunk) for every call the header says is refused
    on the host, for shape [2,2,5,7].  The pointers may be any non-null host addresses: a refusal dereferences none of them."""
    S, nan = (2, 2, 5, 7), float("nan")
    out = []

    def color(label, want, names, flow_=flow, rgb_=rgb, shape=S, norm=NORM["SAMPLE"], max_flow=0.0, ws_=ws, nbytes=ws_bytes):
        out.append(("color: " + label, want, "flow_color:", names,
                    lambda: call_color(flow_, shape, rgb_, norm, max_flow, maxrad_out, ws_, nbytes)))

    def error(label, want, names, pred_=flow, gt_=gt, rgb_=rgb, shape=S, at=ABS_THRESH, rt=REL_THRESH):
        out.append(("error: " + label, want, "flow_error_map:", names, lambda: call_error(pred_, gt_, shape, rgb_, valid, occ, at, rt)))

    color("flow NULL", INVALID, "flow", flow_=None)
    color("rgb NULL", INVALID, "rgb", rgb_=None)
    error("pred NULL", INVALID, "pred", pred_=None)
    error("gt NULL", INVALID, "gt", gt_=None)
    error("rgb NULL", INVALID, "rgb", rgb_=None)
    for label, shape, names in BAD_SHAPES:
        color(label, INVALID, names, shape=shape)
        error(label, INVALID, names, shape=shape)
    color("norm = 3", INVALID, "norm", norm=3)
    color("norm = -1", INVALID, "norm", norm=-1)
    color("max_flow NaN", INVALID, "max_flow", norm=NORM["FIXED"], max_flow=nan)
    color("max_flow = 0", INVALID, "max_flow", norm=NORM["FIXED"], max_flow=0.0)
    color("max_flow < 0", INVALID, "max_flow", norm=NORM["FIXED"], max_flow=-2.0)
    error("abs_thresh NaN", INVALID, "abs_thresh", at=nan)
    error("abs_thresh = 0", INVALID, "abs_thresh", at=0.0)
    error("abs_thresh < 0", INVALID, "abs_thresh", at=-3.0)
    error("rel_thresh NaN", INVALID, "rel_thresh", rt=nan)
    error("rel_thresh = 0", INVALID, "rel_thresh", rt=0.0)
    error("rel_thresh < 0", INVALID, "rel_thresh", rt=-0.05)
    for norm in ("SAMPLE", "BATCH"):
        color(f"workspace NULL ({norm})", WORKSPACE, "workspace", norm=NORM[norm], ws_=None)
        color(f"workspace too small ({norm})", WORKSPACE, "workspace", norm=NORM[norm], nbytes=ws_bytes - 1)
    return out
