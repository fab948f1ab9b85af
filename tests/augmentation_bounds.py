"""fp64 statements of DataAugmentation (csrc/data_augmentation.hip) and FlowAugmentation (csrc/augmentation.hip) with element-wise
error bounds, in plain NumPy float64, written from the formulas of the layers (data_augmentation_layer.cu:24-317, :452-637,
flow_augmentation_layer.cu:23-88).  Shares no code with oracle/ or csrc/; no file of the reference tree is read.

Inputs.  The fp32 blobs; the fp32 matrices ops.augmentation_matrix returns (the host function is held to the oracle bit for bit and to an
  fp64 composition in test_augmentation.py); the fp32 coefficient values after exp and clear_defaults, restated here (coeff_values).
  The matrix of DataAugmentation is built AFTER clear_defaults, the one of FlowAugmentation without it; coeff_values asserts that no
  spatial field of a case lies within 1e-3 of its default without being the default, so both are the same matrix.

Value and error.  Every quantity is a pair (v, e): the fp64 value and a first-order bound on |fp32 value - v| (class VE).  An fp32
  operation adds u |result| (u = 2^-24) and carries the incoming errors through the operation's derivative; min, max, abs and copysign
  are 1-Lipschitz and exact; sqrt and pow carry the incoming error through the function's values at the interval ends (they are
  monotone; the derivative is unbounded at 0).  powf adds E_POW ulps (tests/lpq_ref.py: measured on the MI355X over x in [1e-7, 1e4] and
  exponents in [-0.8, 2]; the statement records every argument and exponent, the tests assert that range).  ASSUMPTION: nobody has
  measured the device's cosf / sinf / logf; each gets E_POW ulps of its result too.  The FINAL bound of a colour chain is TWICE the
  first-order one (COLOUR_MARGIN): the margin for the higher-order terms; it is not fitted to anything.  A chain that only samples and
  subtracts the mean, and the flow chain, are sums of products: their higher orders are u^2 terms, margin 1 + 2^-10 (LINEAR_MARGIN).

Spatial sampling.  Position in fp64 from the fp32 matrix entries; ep = 3u(|x t0| + |y t2| + |t4|) (two fused or three plain roundings);
  clamp to [0, fp32(fp32(W) - 1.05f)] (1-Lipschitz).  The sample is continuous and piecewise bilinear in the position:
  e = ep_x Lx + ep_y Ly + 6u sum |w||tap|, Lx / Ly the largest tap differences over the at most 2 x 2 cells [pos - ep, pos + ep] touches.
  Nothing is excluded: a position within ep of an integer is covered by continuity.

Statistics.  max_rgb / min_rgb are exact; max_abs_eig within 3u sum |v||rgb|; mean_rgb within (d + 2) u A, A = sum |rgb| / (W H N),
  d from the launch plan (stats_plan, mean_depth); mean_eig and max_l follow as VE chains.

Thresholds.  s > 1e-2f and l > 1e-2f per pixel: a pixel whose fp64 s or l lies within COLOUR_MARGIN x its running error of the threshold
  is reported in `excluded`.  The batch thresholds (max_abs_eig[c], max_l against 1e-2f) and the shadow edge are asserted to be decided:
  a case keeps them away from the threshold by construction.

Flow.  pos1 with the same ep; tap = trunc(pos + 0.5) (toward zero); where pos + 0.5 is within its error of an integer both taps are
  admissible per axis: flow_statement returns up to four candidates.  Flat index row W + col without a per-axis clamp; reads below 0 or at
  or beyond src_count give 0.  Nothing is excluded.
"""
import math

import numpy as np

from lpq_ref import E_POW, U

COLOUR_MARGIN = 2.0
LINEAR_MARGIN = 1.0 + 2.0 ** -10
THR = float(np.float32(1e-2))
FLT_MAX = float(np.finfo(np.float32).max)
POW_ARG_RANGE, POW_EXP_RANGE = (1e-7, 1e4), (-0.8, 2.0)           # what E_POW was measured over (tests/lpq_ref.py)

FIELDS = ("mirror dx dy angle zoom_x zoom_y gamma brightness contrast color1 color2 color3 pow_nomean0 pow_nomean1 pow_nomean2 "
          "add_nomean0 add_nomean1 add_nomean2 mult_nomean0 mult_nomean1 mult_nomean2 pow_withmean0 pow_withmean1 pow_withmean2 "
          "add_withmean0 add_withmean1 add_withmean2 mult_withmean0 mult_withmean1 mult_withmean2 lmult_pow lmult_add lmult_mult col_angle "
          "fog_amount fog_size motion_blur_angle motion_blur_size shadow_angle shadow_distance shadow_strength noise").split()
F = {name: i for i, name in enumerate(FIELDS)}
DEFAULT = np.array([0, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
assert len(FIELDS) == 42 and F["col_angle"] == 33 and F["noise"] == 41


def coeff_array(N, per_sample=(), **fields):
    """[N,42] in the layout of coeff_to_array: the value itself for a field whose default is 0, its log for one whose default is 1.
    fields apply to every sample, per_sample = {n: {field: value}} on top."""
    a = np.zeros((N, 42), np.float32)
    def put(n, name, value):
        a[n, F[name]] = np.float32(value) if DEFAULT[F[name]] == 0 else np.float32(math.log(value))
    for n in range(N):
        for name, value in fields.items():
            put(n, name, value)
    for n, d in dict(per_sample).items():
        for name, value in d.items():
            put(n, name, value)
    return a


def coeff_values(arr):
    """array_to_coeff (exp in double, stored as float) and clear_defaults (within 1e-3 of the default -> the default): [N,42] fp32."""
    arr = np.asarray(arr, np.float32).reshape(-1, 42)
    v = np.where(DEFAULT == 0, arr, np.exp(arr.astype(np.float64)).astype(np.float32)).astype(np.float32)
    near = np.abs((DEFAULT - v).astype(np.float32)).astype(np.float64) < 1e-3
    out = np.where(near, DEFAULT, v).astype(np.float32)
    assert np.array_equal(out[:, :6], v[:, :6]), "a spatial field within 1e-3 of its default: the two layers' matrices would differ"
    return out


def batch_flags(vals):
    """needsComputation() of the three groups, or-ed over the batch (data_augmentation_layer.cu:456-476)."""
    chromatic = bool((vals[:, 6:12] != DEFAULT[6:12]).any())
    eigen = bool((vals[:, 12:34] != DEFAULT[12:34]).any())
    effect = bool(((vals[:, F["fog_amount"]] != 0) & (vals[:, F["fog_size"]] != 0)).any() or (vals[:, F["motion_blur_size"]] > 0).any()
                  or (vals[:, F["shadow_strength"]] > 0).any() or (vals[:, F["noise"]] > 0).any())
    return chromatic, eigen, effect


# ---------------------------------------------------------------------------------------------------------
# launch plans, restated from fn2_data_augmentation_forward / fn2_flow_augmentation_forward
# ---------------------------------------------------------------------------------------------------------
STAT_ROWS_MAX, ITEM_CHUNK, FLOW_CHUNK, RECORD_FLOATS, PARTIAL_OFFSET = 1024, 16, 64, 25, 256


def workspace_bytes():
    return PARTIAL_OFFSET + 4 * 12 * STAT_ROWS_MAX


def stats_plan(N, H, W, aligned16=True):
    hw = H * W
    vec4 = hw % 4 == 0 and aligned16
    per_sample = max(STAT_ROWS_MAX // N, 1)
    work = hw // 4 if vec4 else hw
    bx = min(max(-(-work // 256), 1), per_sample)
    rows = bx * N
    return dict(vec4=vec4, per_sample=per_sample, bx=bx, rows=rows, trips=-(-work // (bx * 256)), capped=-(-work // 256) > per_sample,
                finish_trips=-(-rows // 256))


def mean_depth(plan):
    """Longest chain of dependent roundings behind one mean_rgb: rgb / W / H (2), the trips of one thread (x 4 with 16-byte loads), 6
    shuffle steps, 3 wave sums, ceil(rows / 256) trips and 8 tree steps of eigenspace_finish, the division by N."""
    return 2 + plan["trips"] * (4 if plan["vec4"] else 1) + 6 + 3 + plan["finish_trips"] + 8 + 1


def chunks(N, size):
    return [(n0, min(size, N - n0)) for n0 in range(0, N, size)]


# ---------------------------------------------------------------------------------------------------------
# value +- error
# ---------------------------------------------------------------------------------------------------------
_pow_log = []


class VE:
    __slots__ = ("v", "e")
    __array_ufunc__ = None                    # ndarray * VE goes to VE.__rmul__

    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, np.float64), np.asarray(e, np.float64)

    def __add__(self, o):
        o = lift(o)
        return _rnd(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = lift(o)
        return _rnd(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return lift(o) - self

    def __mul__(self, o):
        o = lift(o)
        return _rnd(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = lift(o)
        with np.errstate(all="ignore"):
            return _rnd(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))


def lift(x):
    return x if isinstance(x, VE) else VE(x)


def _rnd(v, e):
    return VE(v, e + U * np.abs(v))


def vabs(a):
    return VE(np.abs(a.v), a.e)


def vmin(a, b):
    a, b = lift(a), lift(b)
    return VE(np.minimum(a.v, b.v), np.maximum(a.e, b.e))


def vmax(a, b):
    a, b = lift(a), lift(b)
    return VE(np.maximum(a.v, b.v), np.maximum(a.e, b.e))


def vwhere(m, a, b):
    a, b = lift(a), lift(b)
    return VE(np.where(m, a.v, b.v), np.where(m, a.e, b.e))


def vsqrt(a):
    v = np.maximum(a.v, 0)
    r = np.sqrt(v)
    return _rnd(r, np.maximum(np.sqrt(v + a.e) - r, r - np.sqrt(np.maximum(v - a.e, 0))))


def vpow(a, p, live=True):
    """powf(a, p) for a >= 0: the interval ends carry the incoming error, E_POW ulps (1 ulp = 2u relative) on top."""
    p = np.asarray(p, np.float64)
    v = np.maximum(a.v, 0)
    with np.errstate(all="ignore"):
        r = v ** p
        prop = np.maximum(np.abs((v + a.e) ** p - r), np.abs(np.maximum(v - a.e, 0) ** p - r))
    m = np.broadcast_to(live, np.broadcast(v, p).shape) & np.broadcast_to(v > 0, np.broadcast(v, p).shape)
    if m.any():
        _pow_log.append((float(np.broadcast_to(v, m.shape)[m].min()), float(np.broadcast_to(v, m.shape)[m].max()),
                         float(np.broadcast_to(p, m.shape)[m].min()), float(np.broadcast_to(p, m.shape)[m].max())))
    return VE(r, prop + E_POW * 2 * U * np.abs(r))


def vsignpow(a, p, live=True):
    """copysign(powf(|a|, p), a): where the sign of a is not decided the other sign's value is within the error."""
    r = vpow(vabs(a), p, live)
    unsure = np.abs(a.v) <= a.e
    with np.errstate(all="ignore"):
        e = np.where(unsure, (np.abs(a.v) + a.e) ** np.asarray(p, np.float64) * (1 + E_POW * 2 * U) + r.v, r.e)
    return VE(np.copysign(r.v, a.v), e)


def vcos(a):
    return VE(np.cos(a.v), np.abs(np.sin(a.v)) * a.e + E_POW * 2 * U * np.abs(np.cos(a.v)))


def vsin(a):
    return VE(np.sin(a.v), np.abs(np.cos(a.v)) * a.e + E_POW * 2 * U * np.abs(np.sin(a.v)))


def vlog(a):                                                          # exact argument
    return VE(np.log(a.v), E_POW * 2 * U * np.abs(np.log(a.v)))


# ---------------------------------------------------------------------------------------------------------
# DataAugmentation
# ---------------------------------------------------------------------------------------------------------
def positions(mats, ch, cw):
    """(x, y) of M applied to the crop's pixel grid, [N, ch*cw] each, with ep."""
    t = np.asarray(mats, np.float32).astype(np.float64).reshape(-1, 6, 1)
    ys, xs = (g.reshape(1, -1).astype(np.float64) for g in np.mgrid[0:ch, 0:cw])
    px, py = xs * t[:, 0] + ys * t[:, 2] + t[:, 4], xs * t[:, 1] + ys * t[:, 3] + t[:, 5]
    ex = 3 * U * (np.abs(xs * t[:, 0]) + np.abs(ys * t[:, 2]) + np.abs(t[:, 4]))
    ey = 3 * U * (np.abs(xs * t[:, 1]) + np.abs(ys * t[:, 3]) + np.abs(t[:, 5]))
    return px, py, ex, ey, xs, ys


def spatial_statement(img, mats, ch, cw, mut=None):
    """SpatialAugmentation (:24-69) -> VE [N, C, ch*cw], and the number of clamped positions (low, high) per axis."""
    N, C, H, W = img.shape
    flat = img.astype(np.float64).reshape(N, C, H * W)
    px, py, ex, ey, _, _ = positions(mats, ch, cw)
    hx, hy = (float(np.float32(np.float32(s) - np.float32(1.05))) for s in (W, H))
    cx, cy = np.clip(px, 0, hx), np.clip(py, 0, hy)

    def tap(yy, xx):
        idx = (yy * W + xx).astype(np.int64)
        return np.take_along_axis(flat, np.broadcast_to(idx[:, None, :], (N, C, idx.shape[1])), axis=2)

    x0, y0 = np.floor(cx), np.floor(cy)
    fx, fy = (cx - x0)[:, None, :], (cy - y0)[:, None, :]
    tl, tr, bl, br = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    w00, w11, w01, w10 = (1 - fx) * (1 - fy), fx * fy, (1 - fx) * fy, fx * (1 - fy)
    if mut == "swap_w":
        w01, w10 = w10, w01
    value = w00 * tl + w11 * br + w01 * bl + w10 * tr                                                    # :61-64
    rounding = 6 * U * (np.abs(w00 * tl) + np.abs(w11 * br) + np.abs(w01 * bl) + np.abs(w10 * tr))
    lx, ly = np.zeros_like(value), np.zeros_like(value)
    for qx in (np.floor(np.clip(px - ex, 0, hx)), np.floor(np.clip(px + ex, 0, hx))):
        for qy in (np.floor(np.clip(py - ey, 0, hy)), np.floor(np.clip(py + ey, 0, hy))):
            a, b, c, d = tap(qy, qx), tap(qy, qx + 1), tap(qy + 1, qx), tap(qy + 1, qx + 1)
            lx = np.maximum(lx, np.maximum(np.abs(b - a), np.abs(d - c)))
            ly = np.maximum(ly, np.maximum(np.abs(c - a), np.abs(d - b)))
    clamped = dict(x_low=int((px < 0).sum()), x_high=int((px > hx).sum()), y_low=int((py < 0).sum()), y_high=int((py > hy).sum()))
    return VE(value, ex[:, None, :] * lx + ey[:, None, :] * ly + rounding), clamped


def eigen_stats(img, eigvec, d_mean, mut=None):
    """ComputeChromaticEigenspace (:147-187) and the host part (:517-534).  d_mean: roundings behind one mean_rgb."""
    N, C, H, W = img.shape
    x, ev = img.astype(np.float64), np.asarray(eigvec, np.float32).astype(np.float64).reshape(3, 3)
    proj = np.einsum("cj,njhw->nchw", ev, x)
    max_abs = np.abs(proj).max(axis=(0, 2, 3))
    max_abs_e = 3 * U * np.einsum("cj,njhw->nchw", np.abs(ev), np.abs(x)).max(axis=(0, 2, 3))
    mean = x.sum(axis=(0, 2, 3)) / W / H / (N - 1 if mut == "mean_nm1" else N)
    A = np.abs(x).sum(axis=(0, 2, 3)) / W / H / N
    es = dict(max_rgb=np.maximum(img.max(axis=(0, 2, 3)), np.float32(0)), min_rgb=img.min(axis=(0, 2, 3)),       # the kernel starts from 0 / FLT_MAX
              mean_rgb=[VE(mean[c], (d_mean + 2) * U * A[c]) for c in range(3)], max_abs_eig=[VE(max_abs[c], max_abs_e[c]) for c in range(3)], ev=ev)
    for c in range(3):
        assert abs(max_abs[c] - THR) > 100 * max_abs_e[c] + 1e-4, "max_abs_eig at the batch threshold: change the case"
    es["big"] = [bool(max_abs[c] > THR) for c in range(3)]
    es["mean_eig"] = []
    for c in range(3):
        m = ev[c, 0] * es["mean_rgb"][0] + ev[c, 1] * es["mean_rgb"][1] + ev[c, 2] * es["mean_rgb"][2]
        es["mean_eig"].append(m / es["max_abs_eig"][c] if es["big"][c] else m)
    a = es["max_abs_eig"]
    es["max_l"] = vsqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    assert abs(float(es["max_l"].v) - THR) > 100 * float(es["max_l"].e) + 1e-4, "max_l at the batch threshold: change the case"
    es["bigl"] = bool(es["max_l"].v > THR)
    return es


def es_record(es):
    """The EigenSpace record as (values [16], bounds [16]) in the order mean_eig, mean_rgb, max_abs_eig, max_rgb, min_rgb, max_l."""
    ves = es["mean_eig"] + es["mean_rgb"] + es["max_abs_eig"]
    v = [float(a.v) for a in ves] + [float(z) for z in es["max_rgb"]] + [float(z) for z in es["min_rgb"]] + [float(es["max_l"].v)]
    b = ([COLOUR_MARGIN * float(a.e) for a in es["mean_eig"]] + [float(a.e) for a in es["mean_rgb"] + es["max_abs_eig"]] + [0.0] * 6
         + [COLOUR_MARGIN * float(es["max_l"].e)])
    return np.array(v), np.array(b)


def es_from_record(es, rec):
    """The statistics as the device recorded them (25 fp32 values, exact inputs of the pixel chain: error 0), with the branch flags of the
    statement, which are asserted to be decided.  The pixel chain is then held to its own roundings alone, without the worst-case bound
    of the batch statistics on every pixel."""
    rec = np.asarray(rec, np.float32).astype(np.float64)
    return dict(es, mean_eig=[VE(rec[c]) for c in range(3)], mean_rgb=[VE(rec[3 + c]) for c in range(3)],
                max_abs_eig=[VE(rec[6 + c]) for c in range(3)], max_l=VE(rec[15]))


def _eigen_pixel(rgb, k, es, max_multiplier, mut):
    """ChromaticEigenAugmentation (:192-291) on VE arrays [N, P]; k: {field: [N,1] float64}.  Returns rgb and the threshold pixels."""
    ev, big = es["ev"], es["big"]
    d = [rgb[c] - es["mean_rgb"][c] for c in range(3)]                                                   # :209
    eig = []
    for c in range(3):
        e = ev[c, 0] * d[0] + ev[c, 1] * d[1] + ev[c, 2] * d[2]                                          # :214
        if big[c]:
            e = e / es["max_abs_eig"][c]
            e = vsignpow(e, k[f"pow_nomean{c}"])                                                         # :218-231
            e = (e + k[f"add_nomean{c}"]) * k[f"mult_nomean{c}"]
        eig.append(e + es["mean_eig"][c])                                                                # :236-237
    if big[0]:                                                                                           # :240-244
        eig[0] = (vsignpow(eig[0], k["pow_withmean0"]) + k["add_withmean0"]) * k["mult_withmean0"]
    s = vsqrt(eig[1] * eig[1] + eig[2] * eig[2])                                                         # :245
    s_on = s.v > THR
    excluded = np.abs(s.v - THR) <= COLOUR_MARGIN * s.e
    s1 = vwhere(s_on, vmax(vpow(s, k["pow_withmean1"], s_on) + k["add_withmean1"], 0.0) * k["mult_withmean1"], s)   # :247-251
    ang = VE(k["col_angle"])                                                                             # :252-259
    t1 = vcos(ang) * eig[1] - vsin(ang) * eig[2]
    t2 = vsin(ang) * eig[1] + vcos(ang) * eig[2]
    eig[1], eig[2] = vwhere(k["col_angle"] != 0, t1, eig[1]), vwhere(k["col_angle"] != 0, t2, eig[2])
    for c in range(3):
        if big[c]:
            eig[c] = eig[c] * es["max_abs_eig"][c]                                                       # :260-263
    if es["bigl"]:                                                                                       # :264-267
        l1 = vsqrt(eig[0] * eig[0] + eig[1] * eig[1] + eig[2] * eig[2]) / es["max_l"]
    eig[1], eig[2] = vwhere(s_on, eig[1] / s * s1, eig[1]), vwhere(s_on, eig[2] / s * s1, eig[2])        # :268-271
    if es["bigl"]:                                                                                       # :272-284
        l = vsqrt(eig[0] * eig[0] + eig[1] * eig[1] + eig[2] * eig[2])
        l1 = vmax(vpow(l1, k["lmult_pow"]) + k["lmult_add"], 0.0) * k["lmult_mult"] * es["max_l"]
        l_on = l.v > THR
        excluded = excluded | (np.abs(l.v - THR) <= COLOUR_MARGIN * l.e)
        eig = [vwhere(l_on, vmin(eig[c] / l * l1, es["max_abs_eig"][c]), eig[c]) for c in range(3)]
    out = []
    for c in range(3):                                                                                   # :285-290: eigvec TRANSPOSED
        col = ev[c, :] if mut == "eigvec_not_transposed" else ev[:, c]
        v = col[0] * eig[0] + col[1] * eig[1] + col[2] * eig[2]
        out.append(vmax(vmin(v, max_multiplier), 0.0))
    return out, excluded


def _chromatic_pixel(rgb, k, max_multiplier, mut):
    """ColorContrastAugmentation (:72-116)."""
    mean_in, mean_out, scaled = VE(0.0), VE(0.0), []
    for c in range(3):
        mean_in = mean_in + rgb[c]
        scaled.append(rgb[c] * k[f"color{c + 1}"])
        mean_out = mean_out + scaled[c]
    coeff = mean_in / (mean_out if mut == "no_001" else mean_out + float(np.float32(0.01)))              # :97
    out = []
    for c in range(3):
        v = vmax(0.0, vmin(scaled[c] * coeff, 1.0))                                                      # :101
        v = vpow(v, k["gamma"]) + k["brightness"]                                                        # :104-107
        v = 0.5 + (v - 0.5) * k["contrast"]                                                              # :110
        out.append(vmax(0.0, vmin(v, max_multiplier)))                                                   # :113
    return out


def noise_z(N, P, seed, stream):
    """Box-Muller on the words of Philox4x32-10 with counter (pixel, sample * 4 + channel triple, stream) and key = seed: three VE [N, P].
    philox_unit is exact fp32 arithmetic (a conversion, an addition, a product with 2^-32), restated as such."""
    from flownet2_amd.augment import PhiloxStream
    pix = np.broadcast_to(np.arange(P, dtype=np.uint64)[None, :], (N, P))
    smp = np.broadcast_to((np.arange(N, dtype=np.uint64) * np.uint64(4))[:, None], (N, P))
    fill = lambda w: np.full((N, P), w, np.uint64)
    w = PhiloxStream.words(pix, smp, fill(stream & 0xffffffff), fill(stream >> 32), seed & 0xffffffff, seed >> 32)
    u = ((w.astype(np.float32) + np.float32(1.0)) * np.float32(2.3283064365386963e-10)).astype(np.float64)
    two_pi = float(np.float32(6.283185307179586))
    out = []
    for j in (0, 2):
        r = vsqrt(-2.0 * vlog(VE(u[..., j])))
        t = _rnd(two_pi * u[..., j + 1], 0.0)
        out += [r * vcos(t), r * vsin(t)]
    return out[:3]


def data_aug_statement(img, coeffs, mats, ch, cw, mean=None, mean_mode=0, max_multiplier=255.0, eigvec=None, seed=0, stream=0,
                       d_mean=None, mut=None, record=None):
    """-> dict(value, bound [N,C,ch,cw], excluded [N,1,ch,cw], es, flags, clamped, pow_log).  ch = cw = 0: no cropping (the bottom is copied,
    :590, whatever the coefficients say).  mats: [N,6] fp32.  mean_mode as FN2_MEAN_*: 0 none, 1 per channel, 2 per pixel.
    record: the 25 floats of the device's EigenSpace record; the pixel chain then starts from them (es_from_record)."""
    del _pow_log[:]
    img = np.asarray(img, np.float32)
    N, C, H, W = img.shape
    crop = ch > 0 and cw > 0
    res = dict(es=None, flags=(False, False, False), clamped=None)
    if not crop:
        ch, cw = H, W
        px = VE(img.astype(np.float64).reshape(N, C, H * W))
    else:
        px, res["clamped"] = spatial_statement(img, mats, ch, cw, mut)
    P = ch * cw
    excluded = np.zeros((N, P), bool)
    margin = LINEAR_MARGIN
    if crop:
        vals = coeff_values(coeffs if coeffs is not None else np.zeros((N, 42), np.float32))
        chromatic, eigen, effect = res["flags"] = batch_flags(vals)
        k = {name: vals[:, i].astype(np.float64)[:, None] for name, i in F.items()}
        if chromatic or eigen or effect:
            assert C == 3
            margin = COLOUR_MARGIN
            rgb = [VE(px.v[:, c], px.e[:, c]) for c in range(3)]
            if eigen:
                res["es"] = eigen_stats(img, eigvec, d_mean, mut)
                rgb, excluded = _eigen_pixel(rgb, k, res["es"] if record is None else es_from_record(res["es"], record), max_multiplier, mut)
            if chromatic:
                rgb = _chromatic_pixel(rgb, k, max_multiplier, mut)
            if effect:                                                                                   # ApplyEffects, :308-315
                ys, xs = (g.reshape(1, -1).astype(np.float64) for g in np.mgrid[0:ch, 0:cw])
                nx = np.cos(k["shadow_angle"]).astype(np.float32).astype(np.float64)                     # hpp:110: cos in double, stored as float
                ny = np.sin(k["shadow_angle"]).astype(np.float32).astype(np.float64)
                side = (xs - cw // 2) * nx + (ys - ch // 2) * ny - k["shadow_distance"]
                slack = 4 * U * (np.abs((xs - cw // 2) * nx) + np.abs((ys - ch // 2) * ny) + np.abs(k["shadow_distance"]))
                assert np.all((side == 0) | (np.abs(side) > slack)), "shadow edge within rounding of a pixel: change the case"
                on = side >= 0 if mut == "shadow_ge" else side > 0
                rgb = [vmax(0.0, vmin(vwhere(on, v - k["shadow_strength"], v), max_multiplier)) for v in rgb]
                if (k["noise"] > 0).any():                                                               # :578-587
                    z = noise_z(N, P, int(seed), int(stream))
                    rgb = [vwhere(k["noise"] > 0, rgb[c] + k["noise"] * z[c], rgb[c]) for c in range(3)]
            px = VE(np.stack([np.broadcast_to(v.v, (N, P)) for v in rgb], 1), np.stack([np.broadcast_to(v.e, (N, P)) for v in rgb], 1))
    if mean_mode == 1:                                                                                   # :617-634
        px = px - np.asarray(mean, np.float32).astype(np.float64).reshape(1, C, 1)
    elif mean_mode == 2:                                                                                 # :613-616
        m = np.asarray(mean, np.float32).astype(np.float64)
        px = px - (m.reshape(-1)[:C].reshape(1, C, 1) if mut == "mean_pp_as_pc" else m.reshape(1, C, P))
    res.update(value=px.v.reshape(N, C, ch, cw), bound=(margin * np.broadcast_to(px.e, px.v.shape)).reshape(N, C, ch, cw),
               excluded=excluded.reshape(N, 1, ch, cw), pow_log=list(_pow_log))
    return res


def pow_log_in_range(log):
    return all(POW_ARG_RANGE[0] <= lo and hi <= POW_ARG_RANGE[1] and POW_EXP_RANGE[0] <= plo and phi <= POW_EXP_RANGE[1] for lo, hi, plo, phi in log)


# ---------------------------------------------------------------------------------------------------------
# FlowAugmentation
# ---------------------------------------------------------------------------------------------------------
def flow_statement(flow, m1, m2inv, ch, cw, mut=None):
    """WarpData (flow_augmentation_layer.cu:23-88).  m1: [N,6] fp32 matrices of image 1, m2inv: [N,6] inverted matrices of image 2.
    -> (candidates, situations): candidates = up to four (value, bound) [N,2,ch,cw], one per admissible tap; situations counts the taps
    left of / right of / above / below the image and the reads below 0 / at or beyond src_count."""
    flow = np.asarray(flow, np.float32)
    N, _, H, W = flow.shape
    flat, count = flow.astype(np.float64).reshape(-1), flow.size
    px, py, ex, ey, xs, ys = positions(m1, ch, cw)
    t = np.asarray(m2inv, np.float32).astype(np.float64).reshape(N, 6, 1)
    rnd = np.floor if mut == "floor" else np.trunc
    sx, sy = ex + U * (np.abs(px) + 0.5), ey + U * (np.abs(py) + 0.5)                                    # + the rounding of pos + 0.5f
    cols, rows = [rnd(px + 0.5 - sx), rnd(px + 0.5 + sx)], [rnd(py + 0.5 - sy), rnd(py + 0.5 + sy)]
    n = np.arange(N, dtype=np.int64)[:, None]
    cands, seen, situations = [], [], None
    for row in rows:
        for col in cols:
            if any(np.array_equal(row, r) and np.array_equal(col, c) for r, c in seen):
                continue
            seen.append((row, col))
            off = row.astype(np.int64) * W + col.astype(np.int64)                                        # :45-50: flat, no clamp per axis
            idx = [W * H * (2 * n + j) + off for j in (0, 1)]
            uv = []
            for i in idx:
                inside = (i >= 0) & (i < count)
                g = flat[np.clip(i, 0, count - 1)]
                uv.append(g if mut == "clamped_index" else np.where(inside, g, 0.0))
            if situations is None:
                situations = dict(left=int((col < 0).sum()), right=int((col >= W).sum()), above=int((row < 0).sum()), below=int((row >= H).sum()),
                                  before_first=int((idx[0] < 0).sum() + (idx[1] < 0).sum()), past_last=int((idx[0] >= count).sum() + (idx[1] >= count).sum()))
            x2, y2 = VE(px, ex) + uv[0], VE(py, ey) + uv[1]                                              # :52-53
            x3 = x2 * t[:, 0] + y2 * t[:, 2] + t[:, 4]                                                   # :56-57
            y3 = x2 * t[:, 1] + y2 * t[:, 3] + t[:, 5]
            ox, oy = x3 - xs, y3 - ys                                                                    # :60-61
            cands.append((np.stack([ox.v, oy.v], 1).reshape(N, 2, ch, cw), LINEAR_MARGIN * np.stack([ox.e, oy.e], 1).reshape(N, 2, ch, cw)))
    return cands, situations


def flow_ratio(got, cands):
    """Per pixel the best candidate's worst error / bound over the two channels: <= 1 everywhere is a pass."""
    got = np.asarray(got, np.float64)
    best = None
    for value, bound in cands:
        r = (np.abs(got - value) / np.maximum(bound, 1e-300)).max(axis=1)
        best = r if best is None else np.minimum(best, r)
    return best
