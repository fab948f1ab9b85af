"""Unsupervised-loss references for the tests: the arithmetic of include/flownet2_hip_unsup_loss.h, written once (evaluate) and run twice.

ref32: on NumPy float32 arrays -- every array is float32 and every scalar an np.float32, so a + b, a * b, a / b and np.sqrt (correctly
rounded) are the kernel's operations (compiled without contraction) in the kernel's association; the fp64 sums are added in the kernel's
order (ordered_sum: thread, wave64 tree, four waves, chunks, samples).  With gamma == 0.5 and edge_weight == 0 (no powf, no expf) the
kernel must equal it bit for bit: rows, loss and gradients.

ref64: on `Bnd` arrays -- a float64 value v together with a bound e on |what the fp32 kernel computes - v| (a running error analysis).
Every branch decision (finite, occluded, inside, the tap indices, which terms exist) is taken from the float32 values (decide), as the
other *_ref.py files do, so both evaluations give the same pixels a term.  The bound, with U = 2^-24, operation by operation:
  a + b, a - b      e = e_a + e_b, then one rounding: + U (|v| + e)
  a * b             e = |a| e_b + |b| e_a + e_a e_b, then one rounding
  a / b             e = (e_a + |v| e_b) / (|b| - e_b), then one rounding (fp32 division is correctly rounded)
  sqrt(a)           e = min(e_a / sqrt(a), sqrt(e_a)), then one rounding
  powf(a, g)        e = |g| max(lo^(g-1), hi^(g-1)) e_a with [lo, hi] = a -+ e_a (the derivative is monotone), then E_POW ulps (2 U E_POW
                    relative): the allowance of tests/lpq_ref.py, measured there for the device's powf with a margin of 2; where the
                    kernel's exponent is a rounded float32 (gamma - 1.0f), a^g (exp(|ln a| |dg|) - 1) for its distance dg from g
  expf(a)           e = exp(a) (exp(e_a) - 1), then the same E_POW ulps (the ROCm math documentation is not installed next to the
                    toolchain, so no other figure is at hand)
  |a|, -a, select   e unchanged
  fp64 sum of n     sum of the e, + n 2^-53 sum |v|
and a few multiples of the smallest subnormal (TINY) per rounding cover underflow.  Inputs are float32 and exact.  No file of the
reference tree is read, and no tolerance here comes from the kernel's output."""
import ctypes as C

import numpy as np

from flownet2_amd import _lib
from flownet2_amd.evaluate import UNSUP_LOSS_COL as COL, UNSUP_LOSS_K as K
from lpq_ref import E_POW

U = 2.0 ** -24
TINY = 16 * 2.0 ** -149
OK, INVALID, WORKSPACE = 0, -1, -3
F = np.float32
LIMIT = F(1e9)
COUNT_COLUMNS = [COL[n] for n in ("PIXELS", "COUNTED", "OCCLUDED", "OUTSIDE", "NONFINITE", "SMOOTH_TERMS")]
SUM_COLUMNS = [COL["DATA_SUM"], COL["SMOOTH_SUM"]]
DEFAULTS = dict(data_weight=1.0, smooth_weight=1.0, charbonnier=(1e-3, 0.45), smooth_charbonnier=(1e-3, 0.45), edge_weight=10.0,
                smooth_order=2, flow_mult=1.0)
EXACT = dict(charbonnier=(1e-3, 0.5), smooth_charbonnier=(1e-3, 0.5), edge_weight=0.0)        # no powf, no expf: bit for bit


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- the two number types -----------------------------------------------------------------------------------------------------------
class Bnd:
    """float64 values v with bounds e on |fp32-computed - v| (module docstring)."""
    __array_priority__ = 1000
    __array_ufunc__ = None

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Bnd) else Bnd(np.asarray(x, np.float64))

    @staticmethod
    def rounded(v, e, ulps=0.5):
        return Bnd(v, e + 2 * ulps * U * (np.abs(v) + e) + TINY)

    def __add__(self, o):
        o = Bnd.lift(o)
        return Bnd.rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = Bnd.lift(o)
        return Bnd.rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Bnd.lift(o) - self

    def __mul__(self, o):
        o = Bnd.lift(o)
        return Bnd.rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Bnd.lift(o)
        lo = np.abs(o.v) - o.e
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            e = np.where(lo > 0, (self.e + np.abs(v) * o.e) / np.where(lo > 0, lo, 1.0), np.inf)
        return Bnd.rounded(v, e)

    def __rtruediv__(self, o):
        return Bnd.lift(o) / self

    def __neg__(self):
        return Bnd(-self.v, self.e)

    def __getitem__(self, i):
        return Bnd(self.v[i], self.e[i])


def _sqrt(a):
    if not isinstance(a, Bnd):
        return np.sqrt(a)
    v = np.sqrt(a.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.minimum(np.where(a.v > 0, a.e / np.where(a.v > 0, v, 1.0), np.inf), np.sqrt(a.e))
    return Bnd.rounded(v, e)


def _pow(a, g, g_err=0.0):
    """a ** g for a >= 0.  float32: g is the kernel's float32 exponent.  Bnd: g is the exponent of the exact function and g_err the
    distance of the kernel's float32 exponent from it."""
    if not isinstance(a, Bnd):
        return np.power(a, F(g)).astype(F)
    lo, hi = np.maximum(a.v - a.e, 0.0), a.v + a.e
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = np.power(a.v, g)
        slope = abs(g) * np.maximum(np.power(lo, g - 1.0), np.power(hi, g - 1.0))
        e = np.where(a.e > 0, slope * a.e, 0.0)
        if g_err:
            e = e + np.where(a.v > 0, v * np.expm1(np.abs(np.log(np.where(a.v > 0, a.v, 1.0))) * g_err), 0.0)
    return Bnd.rounded(v, e, ulps=E_POW)


def _exp(a):
    if not isinstance(a, Bnd):
        return np.exp(a).astype(F)
    v = np.exp(a.v)
    return Bnd.rounded(v, v * np.expm1(a.e), ulps=E_POW)


def _abs(a):
    return Bnd(np.abs(a.v), a.e) if isinstance(a, Bnd) else np.abs(a)


def _where(m, a, b):
    if isinstance(a, Bnd) or isinstance(b, Bnd):
        a, b = Bnd.lift(a), Bnd.lift(b)
        return Bnd(np.where(m, a.v, b.v), np.where(m, a.e, b.e))
    return np.where(m, a, b)


def _shift(h, axis, k):
    """out[i] = h[i - k] along `axis` (k = +1: the value of the previous pixel), zero where there is none."""
    if isinstance(h, Bnd):
        return Bnd(_shift(h.v, axis, k), _shift(h.e, axis, k))
    out = np.zeros_like(h)
    src = [slice(None)] * h.ndim
    dst = [slice(None)] * h.ndim
    n = h.shape[axis]
    if abs(k) < n:
        src[axis] = slice(0, n - k) if k > 0 else slice(-k, n)
        dst[axis] = slice(k, n) if k > 0 else slice(0, n + k)
        out[tuple(dst)] = h[tuple(src)]
    return out


def _ok(t):
    with np.errstate(invalid="ignore"):
        return np.abs(t) <= LIMIT                                                   # False for NaN and +-Inf


def _gather(o, c, iy, ix):
    return o[np.arange(o.shape[0])[:, None, None], c, iy, ix]


# ---- the decisions, in float32 --------------------------------------------------------------------------------------------------------
def decide(Ia, Io, a, occ, p):
    """What both evaluations share, decided in float32: cls [N,H,W] (0 counted, 1 occluded, 2 outside, 3 non-finite), the tap indices
    (0 where the pixel did not reach step 4), and per axis the mask of the smoothness terms that exist and are not dropped."""
    N, Cc, H, W = Ia.shape
    mult, order, edge = F(p["flow_mult"]), int(p["smooth_order"]), F(p["edge_weight"])
    with np.errstate(invalid="ignore", over="ignore"):
        au, av = mult * a[:, 0], mult * a[:, 1]
        fin = _ok(au) & _ok(av)
        occl = fin & ~(occ[:, 0] == 0) if occ is not None else np.zeros_like(fin)
        x2 = np.arange(W, dtype=F)[None, None, :] + au
        y2 = np.arange(H, dtype=F)[None, :, None] + av
        inside = (x2 >= 0) & (y2 >= 0) & (x2 < F(W)) & (y2 < F(H))
    cand = fin & ~occl & inside
    x2, y2 = np.where(cand, x2, F(0)), np.where(cand, y2, F(0))
    ixL, iyT = x2.astype(np.int32), y2.astype(np.int32)
    ixR, iyB = np.minimum(ixL + 1, W - 1), np.minimum(iyT + 1, H - 1)
    assert ixL.min() >= 0 and ixR.max() <= W - 1 and iyT.min() >= 0 and iyB.max() <= H - 1
    tapfin = np.ones_like(fin)
    for c in range(Cc):
        tapfin &= _ok(Ia[:, c])
        for iy, ix in ((iyT, ixL), (iyT, ixR), (iyB, ixL), (iyB, ixR)):
            tapfin &= _ok(_gather(Io, c, iy, ix))
    cls = np.where(~fin, 3, np.where(occl, 1, np.where(~inside, 2, np.where(tapfin, 0, 3)))).astype(np.int32)
    img_ok = np.logical_and.reduce([_ok(Ia[:, c]) for c in range(Cc)])
    terms = []
    for axis in (2, 1):                                                             # x (the last axis of [N,H,W]), then y
        n = fin.shape[axis]
        idx = np.arange(n)
        exists = (idx + 1 < n) & ((idx - 1 >= 0) if order == 2 else True)
        exists = exists[None, None, :] if axis == 2 else exists[None, :, None]
        t = exists & fin & _shift(fin, axis, -1)
        if order == 2:
            t = t & _shift(fin, axis, 1)
        if edge != 0:
            t = t & _shift(img_ok, axis, -1) & (_shift(img_ok, axis, 1) if order == 2 else img_ok)
        terms.append(t)
    return dict(cls=cls, taps=(ixL, ixR, iyT, iyB), terms=terms)


# ---- the arithmetic, once ---------------------------------------------------------------------------------------------------------
def _psi(t, eps, gam):
    r = t * t + eps * eps
    return _sqrt(r) if gam == F(0.5) else _pow(r, float(gam))


def _dpsi(t, eps, gam):
    r = t * t + eps * eps
    if gam == F(0.5):
        return t / _sqrt(r)
    c = F(2) * gam                                                                  # exact
    if isinstance(t, Bnd):                                                          # the exact exponent gamma - 1; the kernel's is its float32 rounding
        return (t * float(c)) * _pow(r, float(gam) - 1.0, abs(float(gam - F(1)) - (float(gam) - 1.0)))
    return (t * c) * _pow(r, float(gam - F(1)))


def evaluate(Ia, Io, a, dec, p, bounded):
    """One direction: the per-pixel data term e, the smoothness terms (tx, ty) and the pieces of the gradient (Su, Sv and G_u, G_v), as
    float32 arrays (bounded False) or as Bnd (True)."""
    N, Cc, H, W = Ia.shape
    if bounded:
        clean = lambda t: np.where(np.isfinite(t) & _ok(t), t, 0).astype(np.float64)
        num = lambda t: Bnd(clean(t))
        const = lambda s: Bnd(float(F(s)))
    else:
        num = lambda t: np.ascontiguousarray(t, F)
        const = F
    one, two = const(1), const(2)
    eps_d, gam_d = const(p["charbonnier"][0]), F(p["charbonnier"][1])
    eps_s, gam_s = const(p["smooth_charbonnier"][0]), F(p["smooth_charbonnier"][1])
    edge, order, mult = F(p["edge_weight"]), int(p["smooth_order"]), const(p["flow_mult"])
    ixL, ixR, iyT, iyB = dec["taps"]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        au, av = mult * num(a[:, 0]), mult * num(a[:, 1])
        xs, ys = np.arange(W, dtype=F)[None, None, :], np.arange(H, dtype=F)[None, :, None]
        x2, y2 = (xs + au, ys + av) if not bounded else (au + xs.astype(np.float64), av + ys.astype(np.float64))
        fl = (lambda i: i.astype(F)) if not bounded else (lambda i: i.astype(np.float64))
        al, be = x2 - fl(ixL), y2 - fl(iyT)
        cTL, cTR, cBL, cBR = (one - al) * (one - be), al * (one - be), (one - al) * be, al * be
        gy, gx = fl(iyB) - y2, fl(ixR) - x2
        zero = num(np.zeros((N, H, W), F))
        e, Su, Sv = zero, zero, zero
        for c in range(Cc):
            TL, TR, BL, BR = (num(_gather(Io, c, iy, ix)) for iy, ix in ((iyT, ixL), (iyT, ixR), (iyB, ixL), (iyB, ixR)))
            warped = ((cTL * TL + cTR * TR) + cBL * BL) + cBR * BR
            d = num(Ia[:, c]) - warped
            e = e + _psi(d, eps_d, gam_d)
            dp = _dpsi(d, eps_d, gam_d)
            tu = gy * (TR - TL) + (one - gy) * (BR - BL)
            tv = gx * (BL - TL) + (one - gx) * (BR - TR)
            Su, Sv = Su + dp * tu, Sv + dp * tv
        counted = dec["cls"] == 0
        out = dict(e=_where(counted, e, zero), Su=_where(counted, Su, zero), Sv=_where(counted, Sv, zero), terms=[], G=[])
        G = [None, None]
        for k, axis in enumerate((2, 1)):
            valid = dec["terms"][k]
            s = []
            for f in (au, av):
                fp = _shift(f, axis, -1)
                s.append((_shift(f, axis, 1) - two * f) + fp if order == 2 else fp - f)
            term = _psi(s[0], eps_s, gam_s) + _psi(s[1], eps_s, gam_s)
            h = [_dpsi(s[0], eps_s, gam_s), _dpsi(s[1], eps_s, gam_s)]
            if edge != 0:
                g = zero
                for c in range(Cc):
                    I = num(Ia[:, c])
                    g = g + _abs(_shift(I, axis, -1) - (_shift(I, axis, 1) if order == 2 else I))
                m = g / const(Cc)
                wgt = _exp(m * const(-edge)) if bounded else _exp(F(-edge) * m)
                term, h = wgt * term, [wgt * h[0], wgt * h[1]]
            out["terms"].append(_where(valid, term, zero))
            for j in (0, 1):
                hj = _where(valid, h[j], zero)
                Gj = (_shift(hj, axis, 1) - two * hj) + _shift(hj, axis, -1) if order == 2 else _shift(hj, axis, 1) - hj
                G[j] = Gj if G[j] is None else G[j] + Gj
        out["G"] = G
    return out


# ---- the sums -------------------------------------------------------------------------------------------------------------------------
def chunks(hw):
    return min(max((hw + 1023) // 1024, 1), 128)


def ordered_sum(vals, H, W):
    """The kernel's fp64 sum over one sample of vals [J, H, W] (float32 values; per pixel vals[0] is added first): a thread's pixels in
    ascending order, the wave64 shuffle tree, the four waves in order, the chunks in index order."""
    J = len(vals)
    hw, V, B = H * W, (4 if W % 4 == 0 else 1), chunks(H * W)
    steps = -(-(hw // V) // (B * 256))
    padded = np.zeros((J, steps * B * 256 * V), np.float64)
    padded[:, :hw] = np.asarray(vals, np.float64).reshape(J, hw)
    arr = padded.reshape(J, steps, B, 256, V)
    acc = np.zeros((B, 256), np.float64)
    for s in range(steps):
        for k in range(V):
            for j in range(J):
                acc = acc + arr[j, s, :, :, k]
    w = acc.reshape(B, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[..., :off] + w[..., off:2 * off]
    w = w[..., 0]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    tot = 0.0
    for b in range(B):
        tot = tot + float(part[b])
    return tot


def _count_rows(dec, N):
    rows = np.zeros((N + 1, K), np.float64)
    cls = dec["cls"].reshape(N, -1)
    rows[:N, COL["PIXELS"]] = cls.shape[1]
    for name, v in (("COUNTED", 0), ("OCCLUDED", 1), ("OUTSIDE", 2), ("NONFINITE", 3)):
        rows[:N, COL[name]] = (cls == v).sum(1)
    rows[:N, COL["SMOOTH_TERMS"]] = dec["terms"][0].reshape(N, -1).sum(1) + dec["terms"][1].reshape(N, -1).sum(1)
    return rows


def _directions(img0, img1, fw, bw, occ_fw, occ_bw):
    dirs = [(img0, img1, fw, occ_fw)]
    if bw is not None:
        dirs.append((img1, img0, bw, occ_bw))
    return [tuple(None if t is None else np.ascontiguousarray(t, F) for t in d) for d in dirs]


def ref32(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, p=None, total_diff=1.0):
    """dict(rows [2, N + 1, K] float64, loss float32, diff [per direction [N,2,H,W] float32]) -- what the kernels must equal bit for bit
    where p has gamma == 0.5 and edge_weight == 0."""
    p = p or params()
    N, Cc, H, W = img0.shape
    rows, diffs, L = np.zeros((2, N + 1, K), np.float64), [], 0.0
    dw, sw = float(F(p["data_weight"])), float(F(p["smooth_weight"]))
    for d, (Ia, Io, a, occ) in enumerate(_directions(img0, img1, fw, bw, occ_fw, occ_bw)):
        dec = decide(Ia, Io, a, occ, p)
        ev = evaluate(Ia, Io, a, dec, p, bounded=False)
        assert all(t.dtype == F for t in (ev["e"], ev["Su"], ev["Sv"], *ev["terms"], *ev["G"]))
        r = _count_rows(dec, N)
        for n in range(N):
            r[n, COL["DATA_SUM"]] = ordered_sum([ev["e"][n]], H, W)
            r[n, COL["SMOOTH_SUM"]] = ordered_sum([ev["terms"][0][n], ev["terms"][1][n]], H, W)
        for k in range(K):
            tot = 0.0
            for n in range(N):
                tot = tot + float(r[n, k])
            r[N, k] = tot
        rows[d] = r
        t = r[N]
        L = L + ((dw * t[COL["DATA_SUM"]]) / max(t[COL["COUNTED"]], 1.0) + (sw * t[COL["SMOOTH_SUM"]]) / max(t[COL["SMOOTH_TERMS"]], 1.0))
        kd = F(total_diff) * F(dw / max(t[COL["COUNTED"]], 1.0))
        ks = F(total_diff) * F(sw / max(t[COL["SMOOTH_TERMS"]], 1.0))
        mult = F(p["flow_mult"])
        counted = dec["cls"] == 0
        with np.errstate(invalid="ignore", over="ignore"):
            diff = np.stack([mult * (np.where(counted, (-kd) * S, F(0)) + ks * G) for S, G in ((ev["Su"], ev["G"][0]), (ev["Sv"], ev["G"][1]))], 1)
        assert diff.dtype == F
        diffs.append(diff)
    return dict(rows=rows, loss=F(L), diff=diffs)


def ref64(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, p=None, total_diff=1.0):
    """The float64 evaluation with its bounds: dict(rows, rows_bound [2, N + 1, K], loss, loss_bound, diff, diff_bound [per direction])."""
    p = p or params()
    N, Cc, H, W = img0.shape
    rows, rbound, diffs, dbounds = np.zeros((2, N + 1, K)), np.zeros((2, N + 1, K)), [], []
    dw, sw = float(F(p["data_weight"])), float(F(p["smooth_weight"]))
    L, Lb = 0.0, 0.0
    for d, (Ia, Io, a, occ) in enumerate(_directions(img0, img1, fw, bw, occ_fw, occ_bw)):
        dec = decide(Ia, Io, a, occ, p)
        ev = evaluate(Ia, Io, a, dec, p, bounded=True)
        r, rb = _count_rows(dec, N), np.zeros((N + 1, K))
        for col, parts in ((COL["DATA_SUM"], [ev["e"]]), (COL["SMOOTH_SUM"], ev["terms"])):
            v = sum(t.v.reshape(N, -1).sum(1) for t in parts)
            b = sum(t.e.reshape(N, -1).sum(1) for t in parts)
            r[:N, col], rb[:N, col] = v, b + len(parts) * H * W * 2.0 ** -53 * v
        r[N] = r[:N].sum(0)
        rb[N] = rb[:N].sum(0) + N * 2.0 ** -53 * r[N]
        rb[:, COUNT_COLUMNS] = 0
        rows[d], rbound[d] = r, rb
        t, tb = r[N], rb[N]
        cd, cs = max(t[COL["COUNTED"]], 1.0), max(t[COL["SMOOTH_TERMS"]], 1.0)
        L += dw * t[COL["DATA_SUM"]] / cd + sw * t[COL["SMOOTH_SUM"]] / cs
        Lb += dw * tb[COL["DATA_SUM"]] / cd + sw * tb[COL["SMOOTH_SUM"]] / cs
        g = float(F(total_diff))
        kd, ks = Bnd.rounded(dw / cd, 0.0) * g, Bnd.rounded(sw / cs, 0.0) * g
        mult = float(F(p["flow_mult"]))
        dd = [(((-kd) * S) + ks * G) * mult for S, G in ((ev["Su"], ev["G"][0]), (ev["Sv"], ev["G"][1]))]
        diffs.append(np.stack([t.v for t in dd], 1))
        dbounds.append(np.stack([t.e for t in dd], 1))
    return dict(rows=rows, rows_bound=rbound, loss=L, loss_bound=Lb + 2 * U * abs(L) + TINY, diff=diffs, diff_bound=dbounds)


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------
def make_images(shape, seed, shift=1.5):
    """(img0, img1) float32 [N,C,H,W] in about [0, 1]: sums of a few low-frequency sinusoids, img1 the same pattern moved by `shift`
    pixels along x and half of that along y."""
    N, Cc, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((2,) + tuple(shape), np.float64)
    for n in range(N):
        for c in range(Cc):
            for _ in range(3):
                amp, fx, fy, ph = rng.uniform(0.05, 0.17), rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.5), rng.uniform(0, 6.28)
                for k, s in enumerate((0.0, shift)):
                    out[k, n, c] += amp * np.sin(fx * (x - s) + fy * (y - 0.5 * s) + ph)
    return (out[0] + 0.5).astype(F), (out[1] + 0.5).astype(F)


def make_flows(shape, seed, kind):
    """(fw, bw) float32 [N,2,H,W]: "small" smooth flows of a pixel or two, "large" ones with many targets outside."""
    N, _, H, W = shape
    rng = np.random.default_rng(seed + 1000)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    amp = {"small": 1.5, "large": 0.6 * max(H, W) + 2.0}[kind]
    fw = np.zeros((N, 2, H, W), np.float64)
    for n in range(N):
        for c in range(2):
            fx, fy, ph = rng.uniform(0.02, 0.3), rng.uniform(0.02, 0.3), rng.uniform(0, 6.28, 2)
            fw[n, c] = amp * np.sin(fx * x + ph[0]) * np.cos(fy * y + ph[1]) + rng.uniform(-0.5, 0.5)
    bw = -fw + rng.normal(0, 0.05, fw.shape)
    return fw.astype(F), bw.astype(F)


def make_occ(shape, seed):
    """(occ_fw, occ_bw) float32 [N,1,H,W] of 0 / 1, about a fifth set."""
    N, _, H, W = shape
    rng = np.random.default_rng(seed + 2000)
    return tuple((rng.random((N, 1, H, W)) < 0.2).astype(F) for _ in range(2))


def poison(arrays, seed):
    """NaN, +-Inf and +-1e10 written into a few places of each array, in place (flows, images, occ)."""
    rng = np.random.default_rng(seed + 3000)
    bad = [np.nan, np.inf, -np.inf, 1e10, -1e10]
    for t in arrays:
        flat = t.reshape(-1)
        for k, pos in enumerate(rng.permutation(flat.size)[:min(flat.size // 8 + 1, 6)]):
            flat[pos] = bad[k % len(bad)]


# ---- the raw C ABI --------------------------------------------------------------------------------------------------------------------
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
    assert _lib.lib().fn2_unsup_loss_sizes(int(N), int(H), int(W), C.byref(nbytes), C.byref(k)) == OK
    return nbytes.value, k.value


def scalars(p):
    (ed, gd), (es, gs) = p["charbonnier"], p["smooth_charbonnier"]
    return (f(p["data_weight"]), f(p["smooth_weight"]), f(ed), f(gd), f(es), f(gs), f(p["edge_weight"]), int(p["smooth_order"]), f(p["flow_mult"]))


def forward(img0, img1, fw, bw, occ_fw, occ_bw, shape, p, results, loss, ws, ws_bytes, stream=None):
    N, Cc, H, W = shape
    return _lib.lib().fn2_unsup_loss_forward(ptr(img0), ptr(img1), ptr(fw), ptr(bw), ptr(occ_fw), ptr(occ_bw), int(N), int(Cc), int(H), int(W),
                                             *scalars(p), ptr(results), ptr(loss), ptr(ws), int(ws_bytes), stream)


def backward(img0, img1, fw, bw, occ_fw, occ_bw, shape, p, results, total_diff, fw_diff, bw_diff, stream=None):
    N, Cc, H, W = shape
    return _lib.lib().fn2_unsup_loss_backward(ptr(img0), ptr(img1), ptr(fw), ptr(bw), ptr(occ_fw), ptr(occ_bw), int(N), int(Cc), int(H), int(W),
                                              *scalars(p), ptr(results), ptr(total_diff), ptr(fw_diff), ptr(bw_diff), stream)
