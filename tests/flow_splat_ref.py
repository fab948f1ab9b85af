"""Forward-warping (splatting) references for the tests: the arithmetic of include/flownet2_hip_flow_splat.h, written once (over a small
number-type interface) and run twice.

T32: NumPy float32 arrays -- a + b, a * b, a / b are the kernel's operations, one rounding each, in the kernel's association; the one
fused operation of the header, num = fmaf(value, ws, num), is fma32 (exact product and sum in float64, rounded to odd, then to float32:
one rounding).  The sum at a cell runs over its sources in ascending source index.  Where no expf is evaluated away from 0 (sum, average,
linear, softmax with metric == 0) the kernel must equal it bit for bit: planes, statuses, counts and the three gradients.

T64: `Bnd` arrays of tests/unsup_loss_ref.py -- a float64 value with a running bound on |what the fp32 kernel computes - value| (the
rules are listed there; expf carries E_POW = 2 x 1.32 ulps, the fmaf is bounded as a product and a sum).  Every decision
(status, tap indices, which taps share a cell, which tap has weight 0, den > 0) is taken from the float32 evaluation, so both give the
same sources a term.

No file of the reference tree is read, and no tolerance here comes from the kernel's output."""
import numpy as np

from flownet2_amd.evaluate import FLOW_SPLAT_COL as COL, FLOW_SPLAT_K as K, FLOW_SPLAT_STATUS as STATUS
from unsup_loss_ref import Bnd, _exp, _where

F = np.float32
LIMIT = F(1e9)
NONE, LINEAR, SOFTMAX = 0, 1, 2
IMPORTANCE = {"none": NONE, "linear": LINEAR, "softmax": SOFTMAX}
MASKED, NONFINITE, OUTSIDE, SPLATTED = (STATUS[n] for n in ("MASKED", "NONFINITE", "OUTSIDE", "SPLATTED"))
FILL_NAN_BITS = 0xFFE00000                      # FlowWarp's NaN
OK, INVALID, WORKSPACE = 0, -1, -3


def fma32(a, b, c):
    """fmaf on float32 arrays: a * b is exact in float64; the float64 sum is rounded to odd (TwoSum gives the sign of what was lost), so
    the rounding to float32 that follows is the only one."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


class T32:
    name = "float32"
    lift = staticmethod(lambda x: np.asarray(x, F))
    zeros = staticmethod(lambda shape: np.zeros(shape, F))
    where = staticmethod(np.where)
    cat = staticmethod(lambda parts: np.concatenate(parts))
    fma = staticmethod(fma32)
    exp = staticmethod(lambda a: np.exp(a).astype(F))
    neg = staticmethod(lambda a: -a)

    @staticmethod
    def put(a, idx, val):
        a = a.copy()
        a[idx] = val
        return a


class T64:
    name = "float64 with bound"
    lift = staticmethod(lambda x: x if isinstance(x, Bnd) else Bnd(np.asarray(x, np.float64)))
    zeros = staticmethod(lambda shape: Bnd(np.zeros(shape), np.zeros(shape)))
    where = staticmethod(_where)
    cat = staticmethod(lambda parts: Bnd(np.concatenate([p.v for p in parts]), np.concatenate([np.broadcast_to(p.e, p.v.shape) for p in parts])))
    fma = staticmethod(lambda a, b, c: a * b + c)
    exp = staticmethod(_exp)
    neg = staticmethod(lambda a: -a)

    @staticmethod
    def put(a, idx, val):
        v, e = a.v.copy(), np.array(a.e)
        v[idx] = np.broadcast_to(val.v, v[idx].shape)
        e[idx] = np.broadcast_to(val.e, e[idx].shape)
        return Bnd(v, e)


class Decision:
    """Steps 1 - 6 of the header for one sample, on float32: status [HW], and for the SPLATTED sources S (ascending) the corners."""

    def __init__(self, flow, metric, valid, t, imp):
        _, H, W = flow.shape
        self.H, self.W = H, W
        ys, xs = np.mgrid[0:H, 0:W]
        self.xs, self.ys = xs.reshape(-1).astype(F), ys.reshape(-1).astype(F)
        u, v = flow[0].reshape(-1), flow[1].reshape(-1)
        t = F(t)
        with np.errstate(all="ignore"):
            okf = (np.abs(u) <= LIMIT) & (np.abs(v) <= LIMIT)
            okz = np.ones(H * W, bool)
            if imp != NONE:
                z = metric.reshape(-1)
                okz = np.abs(z) <= LIMIT
                if imp == LINEAR:
                    okz &= ~(z < 0)
                else:
                    okz &= ~np.isinf(np.exp(np.where(okz, z, F(0))).astype(F))
            x2, y2 = self.xs + t * u, self.ys + t * v
            inside = (x2 >= 0) & (y2 >= 0) & (x2 < F(W)) & (y2 < F(H))
        masked = np.zeros(H * W, bool) if valid is None else valid.reshape(-1) == 0
        self.status = np.where(masked, MASKED, np.where(~okf | ~okz, NONFINITE, np.where(~inside, OUTSIDE, SPLATTED))).astype(np.uint8)
        self.S = np.nonzero(self.status == SPLATTED)[0]
        x2, y2 = x2[self.S], y2[self.S]
        self.ixL, self.iyT = np.minimum(x2.astype(np.int64), W - 1), np.minimum(y2.astype(np.int64), H - 1)
        ixR, iyB = np.minimum(self.ixL + 1, W - 1), np.minimum(self.iyT + 1, H - 1)
        self.o = np.stack([self.iyT * W + self.ixL, self.iyT * W + ixR, iyB * W + self.ixL, iyB * W + ixR])      # TL, TR, BL, BR


def _source_values(T, d, flow, metric, t, imp):
    """al, be, the four weights and e of the SPLATTED sources, in the number type T."""
    S = d.S
    u, v = T.lift(flow[0].reshape(-1)[S]), T.lift(flow[1].reshape(-1)[S])
    t = T.lift(F(t))
    x2, y2 = T.lift(d.xs[S]) + t * u, T.lift(d.ys[S]) + t * v
    al, be = x2 - T.lift(d.ixL.astype(F)), y2 - T.lift(d.iyT.astype(F))
    one = T.lift(F(1))
    w = [(one - al) * (one - be), al * (one - be), (one - al) * be, al * be]
    e = None
    if imp == LINEAR:
        e = T.lift(metric.reshape(-1)[S])
    elif imp == SOFTMAX:
        e = T.exp(T.lift(metric.reshape(-1)[S]))
    return al, be, w, e


def _sample_forward(T, d, values, flow, metric, t, imp, w32=None):
    """num [C,HW], den [HW] of one sample; w32: the float32 weights (the zero-weight decision), None when T is T32."""
    C_ = values.shape[0]
    HW = d.H * d.W
    al, be, w, e = _source_values(T, d, flow, metric, t, imp)
    wdec = w if w32 is None else w32
    vals = T.lift(values.reshape(C_, HW))
    cells, srcs, wss, zts = [], [], [], []
    for k in range(4):
        first = np.ones(d.S.size, bool)
        for j in range(k):
            first &= d.o[j] != d.o[k]
        wsum = T.zeros(d.S.size)
        hits, zero = np.zeros(d.S.size, np.int64), np.zeros(d.S.size, bool)
        for j in range(4):
            same = d.o[j] == d.o[k]
            wsum = T.where(same, wsum + w[j], wsum)
            hits += same
            zero |= same & (wdec[j] == 0)
        ws = wsum if imp == NONE else wsum * e
        cells.append(d.o[k][first]); srcs.append(d.S[first]); wss.append(ws[first]); zts.append(((hits > 1) & zero)[first])
    cell, src, ws, zt = np.concatenate(cells), np.concatenate(srcs), T.cat(wss), np.concatenate(zts)
    order = np.lexsort((src, cell))
    cell, src, ws, zt = cell[order], src[order], ws[order], zt[order]
    start = np.r_[True, cell[1:] != cell[:-1]] if cell.size else np.zeros(0, bool)
    rank = np.arange(cell.size) - np.maximum.accumulate(np.where(start, np.arange(cell.size), 0)) if cell.size else np.zeros(0, np.int64)
    num, den = T.zeros((C_, HW)), T.zeros(HW)
    zero_f = T.lift(F(0))
    with np.errstate(all="ignore"):
        for r in range(int(rank.max()) + 1 if rank.size else 0):
            sel = np.nonzero(rank == r)[0]
            c, s = cell[sel], src[sel]
            num = T.put(num, (slice(None), c), T.fma(vals[:, s], ws[sel], num[:, c]))
            z = sel[zt[sel]]
            if z.size:
                num = T.put(num, (slice(None), cell[z]), T.fma(vals[:, src[z]], zero_f, num[:, cell[z]]))
            den = T.put(den, c, den[c] + ws[sel])
    return num, den, (al, be, w, e)


def _raw(x):
    return x.v if isinstance(x, Bnd) else x


class Forward:
    """The forward of a batch.  kind T32: everything on float32.  kind T64: `decide` is the T32 Forward of the same inputs."""

    def __init__(self, values, flow, metric=None, src_valid=None, t=1.0, importance="none", normalize=False, fill_nan=False, T=T32, decide=None):
        self.T, self.imp, self.normalize, self.t = T, IMPORTANCE[importance], bool(normalize), t
        self.values, self.flow, self.metric, self.valid = values, flow, metric, src_valid
        N, C_, H, W = values.shape
        self.shape = (N, C_, H, W)
        self.dec, self.num, self.den, self.src = [], [], [], []
        for n in range(N):
            m = None if metric is None or self.imp == NONE else metric[n, 0]
            d = decide.dec[n] if decide is not None else Decision(flow[n], m, None if src_valid is None else src_valid[n, 0], t, self.imp)
            num, den, src = _sample_forward(T, d, values[n], flow[n], m, t, self.imp, None if decide is None else decide.src[n][2])
            self.dec.append(d); self.num.append(num); self.den.append(den); self.src.append(src)
        den32 = [_raw(x) for x in (decide.den if decide is not None else self.den)]
        self.pos = [x > 0 for x in den32]
        self.hole_mask = [x == 0 for x in den32]
        fill = np.array([FILL_NAN_BITS], np.uint32).view(F)[0] if fill_nan else F(0)
        self.outs = []
        with np.errstate(all="ignore"):
            for n in range(N):
                self.outs.append(T.where(self.pos[n][None, :], self.num[n] / self.den[n][None, :], T.lift(fill)) if self.normalize else self.num[n])

    def _stack(self, parts, ch):
        N, _, H, W = self.shape
        v = np.stack([_raw(p).reshape(ch, H, W) for p in parts])
        if self.T is T32:
            return v
        return Bnd(v, np.stack([np.broadcast_to(p.e, p.v.shape).reshape(ch, H, W) for p in parts]))

    @property
    def out(self):
        return self._stack(self.outs, self.shape[1])

    @property
    def weight(self):
        return self._stack(self.den, 1)

    @property
    def hole(self):
        N, _, H, W = self.shape
        return np.stack([m.reshape(1, H, W) for m in self.hole_mask]).astype(F)

    @property
    def status(self):
        N, _, H, W = self.shape
        return np.stack([d.status.reshape(1, H, W) for d in self.dec])

    def rows(self):
        """[N + 1, K]: the counts and WEIGHT_MAX exactly; WEIGHT_SUM as the float64 sum of the restatement's den in index order."""
        N, _, H, W = self.shape
        r = np.zeros((N + 1, K))
        for n in range(N):
            st, den = self.dec[n].status, _raw(self.den[n]).astype(np.float64)
            r[n, COL["PIXELS"]] = H * W
            for name, code in (("MASKED", MASKED), ("NONFINITE", NONFINITE), ("OUTSIDE", OUTSIDE), ("SPLATTED", SPLATTED)):
                r[n, COL[name]] = np.sum(st == code)
            r[n, COL["HOLES"]] = np.sum(self.hole_mask[n])
            r[n, COL["WEIGHT_SUM"]] = np.sum(den[~np.isnan(den)])
            r[n, COL["WEIGHT_MAX"]] = np.max(den[~np.isnan(den)], initial=0.0)
        r[N] = r[:N].sum(axis=0)
        r[N, COL["WEIGHT_MAX"]] = r[:N, COL["WEIGHT_MAX"]].max()
        return r

    def backward(self, out_diff, weight_diff=None):
        """(values_diff [N,C,H,W], flow_diff [N,2,H,W], metric_diff [N,1,H,W] or None) in the number type."""
        T, imp = self.T, self.imp
        N, C_, H, W = self.shape
        HW = H * W
        dvs, dfs, dzs = [], [], []
        with np.errstate(all="ignore"):
            for n in range(N):
                d = self.dec[n]
                al, be, w, e = self.src[n]
                S, o = d.S, d.o
                g = T.lift(out_diff[n].reshape(C_, HW))
                vals = T.lift(self.values[n].reshape(C_, HW))
                zero = T.lift(F(0))
                den = [self.den[n][o[k]] for k in range(4)]
                pos = [self.pos[n][o[k]] for k in range(4)]
                gd = [T.zeros(S.size) for _ in range(4)]
                if self.normalize:
                    for k in range(4):
                        sgo = T.zeros(S.size)
                        for c in range(C_):
                            sgo = sgo + g[c][o[k]] * self.outs[n][c][o[k]]
                        gd[k] = T.where(pos[k], T.neg(sgo) / den[k], zero)
                if weight_diff is not None:
                    gw = T.lift(weight_diff[n].reshape(HW))
                    gd = [gd[k] + gw[o[k]] for k in range(4)]
                A = [T.zeros(S.size) for _ in range(4)]
                dv = T.zeros((C_, HW))
                for c in range(C_):
                    v = vals[c][S]
                    sv = T.zeros(S.size)
                    for k in range(4):
                        gk = g[c][o[k]]
                        gn = T.where(pos[k], gk / den[k], zero) if self.normalize else gk
                        A[k] = A[k] + gn * v
                        sv = sv + w[k] * gn
                    dv = T.put(dv, (c, S), sv if imp == NONE else e * sv)
                A = [A[k] + gd[k] for k in range(4)]
                dz = None
                if imp != NONE:
                    de = T.zeros(S.size)
                    for k in range(4):
                        de = de + w[k] * A[k]
                    dz = T.put(T.zeros(HW), S, de if imp == LINEAR else de * e)
                one = T.lift(F(1))
                mal, mbe = one - al, one - be
                dx, dy = T.zeros(S.size), T.zeros(S.size)
                for a_, f_ in ((A[0], T.neg(mbe)), (A[1], mbe), (A[2], T.neg(be)), (A[3], be)):
                    dx = dx + a_ * f_
                for a_, f_ in ((A[0], T.neg(mal)), (A[2], mal), (A[1], T.neg(al)), (A[3], al)):
                    dy = dy + a_ * f_
                if imp != NONE:
                    dx, dy = e * dx, e * dy
                t = T.lift(F(self.t))
                df = T.put(T.put(T.zeros((2, HW)), (0, S), t * dx), (1, S), t * dy)
                dvs.append(dv); dfs.append(df); dzs.append(dz)
        return self._stack(dvs, C_), self._stack(dfs, 2), (None if imp == NONE else self._stack(dzs, 1))


def forward32(values, flow, metric=None, src_valid=None, **kw):
    return Forward(values, flow, metric, src_valid, T=T32, **kw)


def forward64(f32):
    """The float64-with-bound evaluation of the same call, decisions from f32."""
    return Forward(f32.values, f32.flow, f32.metric, f32.valid, t=f32.t, importance={v: k for k, v in IMPORTANCE.items()}[f32.imp],
                   normalize=f32.normalize, T=T64, decide=f32)


def random_case(shape, seed, lo_metric=-4.0):
    """values, flow (uniform in [-a, a], a = min(H, W) / 4), metric in [lo_metric, 0], src_valid (about one in eight masked)."""
    N, C_, H, W = shape
    rng = np.random.RandomState(seed)
    a = min(H, W) / 4.0
    values = rng.uniform(-1, 1, (N, C_, H, W)).astype(F)
    flow = rng.uniform(-a, a, (N, 2, H, W)).astype(F)
    metric = rng.uniform(lo_metric, 0, (N, 1, H, W)).astype(F)
    valid = (rng.uniform(0, 1, (N, 1, H, W)) > 0.125).astype(F)
    return values, flow, metric, valid


def metric_for(importance, metric):
    """random_case's metric as the importance takes it: linear needs z >= 0."""
    return -metric if importance == "linear" else metric
