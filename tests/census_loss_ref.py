"""Census-loss references for the tests: the arithmetic of include/flownet2_hip_census_loss.h, written once (evaluate) and run twice.

ref32: on NumPy float32 arrays -- every array is float32 and every scalar an np.float32, so a + b, a * b, a / b and np.sqrt (correctly
rounded) are the kernel's operations (compiled without contraction) in the kernel's association.  With gamma == 0.5 (no powf) the kernel
must equal it bit for bit: the planes G, Wg and pd, every count and, given the device's normaliser, every gradient element.  The fp64 sums
DATA_SUM and DIST_SUM are given as the exact sums (math.fsum) of the per-pixel float32 values: the order in which the kernel adds them is
not restated here; the tests hold it by comparing runs with each other.

ref64: on `Bnd` arrays (tests/unsup_loss_ref.py: a float64 value with a running bound on the fp32 kernel's distance from it, the rules
operation by operation in that file's docstring).  Every branch decision (finite, occluded, inside, the tap indices, which values are
defined and so which pairs exist) is taken from the float32 values (decide), so both evaluations give the same pixels the same pairs.
No file of the reference tree is read, and no tolerance here comes from the kernel's output."""
import ctypes as C
import math

import numpy as np

from flownet2_amd import _lib
from flownet2_amd.evaluate import CENSUS_LOSS_COL as COL, CENSUS_LOSS_K as K
from unsup_loss_ref import (Bnd, F, INVALID, OK, TINY, U, WORKSPACE, _directions, _dpsi, _gather, _ok, _psi, _shift, _sqrt, _where, f,  # noqa: F401
                            ptr)

COUNT_COLUMNS = [COL[n] for n in ("PIXELS", "COUNTED", "OCCLUDED", "OUTSIDE", "NONFINITE", "PAIRS")]
SUM_COLUMNS = [COL["DATA_SUM"], COL["DIST_SUM"]]
DEFAULTS = dict(data_weight=1.0, charbonnier=(1e-3, 0.45), radius=3, census_eps=(0.81, 0.1), intensity_scale=255.0, flow_mult=1.0)
EXACT = dict(charbonnier=(1e-3, 0.5))                                               # no powf: bit for bit


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def offsets(radius):
    """q = (dx, dy) in the header's order: dy ascending, then dx ascending, without (0, 0)."""
    return [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dx, dy) != (0, 0)]


def at(h, dx, dy):
    """out[n, y, x] = h[n, y + dy, x + dx], zero (False) where p + q lies outside the plane."""
    return _shift(_shift(h, 2, -dx), 1, -dy)


# ---- the decisions, in float32 --------------------------------------------------------------------------------------------------------
def decide(Ia, Io, a, occ, p):
    """What both evaluations share, decided in float32: cls [N,H,W] (0 counted, 1 occluded, 2 outside, 3 non-finite), the tap indices (0
    where there is no target), where G and Wg are defined, and per q the mask of the pairs (p, q) that exist."""
    N, Cc, H, W = Ia.shape
    mult = F(p["flow_mult"])
    with np.errstate(invalid="ignore", over="ignore"):
        au, av = mult * a[:, 0], mult * a[:, 1]
        fin = _ok(au) & _ok(av)
        occl = fin & ~(occ[:, 0] == 0) if occ is not None else np.zeros_like(fin)
        x2 = np.arange(W, dtype=F)[None, None, :] + au
        y2 = np.arange(H, dtype=F)[None, :, None] + av
        inside = (x2 >= 0) & (y2 >= 0) & (x2 < F(W)) & (y2 < F(H))
    cand = fin & inside                                                             # occ plays no part in whether Wg is defined
    x2, y2 = np.where(cand, x2, F(0)), np.where(cand, y2, F(0))
    ixL, iyT = x2.astype(np.int32), y2.astype(np.int32)
    ixR, iyB = np.minimum(ixL + 1, W - 1), np.minimum(iyT + 1, H - 1)
    assert ixL.min() >= 0 and ixR.max() <= W - 1 and iyT.min() >= 0 and iyB.max() <= H - 1
    tapfin, gdef = np.ones_like(fin), np.ones_like(fin)
    for c in range(Cc):
        gdef &= _ok(Ia[:, c])
        for iy, ix in ((iyT, ixL), (iyT, ixR), (iyB, ixL), (iyB, ixR)):
            tapfin &= _ok(_gather(Io, c, iy, ix))
    wdef = cand & tapfin
    both = gdef & wdef
    cls = np.where(~fin, 3, np.where(occl, 1, np.where(~inside, 2, np.where(both, 0, 3)))).astype(np.int32)
    exists = {q: both & at(both, *q) for q in offsets(int(p["radius"]))}
    return dict(cls=cls, taps=(ixL, ixR, iyT, iyB), gdef=gdef, wdef=wdef, both=both, exists=exists)


# ---- the penalty of a value whose bound may exceed it -----------------------------------------------------------------------------------
# dist carries the bounds of up to 48 pairs, each of a grey value scaled by 255, and may be a few thousandths where the signatures nearly
# agree: its bound can exceed dist itself and eps.  The operation-by-operation rules of unsup_loss_ref (a division by an interval that
# reaches zero, a power of one) then give no bound at all, so psi and psi' are bounded here as functions of one variable: the distance the
# argument's bound can move the exact function (the largest slope over [t - e, t + e] times e), plus the rounding of the evaluation itself,
# which the rules give for an exact argument at t and at both ends of the interval; twice the largest of the three, because it is
# proportional to the value and the value inside the interval exceeds that at an end by less than slope * e, which is already counted.
# For 0 < gamma <= 1, r = t^2 + eps^2:  |psi'| = 2 gamma |t| r^(gamma-1) <= 2 gamma (|t| + e) rmin^(gamma-1) and
# |psi''| = 2 gamma r^(gamma-2) |eps^2 + (2 gamma - 1) t^2| <= 2 gamma rmin^(gamma-1), rmin = max(|t| - e, 0)^2 + eps^2.
def _wide(fn, t, slope):
    c, lo, hi = fn(Bnd(t.v)), fn(Bnd(t.v - t.e)), fn(Bnd(t.v + t.e))
    return Bnd(c.v, slope * t.e + 2 * np.maximum(c.e, np.maximum(lo.e, hi.e)))


def _slopes(t, eps, gam):
    g = float(gam)
    assert 0 < g <= 1 and float(eps.v) > 0
    tmin, tmax = np.maximum(np.abs(t.v) - t.e, 0.0), np.abs(t.v) + t.e
    base = 2 * g * np.power(tmin * tmin + float(eps.v) ** 2, g - 1.0)
    return tmax * base, base                                                        # of psi, of psi'


def psi(t, eps, gam):
    return _wide(lambda s: _psi(s, eps, gam), t, _slopes(t, eps, gam)[0]) if isinstance(t, Bnd) else _psi(t, eps, gam)


def dpsi(t, eps, gam):
    return _wide(lambda s: _dpsi(s, eps, gam), t, _slopes(t, eps, gam)[1]) if isinstance(t, Bnd) else _dpsi(t, eps, gam)


# ---- the arithmetic, once ---------------------------------------------------------------------------------------------------------
def evaluate(Ia, Io, a, dec, p, bounded, kd=None):
    """One direction: the planes G, Wg, the per-pair h, the per-pixel dist, e = psi(dist) and pd = psi'(dist) and, with the normaliser kd,
    the gradient (du, dv), as float32 arrays (bounded False) or as Bnd (True).  G and Wg hold anything where they are not defined."""
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
    c_t, c_h = const(p["census_eps"][0]), const(p["census_eps"][1])
    gsc, mult = const(F(p["intensity_scale"]) / F(Cc)), const(p["flow_mult"])      # gsc: one float32 division on the host
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
        gs, ws, Su, Sv = zero, zero, zero, zero
        for c in range(Cc):
            TL, TR, BL, BR = (num(_gather(Io, c, iy, ix)) for iy, ix in ((iyT, ixL), (iyT, ixR), (iyB, ixL), (iyB, ixR)))
            gs = gs + num(Ia[:, c])
            ws = ws + (((cTL * TL + cTR * TR) + cBL * BL) + cBR * BR)
            Su = Su + (gy * (TR - TL) + (one - gy) * (BR - BL))
            Sv = Sv + (gx * (BL - TL) + (one - gx) * (BR - TR))
        G, Wg = gs * gsc, ws * gsc
        counted = dec["cls"] == 0
        pairs = []
        dist = zero
        for q in offsets(int(p["radius"])):
            ex = dec["exists"][q]
            da = at(G, *q) - G
            ra = da * da + c_t
            ta = da / _sqrt(ra)
            db = at(Wg, *q) - Wg
            rb = db * db + c_t
            tb = db / _sqrt(rb)
            e = ta - tb
            s = e * e
            den = s + c_h
            h = s / den
            dist = _where(ex, dist + h, dist)
            pairs.append((q, ex, h, e, den, rb))
        dist = _where(counted, dist, zero)
        out = dict(G=G, Wg=Wg, dist=dist, e=_where(counted, psi(dist, eps_d, gam_d), zero), pd=_where(counted, dpsi(dist, eps_d, gam_d), zero),
                   h={q: _where(ex, h, zero) for q, ex, h, *_ in pairs})
        if kd is not None:
            pd, acc = out["pd"], zero
            for q, ex, h, e, den, rb in pairs:
                Fq = (-(((two * c_h) * e) / (den * den))) * (c_t / (rb * _sqrt(rb)))
                acc = _where(ex, acc + (pd + at(pd, *q)) * Fq, acc)
            DW = (-kd) * acc
            there = dec["both"]
            out["du"] = _where(there, mult * ((DW * gsc) * Su), zero)
            out["dv"] = _where(there, mult * ((DW * gsc) * Sv), zero)
    return out


# ---- the rows -------------------------------------------------------------------------------------------------------------------------
def _count_rows(dec, N):
    rows = np.zeros((N + 1, K), np.float64)
    cls = dec["cls"].reshape(N, -1)
    rows[:N, COL["PIXELS"]] = cls.shape[1]
    for name, v in (("COUNTED", 0), ("OCCLUDED", 1), ("OUTSIDE", 2), ("NONFINITE", 3)):
        rows[:N, COL[name]] = (cls == v).sum(1)
    counted = dec["cls"] == 0
    rows[:N, COL["PAIRS"]] = sum((ex & counted).reshape(N, -1).sum(1) for ex in dec["exists"].values())
    return rows


def _kd(p, rows_d, total_diff, N):
    return F(total_diff) * F(float(F(p["data_weight"])) / max(rows_d[N, COL["COUNTED"]], 1.0))


def ref32(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, p=None, total_diff=1.0, rows=None):
    """dict(rows [2, N + 1, K] float64 (DATA_SUM, DIST_SUM: the exact sums of the float32 values), sum_abs [2, N + 1, K] (sum |v| of those two
    columns, for the tests' n 2^-53 sum|v|), loss float32 (from these rows), planes [per direction [N,3,H,W] float32: G, Wg (NaN where not
    defined), pd], diff [per direction [N,2,H,W] float32], h [per direction {q: [N,H,W]}], cls).  rows: the device's results, from which
    the backward's normaliser is then taken, as the kernel takes it."""
    p = p or params()
    N, Cc, H, W = img0.shape
    out_rows, sum_abs = np.zeros((2, N + 1, K), np.float64), np.zeros((2, N + 1, K), np.float64)
    planes, diffs, hs, clss, L = [], [], [], [], 0.0
    dw = float(F(p["data_weight"]))
    for d, (Ia, Io, a, occ) in enumerate(_directions(img0, img1, fw, bw, occ_fw, occ_bw)):
        dec = decide(Ia, Io, a, occ, p)
        r = _count_rows(dec, N)
        ev = evaluate(Ia, Io, a, dec, p, bounded=False)
        for n in range(N):
            for col, v in ((COL["DATA_SUM"], ev["e"][n]), (COL["DIST_SUM"], ev["dist"][n])):
                r[n, col] = math.fsum(v.astype(np.float64).ravel())
                sum_abs[d, n, col] = math.fsum(np.abs(v).astype(np.float64).ravel())
        for k in range(K):
            r[N, k] = math.fsum(r[:N, k])
        sum_abs[d, N] = sum_abs[d, :N].sum(0)
        out_rows[d] = r
        L = L + (dw * r[N, COL["DATA_SUM"]]) / max(r[N, COL["COUNTED"]], 1.0)
        kd = _kd(p, (rows if rows is not None else out_rows)[d], total_diff, N)
        ev = evaluate(Ia, Io, a, dec, p, bounded=False, kd=kd)
        assert all(ev[k].dtype == F for k in ("G", "Wg", "dist", "e", "pd", "du", "dv"))
        nan = F(np.nan)
        planes.append(np.stack([np.where(dec["gdef"], ev["G"], nan), np.where(dec["wdef"], ev["Wg"], nan), ev["pd"]], 1))
        diffs.append(np.stack([ev["du"], ev["dv"]], 1))
        hs.append(ev["h"])
        clss.append(dec["cls"])
    return dict(rows=out_rows, sum_abs=sum_abs, loss=F(L), planes=planes, diff=diffs, h=hs, cls=clss)


def ref64(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, p=None, total_diff=1.0):
    """The float64 evaluation with its bounds: dict(rows, rows_bound [2, N + 1, K], loss, loss_bound, diff, diff_bound [per direction])."""
    p = p or params()
    N, Cc, H, W = img0.shape
    rows, rbound, diffs, dbounds = np.zeros((2, N + 1, K)), np.zeros((2, N + 1, K)), [], []
    dw = float(F(p["data_weight"]))
    L, Lb = 0.0, 0.0
    for d, (Ia, Io, a, occ) in enumerate(_directions(img0, img1, fw, bw, occ_fw, occ_bw)):
        dec = decide(Ia, Io, a, occ, p)
        r, rb = _count_rows(dec, N), np.zeros((N + 1, K))
        cd = max(r[:N, COL["COUNTED"]].sum(), 1.0)
        kd = Bnd.rounded(dw / cd, 0.0) * float(F(total_diff))
        ev = evaluate(Ia, Io, a, dec, p, bounded=True, kd=kd)
        for col, t in ((COL["DATA_SUM"], ev["e"]), (COL["DIST_SUM"], ev["dist"])):
            v = t.v.reshape(N, -1).sum(1)
            r[:N, col], rb[:N, col] = v, t.e.reshape(N, -1).sum(1) + H * W * 2.0 ** -53 * np.abs(t.v).reshape(N, -1).sum(1)
        r[N] = r[:N].sum(0)
        rb[N] = rb[:N].sum(0) + N * 2.0 ** -53 * np.abs(r[N])
        rb[:, COUNT_COLUMNS] = 0
        rows[d], rbound[d] = r, rb
        L += dw * r[N, COL["DATA_SUM"]] / cd
        Lb += dw * rb[N, COL["DATA_SUM"]] / cd
        diffs.append(np.stack([ev["du"].v, ev["dv"].v], 1))
        dbounds.append(np.stack([ev["du"].e, ev["dv"].e], 1))
    return dict(rows=rows, rows_bound=rbound, loss=L, loss_bound=Lb + 2 * U * abs(L) + TINY, diff=diffs, diff_bound=dbounds)


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------
def make_inputs(shape, kind, seed):
    """[img0, img1, fw, bw, occ_fw, occ_bw] from unsup_loss_ref's make_images / make_flows / make_occ, kind "small", "large" or
    "nonfinite" (small flows, then poison), brought to the map so that an unpoisoned case keeps at least two thirds of its pixels COUNTED
    (the tests assert it): "large" flows are scaled to a fifth of the smaller extent (many targets outside, not most of them); on a map with
    an extent below 4, where every flow that points outward from a border pixel loses it, the flows are made non-negative and below one
    pixel, which keeps every target inside; the occlusion planes keep every second of their pixels, about a tenth of the map."""
    from unsup_loss_ref import make_flows, make_images, make_occ, poison
    N, Cc, H, W = shape
    img0, img1 = make_images(shape, seed)
    fw, bw = make_flows(shape, seed, "large" if kind == "large" else "small")
    if min(H, W) < 4:
        top = max(np.abs(fw).max(), np.abs(bw).max())
        fw, bw = ((np.abs(t) * F(0.9 / top)).astype(F) for t in (fw, bw))
    elif kind == "large":
        fw, bw = ((t * F(0.2 * min(H, W) / (0.6 * max(H, W) + 2.0))).astype(F) for t in (fw, bw))
    keep = np.random.default_rng(seed + 4000).random((2, N, 1, H, W)) < 0.5
    occ_fw, occ_bw = ((o * k).astype(F) for o, k in zip(make_occ(shape, seed), keep))
    arrays = [img0, img1, fw, bw, occ_fw, occ_bw]
    if kind == "nonfinite":
        poison(arrays, seed)
    return arrays


def not_counted_share(rows):
    """The share of the pixels of the directions run that are not COUNTED, from the totals rows of [2, N + 1, K]."""
    tot = rows[:, -1]
    return 1.0 - tot[:, COL["COUNTED"]].sum() / max(tot[:, COL["PIXELS"]].sum(), 1.0)


def descent_images():
    """img0 and img1 = img0 translated by 2 px along x PLUS a brightness offset of 0.25: smooth sinusoids [1,1,16,32]; the true forward
    flow is (+2, 0).  (The brightness-constancy term of unsup_loss_ref is larger at the true flow than at zero flow on this pair: 0.2872
    against 0.2844.)"""
    H, W = 16, 32
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    g = lambda x, y: 0.4 + 0.25 * np.sin(2 * np.pi * x / 16 + 0.3) * np.cos(2 * np.pi * y / 32) + 0.2 * np.sin(2 * np.pi * (x / 32 + y / 16) + 1.0)
    return g(x, y)[None, None].astype(F), (g(x - 2, y) + 0.25)[None, None].astype(F)


# 40 plain gradient steps of size 10 on the forward flow from zero, the defaults (radius 3, gamma 0.45).  On the float64 restatement (run
# before the kernel was): loss 6.510285 -> 3.001585, EPE against (2, 0) over the counted pixels 2.0 -> 1.540722.  (Step 5: 3.218707 and
# 1.668501; 15: 3.672158 and 1.600748; 20: 4.031000 and 1.672921; at 50 and above the EPE grows.)
DESCENT = dict(step=10.0, steps=40)


def descent_epe(fw, p):
    """The mean distance of fw [1,2,16,32] from the true flow (2, 0) over the pixels the restatement counts."""
    img0, img1 = descent_images()
    counted = decide(img0, img1, np.ascontiguousarray(fw, F), None, p)["cls"][0] == 0
    return float(np.sqrt((fw[0, 0].astype(np.float64) - 2) ** 2 + fw[0, 1].astype(np.float64) ** 2)[counted].mean()), int(counted.sum())


# ---- the raw C ABI --------------------------------------------------------------------------------------------------------------------
def sizes(N, H, W, radius=3):
    nbytes, nsaved, k = C.c_size_t(), C.c_size_t(), C.c_int()
    assert _lib.lib().fn2_census_loss_sizes(int(N), int(H), int(W), int(radius), C.byref(nbytes), C.byref(nsaved), C.byref(k)) == OK
    return nbytes.value, nsaved.value, k.value


def tiles(H, W):
    return -(-W // 32) * -(-H // 8)


def scalars(p):
    (ed, gd), (ct, ch) = p["charbonnier"], p["census_eps"]
    return (f(p["data_weight"]), f(ed), f(gd), int(p["radius"]), f(ct), f(ch), f(p["intensity_scale"]), f(p["flow_mult"]))


def forward(img0, img1, fw, bw, occ_fw, occ_bw, shape, p, results, loss, saved, ws, ws_bytes, stream=None):
    N, Cc, H, W = shape
    return _lib.lib().fn2_census_loss_forward(ptr(img0), ptr(img1), ptr(fw), ptr(bw), ptr(occ_fw), ptr(occ_bw), int(N), int(Cc), int(H), int(W),
                                              *scalars(p), ptr(results), ptr(loss), ptr(saved), ptr(ws), int(ws_bytes), stream)


def backward(img0, img1, fw, bw, shape, p, results, saved, total_diff, fw_diff, bw_diff, stream=None):
    N, Cc, H, W = shape
    return _lib.lib().fn2_census_loss_backward(ptr(img0), ptr(img1), ptr(fw), ptr(bw), int(N), int(Cc), int(H), int(W), *scalars(p),
                                               ptr(results), ptr(saved), ptr(total_diff), ptr(fw_diff), ptr(bw_diff), stream)
