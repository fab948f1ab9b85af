"""Bounds and launch plan of Resample shared by tests/test_resample.py and tests/test_oracle.py (no GPU, no flownet2_amd import).
The derivation of every constant is in the docstring of tests/test_resample.py."""
import numpy as np

import ref_torch64 as R

U = 2.0 ** -24
NEAREST, LINEAR, CUBIC = 1, 2, 3                      # FN2_RESAMPLE_*
KIND = {LINEAR: "linear", CUBIC: "cubic"}
C_CONST = 8
ILL_CAP = 0.02


def rand(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def resample_plan(NC, Hin, Win, Hout, Wout, code, antialias, aligned_top=True, generic=False):
    """(branch, planes per thread) as fn2_resample_forward_slices selects them; ('refused', 0) for FN2_ERR_UNSUPPORTED."""
    g = R.resample_geometry(Hin, Win, Hout, Wout, KIND.get(code, "linear"), antialias)
    bx = (Hout * Wout + 255) // 256
    ppt = 1
    while ppt < 8 and bx * ((NC + 2 * ppt - 1) // (2 * ppt)) >= 2048:
        ppt *= 2
    if (NC + ppt - 1) // ppt > 65535:
        return "refused", 0
    fast = g["rx"] <= 2 and g["ry"] <= 2
    up = 4 if (Wout, Hout) == (4 * Win, 4 * Hin) else 2 if (Wout, Hout) == (2 * Win, 2 * Hin) else 0
    if code == LINEAR and up and aligned_top and not generic:
        bxi = (Hin * Win + 255) // 256
        ppt = 1
        while ppt < 4 and bxi * ((NC + 2 * ppt - 1) // (2 * ppt)) >= 8192:
            ppt *= 2
        return ("refused", 0) if (NC + ppt - 1) // ppt > 65535 else ("up%d" % up, ppt)
    if (code == LINEAR and fast and g["ax"] == 1 and g["ay"] == 1 and g["rx"] == 2 and g["ry"] == 2 and g["fx"] <= 1 and g["fy"] <= 1
            and not generic):
        tiles_y, groups = (Hout + 31) // 32, (NC + 1) // 2
        return ("refused", 0) if tiles_y > 65535 or groups > 65535 else ("lean", 2)
    if code == NEAREST:
        return "nearest", ppt
    return ("cubic" if code == CUBIC else "linear") + ("_fast" if fast else "_slow"), ppt


def classify(st, code):
    """(zero [Hout,Wout], ill [N,C,Hout,Wout], tau).  zero: must be exactly +0.0;  ill: only the ill-conditioned assertions."""
    tau = (st["m"] + C_CONST) * U * st["Aw"] + (st["Awe"] if code == CUBIC else 0.0)
    zero = (st["ws"] == 0) & ~st["edge"]
    ill = np.broadcast_to((np.abs(st["ws"]) <= tau) & ~zero, st["ref"].shape)
    return zero, ill, tau


def bound_of(st, code):
    """The elementwise bound [N,C,Hout,Wout] (inf / NaN where ws == 0) and the host-side preconditions on the bounded outputs."""
    zero, ill, tau = classify(st, code)
    well = ~zero & ~ill
    aws = np.broadcast_to(np.abs(st["ws"]), well.shape)
    assert (aws[well] >= 64 * np.broadcast_to(tau, well.shape)[well]).all(), "a bounded output has |ws| < 64 tau: choose another shape"
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        b = (st["m"] + C_CONST) * U * (st["A"] + np.abs(st["ref"]) * st["Aw"]) / aws
        if code == CUBIC:                                          # the polynomial's absolute error near its zeros, measured
            b = b + (st["Ae"] + np.abs(st["ref"]) * st["Awe"]) / aws
    return b, zero, ill, well


def check(out, x, Hout, Wout, code, antialias, what, in_scale=1.0, cap=ILL_CAP, st=None):
    """Every assertion of the docstring on one output blob.  Returns the worst error-to-bound ratio."""
    out = np.asarray(out, np.float32)
    st = st if st is not None else R.resample_statement(x, Hout, Wout, KIND[code], antialias, in_scale)
    ref = st["ref"]
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    b, zero, ill, well = bound_of(st, code)
    if cap is not None:
        assert ill.mean() <= cap, f"{what}: {ill.mean():.1%} of the outputs are ill-conditioned (cap {cap:.0%})"
    sel = well
    got, want, bound = out[sel].astype(np.float64), ref[sel], b[sel]
    gn, rn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, rn), f"{what}: NaN pattern differs ({int(gn.sum())} vs {int(rn.sum())})"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all(), f"{what}: non-finite value where the fp64 statement is finite"
    err = np.abs(got[fin] - want[fin])
    bad = err > bound[fin]
    if bad.any():
        i = int(np.argmax(np.where(bad, err / bound[fin], 0)))
        where = np.argwhere(sel & np.isfinite(ref))[i].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements over the bound; at {where}: |{got[fin][i]!r} - {want[fin][i]!r}| = "
                             f"{err[i]:.3e} > {bound[fin][i]:.3e}")
    z = np.broadcast_to(zero, out.shape)
    assert (bits(out[z]) == 0).all(), f"{what}: {int((bits(out[z]) != 0).sum())} outputs with ws == 0 are not exactly +0.0"
    check_ill(out, st, ill, code, what)
    ratio = float((err / np.where(bound[fin] > 0, bound[fin], 1)).max()) if err.size else 0.0
    print(f"resample ratio {what}: {ratio:.3g}  (zero {int(zero.sum())} of {zero.size} pixels, ill {int(ill.sum())} of {ill.size} outputs)")
    return ratio


def check_ill(out, st, ill, code, what):
    """Ill-conditioned outputs whose window holds finite taps only: finite; LINEAR also +0.0 or inside the widened hull of the taps."""
    if not np.any(ill):
        return
    lo, hi = st["hull"]()
    sel = np.broadcast_to(ill, out.shape) & np.isfinite(lo) & np.isfinite(hi) & (lo <= hi)
    got = out[sel].astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite ill-conditioned output"
    if code == LINEAR:
        lo, hi = lo[sel], hi[sel]
        wide = 4 * U * np.maximum(np.abs(lo), np.abs(hi))
        ok = (bits(out[sel]) == 0) | ((got >= lo - wide) & (got <= hi + wide))
        assert ok.all(), f"{what}: {int((~ok).sum())} ill-conditioned outputs outside the hull of their taps"
