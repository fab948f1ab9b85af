"""LpqLoss references for the tests: the formulas of include/flownet2_hip_lpq_loss.h in NumPy float64 (ref64) and op by op in float32
(ref32), and an element-wise error bound from the operation count (bound), in the style of solver_ref.bound.

No file of the reference tree is read.  Inputs are the float32 blobs and the float32 values of the scalar arguments the kernel gets."""
import numpy as np

U = 2.0 ** -24               # unit roundoff of float32
TINY = 8 * 2.0 ** -150       # absolute slack for results in the subnormal range (half the smallest subnormal per rounding, 8 roundings)

# Error of the device's powf, in ulps of float32 (1 ulp = 2 U relative).  The HIP math documentation is not installed next to the
# toolchain, so this is MEASURED: powf on an MI355X against pow in float64 over the argument ranges of tests/test_lpq_loss*.py
# (x log-uniform in [1e-7, 1e4], exponents 2, 0.8, 0.6, 0.5, 0.2, -0.2, -0.4, -0.5, -0.8; 2^22 arguments per exponent) gave between
# 1.292 and 1.315 ulp per exponent, 1.3153 at worst (|powf - pow64| in ulps of the exact result, so the final rounding is in it; rounded up
# to 1.32 here); the constant is that with a margin of 2x, because the ulp error of a math function is not
# uniform over its range (profiles/lpq_loss.md).
POWF_MEASURED_ULP = 1.32
E_POW = 2.0 * POWF_MEASURED_ULP


def gamma(k):
    return k * U / (1 - k * U)


def _mode(power):
    return "one" if power == 0 else "identity" if power == 1 else "square" if power == 2 else "general"


def _compute(b0, b1, p, q, p_eps, q_eps, prescale, normalize, top_diff, f):
    """The formulas in dtype f (np.float64: every scalar is the float32 value widened; np.float32: every operation rounds to float32)."""
    p, q, p_eps, q_eps, top_diff = (f(np.float32(x)) for x in (p, q, p_eps, q_eps, top_diff))
    b0 = np.asarray(b0, np.float32).astype(f)
    N, C, H, W = b0.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = b0 - np.asarray(b1, np.float32).astype(f) if b1 is not None else b0
        ok = d == d
        d = np.where(ok, d, f(0))
        a = np.abs(d)
        t = a + p_eps

        def power(x, e):
            m = _mode(e)
            return x if m == "identity" else np.ones_like(x) if m == "one" else np.power(x, e)

        def dpower(x, e):
            m = _mode(e)
            if m == "identity":
                return np.ones_like(x)
            if m == "one":
                return np.zeros_like(x)
            if m == "square":
                return f(2) * x
            return e * (np.power(x, e) / x)

        u = power(t, p)
        w = (f(1) / f(C)) if prescale else f(1)
        s = np.zeros((N, H, W), f)
        for c in range(C):
            s = s + w * u[:, c]
        base = s + q_eps
        v = power(base, q)
        total = np.sum(v.astype(np.float64))
        if normalize:
            norm = f(np.float32(ok.sum())) / f(C) if f is np.float32 else np.float64(ok.sum()) / np.float64(C)
        else:
            norm = f(N)
        loss = np.float64(total) / np.float64(norm)
        alpha = top_diff / norm
        coef = (alpha * dpower(base, q)) * w
        sign = np.where(d > 0, f(1), f(-1))
        g = (coef[:, None] * dpower(t, p)) * sign
        g = np.where(ok, g, f(0))
    out = {"loss": np.float32(loss) if f is np.float32 else loss, "norm": f(norm), "d0": g.astype(f), "d1": (-g).astype(f) if b1 is not None else None}
    out.update(t=t, u=u, s=s, base=base, v=v, ok=ok, d=d, total=total)
    return out


def ref64(b0, b1, p, q, p_eps=0.0, q_eps=1e-2, prescale=False, normalize=False, top_diff=1.0):
    return _compute(b0, b1, p, q, p_eps, q_eps, prescale, normalize, top_diff, np.float64)


def ref32(b0, b1, p, q, p_eps=0.0, q_eps=1e-2, prescale=False, normalize=False, top_diff=1.0):
    return _compute(b0, b1, p, q, p_eps, q_eps, prescale, normalize, top_diff, np.float32)


def _pow_err(e_in, power):
    """Relative error of x^power computed by the PowerLayer rule from an x with relative error e_in."""
    m = _mode(power)
    if m == "one":
        return 0.0
    if m == "identity":
        return e_in
    return (1 - e_in) ** -abs(float(power)) * (1 + 2 * U * E_POW) - 1           # powf (power 2 included: the forward calls it)


def _dpow_err(e_in, power):
    m = _mode(power)
    if m in ("one", "identity"):
        return 0.0
    if m == "square":
        return e_in                                                                # 2 x: exact doubling
    # power * (powf(x, power) / x): x^(power - 1) amplifies e_in by |power - 1|; powf, one division, one product
    return (1 - e_in) ** -abs(float(power) - 1) * (1 + 2 * U * E_POW) * (1 + U) ** 2 - 1


def bound(b0, b1, p, q, p_eps=0.0, q_eps=1e-2, prescale=False, normalize=False, top_diff=1.0):
    """Bounds on |computed - ref64| for the loss, normalize_coeff and every element of the bottom diffs, from the operation count alone.
    Every summand of the forward is non-negative, so nothing cancels and all bounds are relative (r64 below is ref64's value):

      d = b0 - b1            1 rounding, relative to d itself (a float32 difference is correctly rounded)      e_d = U (0 with one bottom)
      t = |d| + p_eps        1 rounding; |d| <= t                                                              e_t = (1 + e_d)(1 + U) - 1
      u = t^p                identity: e_t; power 0: exact; powf: |p| amplifies e_t, E_POW ulps on top         e_u = _pow_err(e_t, p)
      w u                    w = 1 / C is rounded, then the product                                            e_x = (1 + e_u)(1 + U)^2 - 1
      s = sum_c w u_c        C - 1 additions of non-negative terms                                             e_s = (1 + e_x)(1 + gamma(C - 1)) - 1
      base = s + q_eps       1 rounding                                                                        e_b = (1 + e_s)(1 + U) - 1
      v = base^q                                                                                               e_v = _pow_err(e_b, q)
      sum of v in float64    relative 2^-53 per addition, far below U: one U covers it                         e_S = (1 + e_v)(1 + U) - 1
      norm = float(valid) / float(C): conversion and division (N: exact)                                       e_n = gamma(2) (0)
      loss = float(sum / norm)                                                                                 e_l = (1 + e_S)(1 + U) / (1 - e_n) - 1
      alpha = top_diff / norm                                                                                  e_a = (1 + U) / (1 - e_n) - 1
      dq = d base^q / d base: exact for q in {0, 1}; 2 base for q = 2; q (v / base) else (|q - 1| amplifies e_b)  e_dq = _dpow_err(e_b, q)
      coef = (alpha dq) w    2 products and the rounding of w                                                  e_c = (1 + e_a)(1 + e_dq)(1 + U)^3 - 1
      du likewise from t and p                                                                                  e_du = _dpow_err(e_t, p)
      g = (coef du) sign     1 product; the sign of a correctly rounded difference is exact                    e_g = (1 + e_c)(1 + e_du)(1 + U) - 1
    """
    r = ref64(b0, b1, p, q, p_eps, q_eps, prescale, normalize, top_diff)
    C = np.asarray(b0).shape[1]
    e_d = U if b1 is not None else 0.0
    e_t = (1 + e_d) * (1 + U) - 1
    e_u = _pow_err(e_t, p)
    e_x = (1 + e_u) * (1 + U) ** 2 - 1
    e_s = (1 + e_x) * (1 + gamma(max(C - 1, 0))) - 1
    e_b = (1 + e_s) * (1 + U) - 1
    e_v = _pow_err(e_b, q)
    e_S = (1 + e_v) * (1 + U) - 1
    e_n = gamma(2) if normalize else 0.0
    e_l = (1 + e_S) * (1 + U) / (1 - e_n) - 1
    e_a = (1 + U) / (1 - e_n) - 1
    e_c = (1 + e_a) * (1 + _dpow_err(e_b, q)) * (1 + U) ** 3 - 1
    e_g = (1 + e_c) * (1 + _dpow_err(e_t, p)) * (1 + U) - 1
    with np.errstate(invalid="ignore"):
        Eg = np.abs(r["d0"]) * e_g + TINY
    return {"loss": abs(r["loss"]) * e_l + TINY, "norm": abs(r["norm"]) * e_n, "d0": Eg, "d1": Eg if b1 is not None else None, "ref": r}
