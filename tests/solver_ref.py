"""Yardsticks of the solver update (shared by tests/test_solver_update.py and tests/test_solver_step.py; not a test module).

ref64     the formulas of include/flownet2_hip_solver.h in NumPy float64, on the float32 inputs and the float32 constants the kernel receives
ref32     the same op by op in NumPy float32 (every operation rounded on its own, like the kernel with contraction off)
bound     the one-step error bound, a function of u = 2^-24 and the inputs only (derivation in its docstring)
"""
import numpy as np

U = 2.0 ** -24


def gamma(k):
    """k roundings in sequence: (1 + u)^k - 1 <= k u / (1 - k u)."""
    return k * U / (1 - k * U)


def constants(type_, rate, correction, momentum, momentum2, delta, weight_decay, lr_mult, decay_mult, accum, clip_scale=1.0):
    """Per-element float32 constants exactly as csrc/solver_update.hip forms them (lr_mult / decay_mult: arrays, one value per element)."""
    f = np.float32
    c = {"type": type_, "b1": f(momentum), "b2": f(momentum2), "delta": f(delta), "an": f(accum), "cs": f(clip_scale)}
    c["omb1"], c["omb2"] = f(1) - c["b1"], f(1) - c["b2"]                      # formed in fp32 from the fp32 betas
    c["ld"] = (f(weight_decay) * decay_mult.astype(f)).astype(f)                # local_decay = weight_decay * decay_mult
    lr = (f(rate) * lr_mult.astype(f)).astype(f)                                # local_rate = rate * lr_mult
    c["lr"] = (lr * f(correction)).astype(f) if type_ == "Adam" else lr         # Adam: clr = local_rate * correction
    return c


def _reg_operand(w, l1):
    return np.sign(w) if l1 else w


def ref64(w, g, h0, h1, c, l1=False):
    """-> dict(h0, h1, upd, w) in float64."""
    d = np.float64
    w, g, h0 = w.astype(d), g.astype(d), h0.astype(d)
    g1 = g * d(c["cs"]) * d(c["an"])
    g2 = g1 + c["ld"].astype(d) * _reg_operand(w, l1)
    if c["type"] == "SGD":
        nh0 = d(c["b1"]) * h0 + c["lr"].astype(d) * g2
        return {"h0": nh0, "h1": None, "upd": nh0, "w": w - nh0, "g1": g1, "g2": g2}
    h1 = h1.astype(d)
    nh0 = h0 * d(c["b1"]) + g2 * d(c["omb1"])
    nh1 = h1 * d(c["b2"]) + g2 * g2 * d(c["omb2"])
    upd = c["lr"].astype(d) * nh0 / (np.sqrt(nh1) + d(c["delta"]))
    return {"h0": nh0, "h1": nh1, "upd": upd, "w": w - upd, "g1": g1, "g2": g2}


def ref32(w, g, h0, h1, c, l1=False, clip_on=False):
    """The kernel's sequence in float32, one rounding per operation.  The clip multiply happens only with clipping on (x * 1 is exact anyway);
    the decay is skipped where local_decay == 0, as the kernel skips it."""
    f = np.float32
    w, g, h0 = w.astype(f), g.astype(f), h0.astype(f)
    if clip_on:
        g = g * c["cs"]
    g = g * c["an"]
    with np.errstate(invalid="ignore"):
        t = c["ld"] * _reg_operand(w, l1).astype(f)
        g = np.where(c["ld"] != 0, g + t, g).astype(f)
    if c["type"] == "SGD":
        nh0 = (c["b1"] * h0 + c["lr"] * g).astype(f)
        return {"h0": nh0, "h1": None, "upd": nh0, "w": (w - nh0).astype(f)}
    h1 = h1.astype(f)
    nh0 = (h0 * c["b1"] + g * c["omb1"]).astype(f)
    nh1 = (h1 * c["b2"] + (g * g) * c["omb2"]).astype(f)
    upd = ((c["lr"] * nh0) / (np.sqrt(nh1) + c["delta"])).astype(f)
    return {"h0": nh0, "h1": nh1, "upd": upd, "w": (w - upd).astype(f)}


def bound(w, g, h0, h1, c, l1=False):
    """Elementwise bounds on |computed - ref64| for h0, h1, upd and w, from the operation count alone.  u = 2^-24 is the unit roundoff of
    float32, gamma(k) = k u / (1 - k u) bounds k roundings in sequence; fusing a multiply into an add removes a rounding and never adds
    one, so the bounds hold with and without fma contraction.  sqrt and division are taken as accurate to 1 ulp = 2 u (they are
    correctly rounded in the default build; 1 ulp is what the HIP math library documents), every other operation to u.

      g1 = (g * cs) * an                      2 roundings
      g2 = g1 + ld * r      (r = w | sign w)  2 more             Eg  = gamma(3) (|g1| + |ld r|)
      SGD   h0' = b1 h0 + lr g2               2 products, 1 sum  E0  = gamma(2) (|b1 h0| + |lr| (|g2| + Eg)) + |lr| Eg
      Adam  h0' = h0 b1 + g2 omb1             2 products, 1 sum  E0  = gamma(2) (|h0 b1| + |omb1| (|g2| + Eg)) + |omb1| Eg
            h1' = h1 b2 + (g2 g2) omb2        3 products, 1 sum  Dg  = 2 |g2| Eg + Eg^2   (the error of g2^2 before it is rounded)
                                                                 E1  = gamma(3) (|h1 b2| + |omb2| (g2^2 + Dg)) + |omb2| Dg
            num = clr h0'                     1 product          En  = |clr| E0 + u |clr| (|h0'| + E0)
            den = sqrt(h1') + delta           sqrt, 1 sum        Es  = min(E1 / sqrt(h1'), sqrt(E1)) + 2 u (sqrt(h1') + that)
                                                                 Ed  = Es + u (den + Es)
            upd = num / den                   1 division         Eu  = (En + |upd| Ed) / (den - Ed);   Eu' = Eu + 2 u (|upd| + Eu)
      w' = w - upd                            1 sum              Ew  = Eu' + u (|w'| + Eu')            (SGD: Eu' = E0)
    """
    d = np.float64
    r = ref64(w, g, h0, h1, c, l1)
    ld, lr = np.abs(c["ld"].astype(d)), np.abs(c["lr"].astype(d))
    Eg = gamma(3) * (np.abs(r["g1"]) + ld * np.abs(_reg_operand(w.astype(d), l1)))
    g2 = np.abs(r["g2"])
    if c["type"] == "SGD":
        E0 = gamma(2) * (np.abs(d(c["b1"]) * h0.astype(d)) + lr * (g2 + Eg)) + lr * Eg
        Eu = E0
        out = {"h0": E0, "h1": None, "upd": Eu}
    else:
        omb1, omb2 = abs(d(c["omb1"])), abs(d(c["omb2"]))
        E0 = gamma(2) * (np.abs(h0.astype(d) * d(c["b1"])) + omb1 * (g2 + Eg)) + omb1 * Eg
        Dg = 2 * g2 * Eg + Eg * Eg
        E1 = gamma(3) * (np.abs(h1.astype(d) * d(c["b2"])) + omb2 * (g2 * g2 + Dg)) + omb2 * Dg
        En = lr * E0 + U * lr * (np.abs(r["h0"]) + E0)
        s = np.sqrt(r["h1"])
        with np.errstate(divide="ignore", invalid="ignore"):
            Es = np.where(s > 0, np.minimum(E1 / np.where(s > 0, s, 1), np.sqrt(E1)), np.sqrt(E1))
        Es = Es + 2 * U * (s + Es)
        den = s + d(c["delta"])
        Ed = Es + U * (den + Es)
        assert np.all(den - Ed > 0)
        Eu = (En + np.abs(r["upd"]) * Ed) / (den - Ed)
        Eu = Eu + 2 * U * (np.abs(r["upd"]) + Eu)
        out = {"h0": E0, "h1": E1, "upd": Eu}
    out["w"] = Eu + U * (np.abs(r["w"]) + Eu)
    return out, r


def worst_ratio(got, ref, bnd):
    """max over elements of |got - ref| / bound (0 / 0 counts as 0); inf where an error exceeds a zero bound."""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bnd)
    return float(q.max()) if q.size else 0.0
