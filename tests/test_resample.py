"""Resample (csrc/resample.hip) against the fp64 statement of the reference (ref_torch64.resample_statement / resample_nearest), on
every launch branch of fn2_resample_forward_slices.

The statement rounds fx, fy, ax, ay, rx, ry and the source positions to fp32 as the host function and the kernels do
(x_in = fp32(fp32(fp32(x*fx) + fp32(fy/2)) - 0.5) -- the reference's swapped half-pixel offsets -- and the window centre is
roundf of it); coefficients, products, sum, wsum and the division are fp64 over the in-image taps of that window.  Per output
element it gives ref, ws = sum w, A = sum |w tap|, Aw = sum |w| and the tap count m.

Bounds, u = 2^-24:
  * NEAREST: bitwise, the clamped sample.
  * LINEAR:  |hip - ref| <= (m + c) u (A + |ref| Aw) / |ws|,  c = 8.
    CUBIC:   the same plus (Ae + |ref| Awe) / |ws|, the absolute error of the fp32 polynomial near its zeros.
      m counts the in-image taps whose coefficient is not 0 (a coefficient of exactly 0 adds +0: no rounding).  The fp32 weight
      ((ax k(tx)) ay) k(ty) carries three product roundings, and LINEAR's 1 - |t| one more per axis: 5u relative to the weight.
      sum and wsum are chains of m fused multiply-adds / additions: m u (A resp. Aw) to first order.  The quotient
      (sum + dS) / (wsum + dW) - ref = (dS - ref dW) / (wsum + dW), plus one rounding of the division (u |ref| <= u |ref| Aw / |ws|):
      (m + 6) u (A + |ref| Aw) / |ws|.  The other 2u cover the second-order terms: (1 + u)^m, and 1 / (1 - dW / ws), for which the
      host asserts |ws| >= 64 tau on every bounded output.
      CUBIC's polynomial cancels near its zeros (|t| = 1, 2): there k is off by a few u however small it is, which is not relative
      to the weight.  This part is not estimated but measured: the statement also forms the kernels' fp32 coefficient k32 from the
      same fp32 position, operation by operation (ref_torch64._coeff32; the file is compiled without contraction), and
      Ae = sum |w32 - w| |tap|, Awe = sum |w32 - w| enter CUBIC's bound and tau as they are.  LINEAR gets no such term.
  * ill-conditioned outputs: |ws| <= tau = (m + c) u Aw (CUBIC: + Awe), the bound on the error of wsum itself.  There an fp32 weight of
      order u decides the result (a tap exactly at the edge of the support).  LINEAR: the output is finite and either exactly +0.0
      (fp32 wsum == 0, :93) or within [min, max] of the taps of its window widened by 4u max|tap| (non-negative weights: a convex
      combination);  CUBIC: finite.  At most 2 % of a case's outputs may be ill-conditioned.
  * ws == 0 in fp64 and fp32 agrees that every in-image coefficient is 0 (this includes the empty window): exactly +0.0.
  * NaN patterns equal, infinities identical, nothing non-finite where the fp64 value is finite.
(7,50)->(21,10): fy = 1/3 and fx = 5 put y_in = y/3 + 2 on a half or an integer for a third of the rows, whose LINEAR taps then sit
at |t| = 1 to the last bit.  ref_torch64.resample, which forms positions in fp64, differs from the kernels by O(1) there (asserted);
with fp32 positions this statement has no ill-conditioned output there, so the case gets the bounds AND the
ill-conditioned assertions on every output.

Branches of the host function (resample_plan below restates the selection; every case asserts where it lands):
  nearest                      NEAREST
  cubic_fast / cubic_slow      interp<CUBIC, FAST / !FAST>: radius <= 2 on both axes (up-sampling) / anything else.  The identity is
                               NOT fast: fx == 1 gives rx = ceil(4 / 1) = 4.
  linear_fast / linear_slow    interp<LINEAR, ...>: fast without the debug hook only for non-antialiased down-sampling (rx = ry = 2 but
                               fx > 1 or fy > 1 keeps it off the lean kernel); slow = antialiased down-sampling
  lean                         resample_linear_lean: LINEAR, unit tap scale, fx, fy <= 1; 16-byte scan (Win % 4 == 0 and an aligned
                               bottom) or scalar scan; finite or poisoned footprint
  up2 / up4                    resample_up_linear<2 / 4>: exact integer factor and 16-byte aligned tops, else lean
  ppt                          planes per thread 1, 2, 4, 8 (per-pixel kernels) and 1, 2, 4 (up), ragged last group
  EXTRA                        in_scale != 1, a top slice of a wider blob, a second top
  refused                      too many plane groups: FN2_ERR_UNSUPPORTED, nothing written

Worst error / bound on the MI355X per kernel family (this file's printed ratios): cubic_fast 0.86, cubic_slow 0.75, linear_fast
0.11, linear_slow 0.16, lean 0.15, up2 0.13, up4 0.10 (the C oracle on the CPU: cubic 0.53, linear 0.16).  CUBIC comes close to 1
because most of its bound is the measured coefficient error, which is an error the kernel really has, not an estimate.
Tests marked gpu need the MI355X; the others check the statement, the bounds' teeth and the C oracle on the CPU.
"""
import numpy as np
import pytest
import torch

import oracle
import ref_torch64 as R
from flownet2_amd import ops
from resample_bounds import (CUBIC, KIND, LINEAR, NEAREST, U, bits, bound_of, check, check_ill, classify, rand, resample_plan)

assert (NEAREST, LINEAR, CUBIC) == (ops.NEAREST, ops.LINEAR, ops.CUBIC)
FN2_ERR_UNSUPPORTED = -2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b, what):
    """Bit equality, any NaN equal to any NaN (the kernels agree on values; NaN payloads are not part of the contract)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    assert np.array_equal(an, bn), f"{what}: NaN pattern differs"
    assert np.array_equal(bits(a)[~an], bits(b)[~bn]), f"{what}: bits differ"


def gpu_resample(x, Hout, Wout, code, antialias, generic=False):
    if generic:
        ops.set_resample_generic(True)
    try:
        return host(ops.resample_forward(x if isinstance(x, torch.Tensor) else dev(x), Hout, Wout, code, antialias))
    finally:
        if generic:
            ops.set_resample_generic(False)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

NEAREST_SHAPES = [((4, 6), (8, 12)), ((8, 12), (4, 6)), ((16, 20), (8, 10)), ((9, 12), (9, 12)), ((12, 16), (7, 9)), ((5, 7), (11, 13)),
                  ((12, 64), (12, 8)), ((64, 12), (8, 12)), ((8, 32), (32, 8)), ((32, 8), (8, 32)), ((7, 50), (20, 11))]
MIXED = [((12, 64), (12, 8)), ((64, 12), (8, 12)), ((8, 32), (32, 8)), ((32, 8), (8, 32)), ((7, 50), (20, 11))]
# (type, (Hin, Win), (Hout, Wout), antialias, branch)
INTERP_CASES = [
    (CUBIC, (6, 8), (24, 32), True, "cubic_fast"), (CUBIC, (5, 7), (11, 13), False, "cubic_fast"), (CUBIC, (9, 12), (9, 12), True, "cubic_slow"),
    (CUBIC, (16, 20), (8, 10), True, "cubic_slow"), (CUBIC, (16, 20), (8, 10), False, "cubic_slow"),
    (CUBIC, (12, 16), (7, 9), True, "cubic_slow"), (CUBIC, (12, 16), (7, 9), False, "cubic_slow"),
    (LINEAR, (16, 20), (8, 10), False, "linear_fast"), (LINEAR, (12, 16), (7, 9), False, "linear_fast"), (LINEAR, (20, 8), (10, 16), False, "linear_fast"),
    (LINEAR, (16, 20), (8, 10), True, "linear_slow"), (LINEAR, (12, 16), (7, 9), True, "linear_slow"), (LINEAR, (20, 8), (10, 16), True, "linear_slow"),
    (LINEAR, (5, 7), (11, 13), True, "lean"), (LINEAR, (9, 12), (9, 12), True, "lean"), (LINEAR, (6, 8), (24, 32), True, "up4"),
    (LINEAR, (5, 7), (10, 14), False, "up2"),
]
# every type and both antialias settings at the mixed shapes: antialiasing widens LINEAR's radius beyond 2, CUBIC's is 4 on a down-sampled axis
MIXED_CASES = [(code, hw_in, hw_out, aa, "cubic_slow" if code == CUBIC else "linear_slow" if aa else "linear_fast")
               for code in (LINEAR, CUBIC) for aa in (True, False) for hw_in, hw_out in MIXED]
LEAN_SHAPES = [((9, 12), (9, 12)), ((17, 23), (33, 70)), ((3, 200), (4, 256)), ((24, 48), (40, 130)), ((1, 1), (5, 9)), ((7, 4), (7, 4))]
EDGE_ONLY = ((7, 50), (21, 10))
UP_SHAPES = [(2, 3, 5, 7), (1, 2, 17, 20), (1, 1, 1, 1)]


PPT_CASES = [(code, shp, nc) for code, shp in ((NEAREST, ((3, 4), (5, 7))), (CUBIC, ((3, 4), (5, 7))), (LINEAR, ((5, 7), (3, 4))))
             for nc in (4099, 8195, 16389)]
UP_PPT_CASES = [(16391, 2), (32773, 4)]
SLICE_CASES = [(NEAREST, (5, 7), (11, 13), True, "nearest"), (CUBIC, (5, 7), (11, 13), True, "cubic_fast"), (CUBIC, (12, 16), (7, 9), True, "cubic_slow"),
               (LINEAR, (12, 16), (7, 9), False, "linear_fast"), (LINEAR, (12, 16), (7, 9), True, "linear_slow"), (LINEAR, (17, 23), (33, 70), True, "lean")]
SLICE_SCALES = (20.0, 0.05)                           # in_scale, out2_scale


def ppt_input(NC, Hin, Win):
    x = rand((1, NC, Hin, Win), 17)
    x[0, NC - 1, 0, 0] = np.nan
    return x


def up_ppt_input(NC):
    x = rand((1, NC, 8, 8), 18)
    x[0, NC - 1, 7, 7] = np.inf
    return x


def case_id(c):
    code, (hi, wi), (ho, wo), aa, branch = c
    return f"{KIND[code]}-{hi}x{wi}-{ho}x{wo}-{'aa' if aa else 'noaa'}-{branch}"


def poisoned(x):
    x = x.copy()
    N, C, H, W = x.shape
    x[0, min(1, C - 1), H // 2, W // 3] = np.nan
    x[-1, -1, H - 1, W - 1] = np.inf
    x[-1, 0, 0, 0] = -np.inf
    return x


# ---- CPU: the statement, the teeth of the bounds, the oracle -------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["linear", "cubic"])
@pytest.mark.parametrize("shape", [((6, 8), (24, 32)), ((16, 20), (8, 10)), ((9, 12), (9, 12)), ((12, 16), (7, 9))])
def test_statement_equals_the_fp64_derivation(kind, shape):
    """At the shapes of test_oracle.py the statement is ref_torch64.resample (an independent loop with fp64 positions): bit for bit
    where the ratios are dyadic (no position rounds), to 1e-6 at (12,16)->(7,9), wherever both pick the same window centre --
    which is at least 95 % of the outputs."""
    (Hin, Win), (Hout, Wout) = shape
    x = rand((2, 2, Hin, Win), 15)
    old = R.resample(x.astype(np.float64), Hout, Wout, kind, True)
    st = R.resample_statement(x, Hout, Wout, kind, True)
    g = st["geometry"]
    same = ((st["yr"] == R._roundf(np.arange(Hout) * float(g["fy"]) + float(g["fx"]) / 2 - 0.5))[:, None]
            & (st["xr"] == R._roundf(np.arange(Wout) * float(g["fx"]) + float(g["fy"]) / 2 - 0.5))[None])
    assert same.mean() >= 0.95
    sel = np.broadcast_to(same, old.shape)
    if shape == ((12, 16), (7, 9)):
        np.testing.assert_allclose(st["ref"][sel], old[sel], rtol=0, atol=1e-6)
    else:
        assert same.all()
        np.testing.assert_allclose(st["ref"], old, rtol=1e-12, atol=1e-12)
    assert (st["A"] >= np.abs(st["ref"]) * np.abs(st["ws"]) * (1 - 1e-12)).all() and (st["Aw"] >= np.abs(st["ws"]) * (1 - 1e-12)).all()
    assert st["m"].max() <= (2 * g["rx"] + 1) * (2 * g["ry"] + 1)


def test_nearest_statement_is_the_old_one():
    for (Hin, Win), (Hout, Wout) in NEAREST_SHAPES:
        x = rand((1, 2, Hin, Win), 16)
        g = R.resample_geometry(Hin, Win, Hout, Wout)
        pos = R.resample_positions(Wout, g["fx"], g["fy"]).astype(np.float64)
        if ((Hin, Win), (Hout, Wout)) == ((8, 12), (4, 6)):
            assert (pos % 1 == 0.5).all()                         # x_in = 2x + 0.5: roundf goes away from zero, rint would not
            assert np.array_equal(R._roundf(pos), 2 * np.arange(Wout) + 1)
        new = R.resample_nearest(x, Hout, Wout)
        assert np.array_equal(bits(new), bits(oracle.resample_forward(x, Hout, Wout, NEAREST)))
        if max(g["fx"], g["fy"]) / min(g["fx"], g["fy"]) < 1.5:   # the old loop forms positions in fp64; isotropic shapes agree
            assert np.array_equal(new, R.resample(x.astype(np.float64), Hout, Wout, "nearest").astype(np.float32))


@pytest.mark.parametrize("case", INTERP_CASES + MIXED_CASES, ids=case_id)
def test_oracle_within_the_bounds(case):
    code, (Hin, Win), (Hout, Wout), aa, branch = case
    assert resample_plan(6, Hin, Win, Hout, Wout, code, aa)[0] == branch
    x = rand((2, 3, Hin, Win), 15)
    check(oracle.resample_forward(x, Hout, Wout, code, aa), x, Hout, Wout, code, aa, "oracle " + case_id(case))
    xs = np.float32(20.0)
    check(oracle.resample_forward(x * xs, Hout, Wout, code, aa), x, Hout, Wout, code, aa, "oracle scaled " + case_id(case), in_scale=20.0)


@pytest.mark.parametrize("shape", LEAN_SHAPES)
def test_oracle_within_the_bounds_lean_shapes(shape):
    (Hin, Win), (Hout, Wout) = shape
    assert resample_plan(6, Hin, Win, Hout, Wout, LINEAR, True)[0] == "lean"
    for x in (rand((2, 3, Hin, Win), 93), poisoned(rand((2, 3, Hin, Win), 93))):
        check(oracle.resample_forward(x, Hout, Wout, LINEAR, True), x, Hout, Wout, LINEAR, True, f"oracle lean {shape}")


@pytest.mark.parametrize("F", [2, 4])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_oracle_within_the_bounds_integer_upsampling(F, shape):
    N, C, H, W = shape
    x = poisoned(rand(shape, 91)) if H * W >= 12 else rand(shape, 91)
    check(oracle.resample_forward(x, F * H, F * W, LINEAR, True), x, F * H, F * W, LINEAR, True, f"oracle up{F} {shape}")
    check(oracle.resample_forward(x * np.float32(20.0), F * H, F * W, LINEAR, True), x, F * H, F * W, LINEAR, True, f"oracle up{F} scaled {shape}",
          in_scale=20.0)


@pytest.mark.parametrize("code", [LINEAR, CUBIC])
@pytest.mark.parametrize("aa", [True, False])
def test_oracle_on_the_support_edge_case(code, aa):
    (Hin, Win), (Hout, Wout) = EDGE_ONLY
    x = rand((2, 3, Hin, Win), 15)
    st = R.resample_statement(x, Hout, Wout, KIND[code], aa)
    zero, ill, _ = classify(st, code)
    out = oracle.resample_forward(x, Hout, Wout, code, aa)
    check_ill(out, st, np.ones_like(ill), code, f"oracle edge case {KIND[code]} aa={aa}")
    check(out, x, Hout, Wout, code, aa, f"oracle edge case {KIND[code]} aa={aa}", st=st)
    old = R.resample(x.astype(np.float64), Hout, Wout, KIND[code], aa)
    if code == LINEAR and aa:                                     # fp64 positions put these taps outside the support: the O(1) difference
        assert np.abs(old - st["ref"]).max() > 0.5


# per mixed case, in the order of MIXED_CASES: (outputs with an empty window, outputs with taps but wsum == 0) per plane
MIXED_ZEROS = [(16, 8), (16, 8), (0, 208), (0, 208), (0, 110), (16, 8), (16, 8), (0, 48), (0, 48), (0, 55),
               (0, 16), (0, 16), (0, 208), (0, 208), (0, 55), (0, 16), (0, 16), (0, 24), (0, 24), (0, 22)]


def zero_counts(case):
    code, (Hin, Win), (Hout, Wout), aa, _ = case
    st = R.resample_statement(rand((1, 1, Hin, Win), 15), Hout, Wout, KIND[code], aa)
    zero, _, _ = classify(st, code)
    return int((st["taps"] == 0).sum()), int((zero & (st["taps"] > 0)).sum())


def test_mixed_shapes_reach_the_zero_branch():
    """Row 8 of the table: the empty window and the wsum == 0 branch are present in every mixed case (counted from the statement;
    check() asserts that each of these outputs is exactly +0.0)."""
    assert [zero_counts(c) for c in MIXED_CASES] == MIXED_ZEROS
    assert all(e + z > 0 for e, z in MIXED_ZEROS) and sum(e for e, _ in MIXED_ZEROS) > 0


def _teeth_case():
    (Hin, Win), (Hout, Wout) = (8, 32), (32, 8)
    x = rand((2, 3, Hin, Win), 15)
    return x, Hout, Wout, oracle.resample_forward(x, Hout, Wout, LINEAR, True)


def test_bound_notices_unswapped_offsets(monkeypatch):
    x, Hout, Wout, out = _teeth_case()
    check(out, x, Hout, Wout, LINEAR, True, "swapped")
    positions = R.resample_positions
    monkeypatch.setattr(R, "resample_positions", lambda n, f_own, f_other: positions(n, f_own, f_own))     # x uses fx / 2, y uses fy / 2
    wrong = R.resample_statement(x, Hout, Wout, "linear", True)
    monkeypatch.undo()
    with pytest.raises(AssertionError, match="over the bound|exactly"):
        check(out, x, Hout, Wout, LINEAR, True, "unswapped", st=wrong, cap=None)


@pytest.mark.parametrize("shift", [(0, 1), (1, 0), (0, -1)])
def test_bound_notices_a_window_shifted_by_one_tap(shift):
    """The statement of the image moved by one tap is the statement with every window one tap over."""
    for code, (Hin, Win), (Hout, Wout), aa in ((LINEAR, (16, 20), (8, 10), True), (CUBIC, (6, 8), (24, 32), True)):
        x = rand((2, 3, Hin, Win), 15)
        out = oracle.resample_forward(x, Hout, Wout, code, aa)
        check(out, x, Hout, Wout, code, aa, "unshifted")
        wrong = R.resample_statement(np.roll(x, shift, axis=(2, 3)), Hout, Wout, KIND[code], aa)
        with pytest.raises(AssertionError, match="over the bound"):
            check(out, x, Hout, Wout, code, aa, "shifted", st=wrong, cap=None)


@pytest.mark.parametrize("case", [INTERP_CASES[0], INTERP_CASES[1], INTERP_CASES[7], INTERP_CASES[13], INTERP_CASES[15]], ids=case_id)
def test_bound_notices_one_element_moved_by_32_units(case):
    code, (Hin, Win), (Hout, Wout), aa, _ = case
    x = rand((2, 3, Hin, Win), 15)
    out = oracle.resample_forward(x, Hout, Wout, code, aa)
    st = R.resample_statement(x, Hout, Wout, KIND[code], aa)
    b, zero, ill, well = bound_of(st, code)
    cand = np.argwhere(well[1, 2])
    y, xx = cand[len(cand) // 2]
    unit = U * (st["A"][1, 2, y, xx] + abs(st["ref"][1, 2, y, xx]) * st["Aw"][y, xx]) / abs(st["ws"][y, xx])
    assert b[1, 2, y, xx] < 31 * unit                            # (m + c < 31, CUBIC's absolute term included: the cases are chosen so)
    moved = out.copy()
    moved[1, 2, y, xx] = np.float32(st["ref"][1, 2, y, xx] + 32 * unit)
    check(out, x, Hout, Wout, code, aa, "not moved", st=st)
    with pytest.raises(AssertionError, match="over the bound"):
        check(moved, x, Hout, Wout, code, aa, "moved", st=st)


@pytest.mark.parametrize("code,shape,NC", PPT_CASES)
def test_oracle_within_the_bounds_planes_per_thread_shapes(code, shape, NC):
    (Hin, Win), (Hout, Wout) = shape
    x = ppt_input(NC, Hin, Win)
    out = oracle.resample_forward(x, Hout, Wout, code, True)
    if code == NEAREST:
        assert np.array_equal(bits(out), bits(R.resample_nearest(x, Hout, Wout)))
    else:
        check(out, x, Hout, Wout, code, True, f"oracle {KIND[code]} {NC} planes")


@pytest.mark.parametrize("NC,ppt", UP_PPT_CASES)
def test_oracle_within_the_bounds_planes_per_thread_integer_upsampling(NC, ppt):
    x = up_ppt_input(NC)
    check(oracle.resample_forward(x, 16, 16, LINEAR, True), x, 16, 16, LINEAR, True, f"oracle up2 {NC} planes")


@pytest.mark.parametrize("case", SLICE_CASES, ids=lambda c: c[4])
def test_oracle_within_the_bounds_slice_shapes(case):
    code, (Hin, Win), (Hout, Wout), aa, branch = case
    x = rand((2, 3, Hin, Win), 320, 2.0)
    out = oracle.resample_forward(x * np.float32(SLICE_SCALES[0]), Hout, Wout, code, aa)
    if code == NEAREST:
        assert np.array_equal(bits(out), bits(R.resample_nearest(x, Hout, Wout, in_scale=SLICE_SCALES[0])))
    else:
        check(out, x, Hout, Wout, code, aa, f"oracle slices {branch}", in_scale=SLICE_SCALES[0])


def test_plan_reaches_every_planes_per_thread_value():
    assert resample_plan(4099, 3, 4, 5, 7, NEAREST, True) == ("nearest", 2)
    assert resample_plan(8195, 3, 4, 5, 7, CUBIC, True) == ("cubic_fast", 4)
    assert resample_plan(16389, 5, 7, 3, 4, LINEAR, True) == ("linear_slow", 8)
    assert resample_plan(16391, 8, 8, 16, 16, LINEAR, True) == ("up2", 2) and resample_plan(32773, 8, 8, 16, 16, LINEAR, True) == ("up2", 4)
    assert resample_plan(524281, 1, 1, 1, 1, NEAREST, True)[0] == "refused" and resample_plan(524280, 1, 1, 1, 1, NEAREST, True) == ("nearest", 8)
    assert resample_plan(262145, 1, 1, 2, 2, LINEAR, True)[0] == "refused" and resample_plan(131071, 1, 1, 1, 1, LINEAR, True)[0] == "refused"
    assert resample_plan(131070, 1, 1, 1, 1, LINEAR, True) == ("lean", 2)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", NEAREST_SHAPES)
def test_nearest(shape):
    (Hin, Win), (Hout, Wout) = shape
    x = poisoned(rand((2, 3, Hin, Win), 15))
    assert resample_plan(6, Hin, Win, Hout, Wout, NEAREST, True) == ("nearest", 1)
    for aa in (True, False):
        same_bits(gpu_resample(x, Hout, Wout, NEAREST, aa), R.resample_nearest(x, Hout, Wout), f"nearest {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", INTERP_CASES + MIXED_CASES, ids=case_id)
def test_interp_branches(case):
    code, (Hin, Win), (Hout, Wout), aa, branch = case
    assert resample_plan(6, Hin, Win, Hout, Wout, code, aa) == (branch, 2 if branch == "lean" else 1)
    if case in MIXED_CASES:
        assert zero_counts(case) == MIXED_ZEROS[MIXED_CASES.index(case)]
    for name, x in (("", rand((2, 3, Hin, Win), 15)), (" poisoned", poisoned(rand((2, 3, Hin, Win), 15)))):
        out = gpu_resample(x, Hout, Wout, code, aa)
        check(out, x, Hout, Wout, code, aa, case_id(case) + name)
        if branch in ("lean", "up2", "up4"):
            same_bits(out, gpu_resample(x, Hout, Wout, code, aa, generic=True), case_id(case) + name + " vs the per-pixel kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("code", [LINEAR, CUBIC])
@pytest.mark.parametrize("aa", [True, False])
def test_support_edge_case(code, aa):
    """(7,50)->(21,10): a third of the rows sit on the support edge (see the docstring): the bounds, the ill-conditioned assertions on
    every output, and the debug hook changes no bit (neither the lean nor the up kernel takes this shape)."""
    (Hin, Win), (Hout, Wout) = EDGE_ONLY
    x = rand((2, 3, Hin, Win), 15)
    st = R.resample_statement(x, Hout, Wout, KIND[code], aa)
    out = gpu_resample(x, Hout, Wout, code, aa)
    check_ill(out, st, np.ones(st["ws"].shape, bool), code, f"edge case {KIND[code]} aa={aa}")
    check(out, x, Hout, Wout, code, aa, f"edge case {KIND[code]} aa={aa}", st=st)
    same_bits(out, gpu_resample(x, Hout, Wout, code, aa, generic=True), "edge case, hook")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LEAN_SHAPES)
@pytest.mark.parametrize("poison", [False, True])
def test_lean_variants(shape, poison):
    """16-byte scan (Win % 4 == 0) and scalar scan, finite and poisoned footprints, several ragged tiles; and a bottom whose storage
    offset breaks the 16-byte alignment (scalar scan although Win % 4 == 0): the same bits."""
    (Hin, Win), (Hout, Wout) = shape
    x = rand((2, 3, Hin, Win), 93)
    x = poisoned(x) if poison else x
    assert resample_plan(6, Hin, Win, Hout, Wout, LINEAR, True) == ("lean", 2)
    out = gpu_resample(x, Hout, Wout, LINEAR, True)
    check(out, x, Hout, Wout, LINEAR, True, f"lean {shape} poison={poison}")
    same_bits(out, gpu_resample(x, Hout, Wout, LINEAR, True, generic=True), "lean vs the per-pixel kernel")
    buf = torch.zeros(x.size + 4, device="cuda")
    off = buf[1:1 + x.size].view(x.shape)
    off.copy_(dev(x))
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    same_bits(out, gpu_resample(off, Hout, Wout, LINEAR, True), "lean with a misaligned bottom")


@pytest.mark.gpu
@pytest.mark.parametrize("F", [2, 4])
@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_integer_upsampling(F, extra, shape):
    N, C, H, W = shape
    x = poisoned(rand(shape, 91)) if H * W >= 12 else rand(shape, 91)
    Ho, Wo = F * H, F * W
    assert resample_plan(N * C, H, W, Ho, Wo, LINEAR, True) == (f"up{F}", 1)
    assert resample_plan(N * C, H, W, Ho, Wo, LINEAR, True, aligned_top=False) == ("lean", 2)
    s_in, s_out = (20.0, 0.05) if extra else (1.0, 1.0)
    tops = {}
    for aligned in (True, False):
        n = N * (C + 2) * Ho * Wo
        buf = torch.full((n + 4,), -9.0, device="cuda")
        blob = (buf[:n] if aligned else buf[1:1 + n]).view(N, C + 2, Ho, Wo)
        assert blob.data_ptr() % 16 == (0 if aligned else 4)
        blob2 = torch.full((N, C + 1, Ho, Wo), -9.0, device="cuda")
        if extra:
            ops.resample_forward_slices(dev(x), Ho, Wo, LINEAR, True, s_in, out=(blob, 1, C), out2=(blob2, 0, C), out2_scale=s_out)
            out, out2 = host(blob[:, 1:1 + C]), host(blob2[:, :C])
            same_bits(out2, out * np.float32(s_out), "second top")
            assert float(blob[:, 0].max()) == -9.0 and float(blob[:, C + 1].max()) == -9.0 and float(blob2[:, C].max()) == -9.0
        elif aligned:
            out = gpu_resample(x, Ho, Wo, LINEAR, True)
        else:
            full = (buf[1:1 + N * C * Ho * Wo]).view(N, C, Ho, Wo)
            ops.resample_forward_slices(dev(x), Ho, Wo, LINEAR, True, out=full)
            out = host(full)
        tops[aligned] = out
        check(out, x, Ho, Wo, LINEAR, True, f"up{F} extra={extra} aligned={aligned} {shape}", in_scale=s_in)
    same_bits(tops[True], tops[False], "a misaligned top falls to the lean kernel with the same bits")
    xs = dev(x) * np.float32(s_in) if extra else dev(x)
    same_bits(tops[True], gpu_resample(xs.contiguous(), Ho, Wo, LINEAR, True, generic=True), "up vs the per-pixel kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("code,shape,NC", PPT_CASES)
def test_planes_per_thread(code, shape, NC):
    (Hin, Win), (Hout, Wout) = shape
    branch, ppt = resample_plan(NC, Hin, Win, Hout, Wout, code, True)
    assert branch == {NEAREST: "nearest", CUBIC: "cubic_fast", LINEAR: "linear_slow"}[code] and ppt == {4099: 2, 8195: 4, 16389: 8}[NC]
    assert NC % ppt != 0                                           # a ragged last group
    x = ppt_input(NC, Hin, Win)
    out = gpu_resample(x, Hout, Wout, code, True)
    if code == NEAREST:
        same_bits(out, R.resample_nearest(x, Hout, Wout), f"nearest ppt={ppt}")
    else:
        check(out, x, Hout, Wout, code, True, f"{branch} ppt={ppt}")


@pytest.mark.gpu
@pytest.mark.parametrize("NC,ppt", UP_PPT_CASES)
def test_planes_per_thread_integer_upsampling(NC, ppt):
    assert resample_plan(NC, 8, 8, 16, 16, LINEAR, True) == ("up2", ppt) and NC % ppt != 0
    x = up_ppt_input(NC)
    out = gpu_resample(x, 16, 16, LINEAR, True)
    check(out, x, 16, 16, LINEAR, True, f"up2 ppt={ppt}")


@pytest.mark.gpu
@pytest.mark.parametrize("NC,code,hw_out", [(524281, NEAREST, (1, 1)), (262145, LINEAR, (2, 2)), (131071, LINEAR, (1, 1))])
def test_too_many_planes_is_refused_and_writes_nothing(NC, code, hw_out):
    import flownet2_amd
    assert resample_plan(NC, 1, 1, hw_out[0], hw_out[1], code, True)[0] == "refused"
    x = torch.ones((1, NC, 1, 1), device="cuda")
    top = torch.full((1, NC) + hw_out, -9.0, device="cuda")
    with pytest.raises(flownet2_amd.Fn2Error) as e:
        ops.resample_forward_slices(x, hw_out[0], hw_out[1], code, True, out=top)
    assert e.value.status == FN2_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((top == -9.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", SLICE_CASES, ids=lambda c: c[4])
def test_slices(case):
    """in_scale != 1, a top slice of a wider blob and a second top (the EXTRA instantiation of every family; up2 / up4: above)."""
    code, (Hin, Win), (Hout, Wout), aa, branch = case
    N, C = 2, 3
    assert resample_plan(N * C, Hin, Win, Hout, Wout, code, aa)[0] == branch
    x = rand((N, C, Hin, Win), 320, 2.0)
    s_in, s_out = SLICE_SCALES
    blob, blob2 = torch.full((N, C + 3, Hout, Wout), -9.0, device="cuda"), torch.full((N, C + 1, Hout, Wout), -9.0, device="cuda")
    ops.resample_forward_slices(dev(x), Hout, Wout, code, aa, s_in, out=(blob, 2, C), out2=(blob2, 0, C), out2_scale=s_out)
    out, out2 = host(blob[:, 2:2 + C]), host(blob2[:, :C])
    if code == NEAREST:
        same_bits(out, R.resample_nearest(x, Hout, Wout, in_scale=s_in), "nearest slices")
    else:
        check(out, x, Hout, Wout, code, aa, f"slices {branch}", in_scale=s_in)
    same_bits(out2, out * np.float32(s_out), "second top")
    assert float(blob[:, :2].max()) == -9.0 and float(blob[:, 2 + C:].max()) == -9.0 and float(blob2[:, C:].max()) == -9.0
