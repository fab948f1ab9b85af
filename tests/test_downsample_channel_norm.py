"""Downsample and ChannelNorm (csrc/channel_norm.hip) against their fp64 statements (ref_torch64.downsample_statement,
channel_norm_statement, channel_norm_backward_statement), on every launch branch of the host functions.

Downsample.  botx, boty, widthScale, heightScale and the radii are fp32 as in down_plan / downsample_thread_body; weights and sums
are fp64.  Per output: ref, A = sum |s| w / W, the valid weight W, the NaN weight Wn and the vote ratio r = Wn / W.  u = 2^-24.
  * value:  |hip - ref| <= (d + c) u (A + |ref|),  c = 8.
      d is the longest chain of additions of the decomposition that runs (down_chain below, from the documented layout): the clipped tap
      count for the thread form; column passes x rows per thread + 6 butterfly steps (+ 3 wave partials) for the wave / workgroup forms.
      Each product s * (wx * wy) carries the rounding of wx * wy (u) and the fused multiply-add is the chain's step; accum_value and
      accum_weight are both chains: (d + 1) u on each; the division adds u |ref|: (d + 2) u (A + |ref|), and 2u for second order.
      What is not relative to a weight -- fl(tap - bot), the division by the scale and the cancellation in 1 - q move w by up to 2u q
      whatever its size -- is measured exactly (the statement forms the fp32 weight too: Ae = sum |w32 - w| |s| / W, Ee = sum |w32 - w| / W)
      and has 4u inside c: the host asserts Ae + |ref| Ee <= 4u (A + |ref|) for every bounded output.
  * vote:   NaN (bits 0x7fffffff) exactly where r > 0.5, strict, over the valid weight only.  An output whose r lies within
      (d + c) u (1 + r) of 0.5 may go either way; every case asserts on the host that it holds no such output.  At the three
      forms' smallest windows (scales 4, 8, 32: dyadic weights, every sum exact in fp32 in any order) NaN is planted so that chosen
      outputs vote exactly 0.5 (finite), one weight step above (NaN) and below (finite), and see an all-NaN window (W = 0, r = inf: NaN).
      A tie needs Wn = (Wn + W) / 3: the window's total weight, in units of the smallest weight, must be a multiple of 3.  At scale 4
      ((17,17)->(5,5): totals 16, 10, 6.25) that never holds, so the thread form's tie is planted at (33,9)->(5,5) (scales 8 x 2).
  * NaN patterns equal (outside the either-way band), nothing non-finite where the statement is finite.
  The grid-stride cases use the smallest planes that still select each form: (33,33)->(5,5) for the wave form and (33,33)->(2,2)
  (scale 32, a 65 x 65 window clipped to the plane) for the workgroup form.
  Branches (down_plan below restates the selection): thread (< 256 taps, or a window taller than the 1025-row table), wave (256 ..
  4095 taps), workgroup (>= 4096); their grid-stride loops (N C > 65535; > 4 x 65536 outputs; > 65536 outputs); a window wider than a
  wave (several column passes); the pyramid launch with all three forms in one grid, bitwise the single launches.

ChannelNorm.
  * forward  sqrt(sum_c v^2), v the fp32 difference for the `minus` form:  |hip - ref| <= (C + 2) u ref.
      C fused multiply-adds: the sum of squares is off by at most C u (relative: all terms are >= 0), the square root halves that and
      adds its own u: (C / 2 + 1) u, second order included in (C + 2) u.
  * backward (g x) / (top + 1e-9) with g x rounded to fp32 first, the quotient formed in double:  |hip - ref| <= 3u |ref|
      (one rounding to fp32, u |ref|; the double arithmetic is far below that; no case here has a denormal quotient).
  * all-zero input: forward exactly +0.0; backward a zero with the sign of g * 0 (the reference's own expression gives -0.0 for g < 0).
  Branches: the grid-stride loops over N (forward, N > 65535) and N C (backward, N C > 65535); pixel blocks with a ragged tail
  (hw = 1, 255, 256, 257); the folded subtraction and channel slices.

Worst error / bound on the MI355X (this file's printed ratios): Downsample thread form 0.088, wave form 0.065, workgroup form 0.017
(d is a worst-case chain; rounding errors do not line up); ChannelNorm forward 0.45, backward 0.33.
Tests marked gpu need the MI355X; the others check the statements, the teeth of the bounds and the C oracle on the CPU.
"""
import numpy as np
import pytest
import torch

import oracle
import ref_torch64 as R
from flownet2_amd import ops

U = 2.0 ** -24
C_DOWN = 8
NAN_BITS = 0x7FFFFFFF
DOWN_MAX_ROWS = 2 * 512 + 1                           # kDownMaxRows, channel_norm.hip


def rand(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bounded(got, ref, bound, what):
    """Elementwise |got - ref| <= bound where ref is finite; equal NaN patterns; identical infinities.  Returns the worst ratio."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN pattern differs at {np.argwhere(gn != rn)[:5].tolist()}"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{what}: infinities differ"
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all(), f"{what}: non-finite value where the fp64 statement is finite"
    err, b = np.abs(got[fin] - ref[fin]), bound[fin]
    bad = err > b
    if bad.any():
        i = int(np.argmax(np.where(bad, err - b, -np.inf)))
        raise AssertionError(f"{what}: {int(bad.sum())} elements over the bound; at {np.argwhere(fin)[i].tolist()}: "
                             f"|{got[fin][i]!r} - {ref[fin][i]!r}| = {err[i]:.3e} > {b[i]:.3e}")
    return float((err / np.where(b > 0, b, 1)).max()) if err.size else 0.0


# ---- Downsample: plan, chain length, the check ---------------------------------------------------------------------------------------

def down_plan(NC, Hin, Win, Hout, Wout, wave_taps=256):
    """(form, grid-stride?) as down_plan in channel_norm.hip: 0 thread, 1 wave, 2 workgroup per output element."""
    g = R.downsample_geometry(Hin, Win, Hout, Wout)
    taps, outs = (2 * g["wr"] + 1) * (2 * g["hr"] + 1), NC * Hout * Wout
    fits = 2 * g["hr"] + 1 <= DOWN_MAX_ROWS
    if taps >= 4096 and fits:
        return 2, outs > 65536
    if taps >= wave_taps and fits:
        return 1, (outs + 3) // 4 > 65536
    return 0, NC > 65535


def down_chain(form, Hin, Win, Hout, Wout):
    """[Hout,Wout]: the longest chain of additions behind an output in the decomposition `form`."""
    g = R.downsample_geometry(Hin, Win, Hout, Wout)
    nx, ny = (g["x1"] - g["x0"] + 1)[None], (g["y1"] - g["y0"] + 1)[:, None]
    if form == 0:
        return nx * ny
    G = 64 if form == 1 else 256
    cw = np.minimum(2 ** np.ceil(np.log2(nx)).astype(np.int64), G)             # column slots: the power of two >= nx, at most the group
    rows_per_thread = -(-ny // (G // cw))
    passes = -(-nx // cw)
    return passes * rows_per_thread + 6 + (3 if form == 2 else 0)


def check_down(out, x, Hout, Wout, what, form=None, st=None, exact=False):
    """Every Downsample assertion of the docstring on one output blob.  Returns (worst value ratio, statement)."""
    out = np.asarray(out, np.float32)
    N, C, Hin, Win = x.shape
    form = down_plan(N * C, Hin, Win, Hout, Wout)[0] if form is None else form
    st = st if st is not None else R.downsample_statement(x, Hout, Wout)
    d = down_chain(form, Hin, Win, Hout, Wout)[None, None]
    ref, r, W = st["ref"], st["r"], st["W"]
    assert ((st["Wn"] > 0) | (W > 0)).all()                      # no 0 / 0 vote: some tap of every window carries weight
    allnan = W == 0
    with np.errstate(invalid="ignore"):
        band = (np.abs(r - 0.5) <= (d + C_DOWN) * U * (1 + r)) & ~allnan      # (r = inf for an all-NaN window: no near-tie)
    if exact:                                                    # dyadic weights, sums below 2^24 units: fp32 votes as fp64 does
        assert not st["Ee"][W > 0].any()
        band = np.zeros_like(band)
    assert not band.any(), f"{what}: {int(band.sum())} outputs vote within the either-way band: pick another seed"
    voted = st["voted"] & ~band
    assert (bits(out[voted & ~allnan]) == NAN_BITS).all(), f"{what}: a NaN vote that is not 0x7fffffff"
    assert np.isnan(out[allnan]).all(), f"{what}: an all-NaN window that is not NaN"
    keep = ~st["voted"] & ~band
    A, aref = st["A"][keep], np.abs(ref[keep])
    assert (st["Ae"][keep] + aref * st["Ee"][keep] <= 4 * U * (A + aref)).all(), f"{what}: the weights' absolute error exceeds its 4u"
    ratio = bounded(out[keep], ref[keep], (np.broadcast_to(d, ref.shape)[keep] + C_DOWN) * U * (A + aref), what)
    print(f"downsample ratio {what}: {ratio:.3g}  (form {form}, d <= {int(d.max())}, NaN {int(st['voted'].sum())} of {ref.size})")
    return ratio, st


def nan_mask(x, seed, frac=0.33):
    x = x.copy()
    x[np.random.default_rng(seed).random(x.shape) < frac] = np.nan
    return x


def planted_votes(Hin, Win, Hout, Wout, seed):
    """x [1,4,Hin,Win] for a shape with exact weights, and the planted output (dy, dx): plane 0 votes exactly 0.5 there if the
    window's total weight allows a tie (else it is left alone), plane 1 one weight step above 0.5, plane 2 the nearest step below,
    plane 3 sees an all-NaN window.  Returns (x, (dy, dx), tie possible?)."""
    g, wy, wx, ey, ex = R.downsample_weights(Hin, Win, Hout, Wout)
    assert not ey.any() and not ex.any()                          # fp32 weights are the fp64 ones: dyadic scales
    unit = 1.0 / (float(g["ws"]) * float(g["hs"]))
    best = None
    for dy in range(Hout):
        for dx in range(Wout):
            T = wy[dy].sum() * wx[dx].sum() / unit
            assert T == round(T)
            if best is None or (round(T) % 3 == 0 and not best[2]):
                best = (dy, dx, round(T) % 3 == 0, int(round(T)))
    dy, dx, tie, T = best
    w = np.round(np.outer(wy[dy], wx[dx]) / unit).astype(np.int64)          # the window's weights in units of the smallest one
    assert (w == np.outer(wy[dy], wx[dx]) / unit).all() and w.sum() == T and T < 2 ** 24

    def subset(target):                                          # taps whose weights add up to `target`: greedy, largest first
        pick, left = np.zeros_like(w, bool), target
        for i in np.argsort(-w, axis=None, kind="stable"):
            y, xx = divmod(int(i), w.shape[1])
            if 0 < w[y, xx] <= left:
                pick[y, xx], left = True, left - w[y, xx]
        assert left == 0 and w[pick].sum() == target
        return pick

    x = rand((1, 4, Hin, Win), seed)
    if tie:
        x[0, 0][subset(T // 3)] = np.nan
    x[0, 1][subset(T // 3 + 1)] = np.nan
    x[0, 2][subset(-(-T // 3) - 1)] = np.nan
    x[0, 3][w > 0] = np.nan
    return x, (dy, dx), tie


def check_planted(out, x, Hout, Wout, where, tie, what, form=None):
    _, st = check_down(out, x, Hout, Wout, what, form=form, exact=True)
    dy, dx = where
    r = st["r"][0, :, dy, dx]
    assert (not tie or r[0] == 0.5) and r[1] > 0.5 and r[2] < 0.5 and np.isinf(r[3])
    unit = 1.0 / (float(st["geometry"]["ws"]) * float(st["geometry"]["hs"]))
    Wn = st["Wn"][0, :, dy, dx] / unit
    assert Wn[1] - Wn[2] <= 2                                    # the smallest weight steps on either side of the threshold
    got = np.asarray(out)[0, :, dy, dx]
    if tie:
        assert np.isfinite(got[0]), f"{what}: a vote of exactly 0.5 must not give NaN"
    assert bits(got[1]) == NAN_BITS and np.isfinite(got[2]) and np.isnan(got[3]), what


FORM_SHAPES = [((17, 17), (5, 5), 0), ((33, 9), (5, 5), 0), ((33, 33), (5, 5), 1), ((129, 129), (5, 5), 2)]
RANDOM_SHAPES = [((17, 17), (5, 5), 0), ((33, 33), (5, 5), 1), ((129, 129), (5, 5), 2), ((23, 31), (6, 7), 0), ((40, 56), (10, 14), 0),
                 ((64, 96), (7, 9), 1), ((12, 1200), (9, 20), 1), ((1300, 9), (2, 5), 0), ((97, 130), (3, 4), 2)]
PYRAMID = ((2, 2, 129, 129), [(33, 33), (5, 5), (17, 17)], [0, 2, 1], 41)      # bottom, tops, their forms, mask seed
MASK_SEED = {((1300, 9), (2, 5)): 32}                # seeds for which no vote falls into the either-way band (asserted); default 31


def test_down_plan_and_chain():
    assert [down_plan(4, *a, *b)[0] for a, b, _ in FORM_SHAPES] == [f for _, _, f in FORM_SHAPES]
    assert [down_plan(4, *a, *b) for a, b, _ in RANDOM_SHAPES] == [(f, False) for _, _, f in RANDOM_SHAPES]
    g = R.downsample_geometry(17, 17, 5, 5)
    assert (g["wr"], g["hr"]) == (4, 4) and (2 * g["wr"] + 1) * (2 * g["hr"] + 1) == 81
    g = R.downsample_geometry(129, 129, 5, 5)
    assert (2 * g["wr"] + 1) * (2 * g["hr"] + 1) == 4225
    g = R.downsample_geometry(1300, 9, 2, 5)                      # taller than the row table: the thread form despite 4096+ taps
    assert 2 * g["hr"] + 1 > DOWN_MAX_ROWS and (2 * g["wr"] + 1) * (2 * g["hr"] + 1) >= 4096
    g = R.downsample_geometry(12, 1200, 9, 20)                    # wider than a wave: three column passes
    assert (g["x1"] - g["x0"] + 1).max() == 129 and down_chain(1, 12, 1200, 9, 20).max() == 3 * 5 + 6
    assert down_chain(0, 17, 17, 5, 5).max() == 81 and down_chain(0, 17, 17, 5, 5).min() == 25
    assert down_chain(1, 33, 33, 5, 5).max() == 1 * 9 + 6         # 17 columns -> 32 slots, 2 row slots, 17 rows
    assert down_chain(2, 129, 129, 5, 5).max() == 1 * 33 + 9      # 65 columns -> 128 slots, 2 row slots, 65 rows
    assert down_plan(65537, 3, 3, 2, 2) == (0, True) and down_plan(10500, 33, 33, 5, 5) == (1, True) and down_plan(16400, 33, 33, 2, 2) == (2, True)
    assert down_plan(10485, 33, 33, 5, 5) == (1, False) and down_plan(16384, 33, 33, 2, 2) == (2, False)


@pytest.mark.parametrize("shape", [((16, 24), (4, 6)), ((17, 23), (5, 7)), ((23, 31), (6, 7))])
def test_downsample_statement_is_the_old_one(shape):
    (Hin, Win), (Hout, Wout) = shape
    x = nan_mask(rand((1, 2, Hin, Win), 20), 21)
    st = R.downsample_statement(x, Hout, Wout)
    old = R.downsample(x, Hout, Wout)
    assert np.array_equal(np.isnan(st["ref"]), np.isnan(old))
    np.testing.assert_allclose(np.nan_to_num(st["ref"]), np.nan_to_num(old), rtol=1e-12, atol=1e-12)
    assert (st["A"][~st["voted"]] >= np.abs(st["ref"][~st["voted"]]) * (1 - 1e-12)).all()
    np.testing.assert_allclose(st["W"] + st["Wn"], np.broadcast_to(st["Wt"], st["W"].shape), rtol=1e-12)


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=str)
def test_oracle_downsample_random_masks(shape):
    (Hin, Win), (Hout, Wout), _ = shape
    x = nan_mask(rand((2, 2, Hin, Win), 30, 3.0), MASK_SEED.get(shape[:2], 31))
    _, st = check_down(oracle.downsample_forward(x, Hout, Wout), x, Hout, Wout, f"oracle {shape}", form=0)       # the oracle is one thread
    assert 0.1 < st["voted"].mean() < 0.9 or Hout * Wout < 16


def test_oracle_downsample_pyramid_inputs():
    shape, sizes, forms, seed = PYRAMID
    x = nan_mask(rand(shape, 34, 3.0), seed)
    for (h, w), form, got in zip(sizes, forms, oracle.downsample_forward_multi(x, sizes)):
        check_down(got, x, h, w, f"oracle pyramid {h}x{w}", form=0)
        d = down_chain(form, 129, 129, h, w)
        st = R.downsample_statement(x, h, w)
        assert not (np.abs(st["r"] - 0.5) <= (d + C_DOWN) * U * (1 + st["r"])).any()      # nor in the band of the form the GPU runs


@pytest.mark.parametrize("shape", FORM_SHAPES, ids=str)
def test_oracle_downsample_planted_votes(shape):
    (Hin, Win), (Hout, Wout), _ = shape
    x, where, tie = planted_votes(Hin, Win, Hout, Wout, 32)
    assert tie == ((Hin, Win) != (17, 17))
    check_planted(oracle.downsample_forward(x, Hout, Wout), x, Hout, Wout, where, tie, f"oracle planted {shape}", form=0)


@pytest.mark.parametrize("vote", ["valid>=", "total>"])
def test_vote_check_notices_a_wrong_vote(vote):
    """A vote taken with >= flips the exact tie; a vote over the total weight flips the output one step above 0.5."""
    (Hin, Win), (Hout, Wout) = (33, 33), (5, 5)
    x, where, tie = planted_votes(Hin, Win, Hout, Wout, 32)
    right = R.downsample_statement(x, Hout, Wout)
    with np.errstate(invalid="ignore", divide="ignore"):
        nan = right["r"] >= 0.5 if vote == "valid>=" else right["Wn"] / right["Wt"] > 0.5
    wrong = np.where(nan, np.nan, right["value"]).astype(np.float32)
    wrong.view(np.uint32)[np.isnan(wrong)] = NAN_BITS
    plane = 0 if vote == "valid>=" else 1
    assert np.isnan(wrong[0, plane, where[0], where[1]]) != np.isnan(right["ref"][0, plane, where[0], where[1]])
    with pytest.raises(AssertionError):
        check_down(wrong, x, Hout, Wout, "wrong vote", form=0)


# ---- ChannelNorm helpers ---------------------------------------------------------------------------------------------------------------

def check_norm(top, x, what, minus=None):
    ref = R.channel_norm_statement(x, minus)
    C = x.shape[1]
    ratio = bounded(top, ref, (C + 2) * U * ref, what)
    print(f"channel_norm ratio {what}: {ratio:.3g}")
    return ref


def check_norm_backward(d, x, top, g, what):
    ref = R.channel_norm_backward_statement(x, top, g)
    ratio = bounded(d, ref, 3 * U * np.abs(ref), what)
    z = ref == 0
    assert np.array_equal(bits(np.asarray(d)[z]), bits(ref[z].astype(np.float32))), f"{what}: a zero of the wrong sign"
    print(f"channel_norm ratio {what}: {ratio:.3g}")


MINUS_SHAPES = [(2, 3, 1, 257), (1, 37, 5, 7)]
NORM_SHAPES = [(2, C, 1, hw) for C in (1, 2, 3, 37) for hw in (1, 255, 256, 257)]


def nonfinite(x, seed):
    x = x.copy()
    m = np.random.default_rng(seed).random(x.shape) < 0.15 / x.shape[1]          # about one pixel in seven sees a NaN / Inf channel
    x[m] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.random.default_rng(seed + 1).integers(0, 3, int(m.sum()))]
    return x


@pytest.mark.parametrize("shape", NORM_SHAPES, ids=str)
def test_oracle_channel_norm(shape):
    x, g = rand(shape, 40), rand((shape[0], 1) + shape[2:], 41)
    for name, xx in (("", x), (" non-finite", nonfinite(x, 42)), (" zero", np.zeros_like(x))):
        ref = check_norm(oracle.channel_norm_forward(xx), xx, f"oracle forward {shape}{name}")
        top = ref.astype(np.float32)
        check_norm_backward(oracle.channel_norm_backward(xx, top, g), xx, top, g, f"oracle backward {shape}{name}")
        if name == " zero":
            assert (bits(oracle.channel_norm_forward(xx)) == 0).all()


@pytest.mark.parametrize("shape", MINUS_SHAPES)
def test_oracle_channel_norm_minus_form(shape):
    N, C, H, W = shape
    a, b = nonfinite(rand((N, C, H, W), 43), 44), rand((N, C, H, W), 45)
    check_norm(oracle.channel_norm_forward(a - b), a, f"oracle minus form {shape}", minus=b)


def test_norm_bound_notices_a_dropped_channel():
    x = rand((2, 37, 1, 257), 40)
    with pytest.raises(AssertionError):
        check_norm(oracle.channel_norm_forward(x[:, :36]), x, "dropped channel")
    top = R.channel_norm_statement(x).astype(np.float32)
    g = rand((2, 1, 1, 257), 41)
    d = oracle.channel_norm_backward(x, top, g)
    d[1, 36, 0, 256] *= np.float32(1 + 8 * U)
    with pytest.raises(AssertionError):
        check_norm_backward(d, x, top, g, "moved by 4u")


# ---- GPU: Downsample -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", FORM_SHAPES, ids=str)
def test_downsample_planted_votes(shape):
    (Hin, Win), (Hout, Wout), form = shape
    x, where, tie = planted_votes(Hin, Win, Hout, Wout, 32)
    assert down_plan(4, Hin, Win, Hout, Wout) == (form, False)
    check_planted(host(ops.downsample_forward(dev(x), Hout, Wout)), x, Hout, Wout, where, tie, f"planted {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=str)
def test_downsample_random_masks(shape):
    (Hin, Win), (Hout, Wout), form = shape
    x = nan_mask(rand((2, 2, Hin, Win), 30, 3.0), MASK_SEED.get(shape[:2], 31))
    assert down_plan(4, Hin, Win, Hout, Wout) == (form, False)
    check_down(host(ops.downsample_forward(dev(x), Hout, Wout)), x, Hout, Wout, f"random mask {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(65537, (3, 3), (2, 2), 0), (10500, (33, 33), (5, 5), 1), (16400, (33, 33), (2, 2), 2)], ids=str)
def test_downsample_grid_stride(case):
    NC, (Hin, Win), (Hout, Wout), form = case
    assert down_plan(NC, Hin, Win, Hout, Wout) == (form, True)
    x = rand((1, NC, Hin, Win), 33)
    x[0, ::7, ::2, 1::3] = np.nan
    x[0, NC - 1] = np.nan
    x[0, NC - 1, Hin // 2, Win // 2] = 1.0
    check_down(host(ops.downsample_forward(dev(x), Hout, Wout)), x, Hout, Wout, f"grid-stride {case}")


@pytest.mark.gpu
def test_downsample_pyramid_covers_the_three_forms():
    shape, sizes, forms, seed = PYRAMID
    assert [down_plan(4, 129, 129, h, w)[0] for h, w in sizes] == forms
    x = nan_mask(rand(shape, 34, 3.0), seed)
    d = dev(x)
    for (h, w), got in zip(sizes, ops.downsample_forward_multi(d, sizes)):
        assert np.array_equal(bits(host(got)), bits(host(ops.downsample_forward(d, h, w))))
        check_down(host(got), x, h, w, f"pyramid {h}x{w}")


# ---- GPU: ChannelNorm ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=str)
def test_channel_norm(shape):
    x, g = rand(shape, 40), rand((shape[0], 1) + shape[2:], 41)
    for name, xx in (("", x), (" non-finite", nonfinite(x, 42)), (" zero", np.zeros_like(x))):
        out = host(ops.channel_norm_forward(dev(xx)))
        ref = check_norm(out, xx, f"forward {shape}{name}")
        top = ref.astype(np.float32)
        check_norm_backward(host(ops.channel_norm_backward(dev(xx), dev(top), dev(g))), xx, top, g, f"backward {shape}{name}")
        if name == " zero":
            assert (bits(out) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MINUS_SHAPES)
def test_channel_norm_minus_and_slices(shape):
    N, C, H, W = shape
    a, b = nonfinite(rand((N, C + 2, H, W), 43), 44), rand((N, C + 5, H, W), 45)
    top = torch.full((N, 4, H, W), -9.0, device="cuda")
    ops.channel_norm_forward_slices((dev(a), 1, C), minus=(dev(b), 4, C), out=(top, 2, 1))
    check_norm(host(top[:, 2:3]), a[:, 1:1 + C], f"minus form {shape}", minus=b[:, 4:4 + C])
    ops.channel_norm_forward_slices((dev(a), 1, C), out=(top, 0, 1))
    check_norm(host(top[:, 0:1]), a[:, 1:1 + C], f"slices {shape}")
    assert float(top[:, 1].max()) == -9.0 and float(top[:, 3].max()) == -9.0


@pytest.mark.gpu
def test_channel_norm_grid_stride():
    x = rand((65537, 2, 2, 2), 46)
    check_norm(host(ops.channel_norm_forward(dev(x))), x, "forward N = 65537")
    b = rand((65537, 2, 2, 2), 47)
    check_norm(host(ops.channel_norm_forward_slices(dev(x), minus=dev(b))), x, "forward minus N = 65537", minus=b)
    x, g = rand((65537, 1, 2, 2), 48), rand((65537, 1, 2, 2), 49)
    top = R.channel_norm_statement(x).astype(np.float32)
    check_norm_backward(host(ops.channel_norm_backward(dev(x), dev(top), dev(g))), x, top, g, "backward N C = 65537")
    x, g = rand((21846, 3, 2, 2), 50), rand((21846, 1, 2, 2), 51)                # N C = 65538: the plane -> sample division inside the loop
    top = R.channel_norm_statement(x).astype(np.float32)
    check_norm_backward(host(ops.channel_norm_backward(dev(x), dev(top), dev(g))), x, top, g, "backward N C = 65538, C = 3")
