"""The flow heads (csrc/flow_head.hip, csrc/flow_head_bwd.hip) and the bias / ReLU kernels (csrc/bias_act.hip) against their fp64
statements (flow_head_bounds: torch float64 on the CPU -- conv2d, conv_transpose2d, aten.convolution_backward -- and plain fp64 sums),
on every launch branch of the host functions.

Sums.  Per element |hip - ref| <= (d + c) u A, u = 2^-24, c = 2.  A is the fp64 sum of the absolute values of the element's terms (the
  same statement applied to |x|, |w|, |g|); d is the longest chain of dependent roundings of the decomposition that runs; every
  multiplication is fused into its addition (fmaf) unless said otherwise.  With `accumulate` the statement is start + gradient in fp64
  and the bound gains u |ref| (the one rounding of the final addition).  c: every partial sum of a chain is at most A (1 + d u), so the
  first-order error is d u A and all higher orders together stay below d^2 u^2 A < u A for d < 4096 (asserted for every chain): one u.
  The second u is margin for a chain counted one step short; the counts below are upper bounds already (an addition to an exact
  zero is counted as a rounding), so it is not needed by any case here and is not fitted to anything.  Nothing else is rounded: no
  operand is converted, no weight is computed.  No element is left out of any comparison.
  * pf_dgrad (predict_flow bottom gradient): one chain of 18 fmas per element.  d = 18, whatever the channels per block (cpb).
  * pf_wgrad + pf_finalize (predict_flow weight gradient): a lane walks pixels lane, lane + 64, ... of the band's rows x W pixels
      (rows = min(rb, H)): ceil(rows W / 64) fmas; the reduce-scatter (4 halving steps + 2 butterfly steps) or the butterfly of sums 16
      and 17: 6 additions; pf_finalize: lane l adds parts l, l + 64, ...: ceil(parts / 64), then 6.
      d = ceil(rows W / 64) + 6 + ceil(parts / 64) + 6, parts = N bands.
  * predict_flow bias gradient (rides in pf_wgrad): a thread adds elements tid, tid + 256, ...: ceil(rows W / 256); butterfly 6; the four
      wave sums ((a + b) + c) + d: 3; pf_finalize ceil(parts / 64) + 6.
  * predict_flow forward: a wave's chain over its c_per = ceil(C / (16 nsplit)) channels; the 16 wave partials added from + 0.0f (the
      first addition is exact): 15; the gather adds 9 nsplit values to the bias.  d = c_per + 15 + 9 nsplit.
  * uf_backward bottom gradient: 32 fmas.  d = 32.
  * uf_backward + uf_finalize weight gradient: the product b * g (1), reduce-scatter over the wave (6), the four wave sums (3),
      uf_finalize ceil(parts / 64) + 6, parts = N ceil(H W / 256).  Bias gradient: (a + b) + (c + d) of the pixel's own four top pixels
      (2, not 3: the two pairs are added side by side), then the same 6 + 3 + ceil(parts / 64) + 6.
  * upsample_flow forward (deconv4x4s2_c2): the bias and at most 2 x 2 taps x 2 channels fmas.  d = 8.
  * bias gradients of bias_act.hip.  The terms are the fp32 values the kernel sums (the bottom_diff it has just rounded, or top_diff
      itself for conv_backward_bias).  Two-launch form: a block of 256 threads takes every 8th stretch of its plane: ceil(hw / 2048) trips
      of one addition, or ceil(hw / 4 / 2048) trips of three with 16-byte loads ((g0 + g1) + (g2 + g3), then the running sum);
      butterfly 6; (r0 + r1) + (r2 + r3): 2; bias_diff_finalize ceil(8 N / 64) + 6.  One-launch form (small_map): ceil(N hw / 256) trips,
      or 3 ceil(N hw / 4 / 256); 6; 2.
Bit-exact (compared as bit patterns with a numpy fp32 statement: each is one or two roundings): bias_leaky_relu forward (x + b, then
  t > 0 ? t : t * slope), scale_shift_forward (the product rounded, then the sum rounded) and the bottom_diff of the ReLU backward
  (g * (y > 0 ? 1 : slope)); top_data + 0.0 and - 0.0 both take the slope; slopes 0, 0.1 and 1.

Branches (flow_head_bounds restates pf_rb, pf_bands, the cpb loop, head_splits, small_map and the VEC4 condition; every case asserts
  the branch it is meant to select, and test_plans_match_the_c_api holds the restatement against the workspace sizes and the
  `supported` answers of the C API): rows per band 32, 16, 8, 2, 1, one band and several, full and ragged last bands; W = 1, W = 64,
  W > 64 in the lane walk; more than 64 parts in pf_finalize, uf_finalize and bias_diff_finalize (N >= 9); cpb 8, 16, 32, 64 with a
  channel tail; nsplit 1, 2, 4, 8 and empty channel groups; the scalar forms for hw % 4 != 0 and for a 4-byte aligned pointer; the
  grid-stride trips of the bias forward (> 64 blocks), scale_shift (> 256 or > 64 blocks) and deconv4x4s2_c2 (> 4096 blocks); a second
  chunk of 65535 planes in the bias forward; small_map from both sides of C = 128 and N hw = 20000; channel slices; accumulate.

Fixed with these tests: fn2_bias_leaky_relu_forward launched its first chunk of 65535 planes in place and only then refused a blob
  whose C does not divide 65535; it now refuses before the first launch and leaves the blob as it was
  (test_bias_forward_refused_chunking_leaves_the_blob).

Worst error / bound on the MI355X (this file's printed ratios; d is a worst-case chain, rounding errors do not line up): pf_dgrad 0.24
  (cpb 8 0.24, 16 0.21, 32 0.22, 64 0.24); pf_wgrad + pf_finalize 0.050 (accumulating 0.021); predict_flow bias gradient 0.0054;
  predict_flow forward 0.056, 0.0054, 0.0022, 0.0013 for nsplit 1, 2, 4, 8; uf_backward bottom gradient 0.084, weight gradient 0.049
  (accumulating 0.38: the final addition's u |ref| is most of that bound), bias gradient 0.046; upsample_flow forward 0.47; bias
  gradients of bias_act.hip: two-launch 0.022 (VEC4) and 0.018 (scalar), one-launch 0.0011 (VEC4) and 0.12 (scalar).
Tests marked gpu need the MI355X; the others check the plans, the statements against the C oracle and the teeth of the bounds on the CPU.
"""
import functools

import numpy as np
import pytest
import torch

import flow_head_bounds as B
import oracle
from flownet2_amd import _lib, ops

U = B.U


def rand(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def dev_misaligned(a):
    """The blob on the GPU as a contiguous view that starts one float into its storage: 4-byte, not 16-byte aligned."""
    a = np.array(a, dtype=np.float32, order="C")
    t = torch.empty(a.size + 1, device="cuda", dtype=torch.float32)[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = B.bits(got) != B.bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits; first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[bad][0]!r} != {want[bad][0]!r}"


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

# predict_flow backward: shape (N, C, H, W) -> rows per band, bands, channels per block of pf_dgrad
PF_BWD = {
    (1, 5, 1, 1): (32, 1, 8),              # a single pixel
    (3, 33, 40, 1): (8, 5, 8),             # W = 1, C % 16 = 1
    (2, 21, 3, 64): (32, 1, 8),            # W = 64
    (9, 17, 70, 65): (8, 9, 8),            # W > 64, ragged last band (6 rows), 81 parts
    (25, 100, 20, 3): (16, 2, 8),          # rb 16, ragged (4 rows)
    (25, 256, 64, 5): (32, 2, 8),          # rb 32, two full bands
    (1, 3088, 63, 3): (32, 2, 8),          # rb 32, ragged (31 rows)
    (1, 3, 5, 1500): (2, 3, 8),            # rb 2, ragged (1 row)
    (1, 3, 3, 2000): (1, 3, 8),            # rb 1
    (16, 2050, 5, 7): (32, 1, 16),         # cpb 16, 32, 64: C is no multiple of cpb
    (32, 2050, 5, 7): (32, 1, 32),
    (33, 4100, 5, 7): (32, 1, 64),
}
PF_BWD_SLICE = [(9, 17, 70, 65), (25, 100, 20, 3), (1, 3, 5, 1500)]       # channel slice, accumulate, determinism
UF_BWD = {(1, 1, 1): 1, (2, 16, 16): 2, (1, 257, 1): 2, (2, 1, 300): 4, (70, 3, 5): 70}      # (N, H, W) -> parts
UF_FWD = list(UF_BWD) + [(1, 520, 520)]
# predict_flow forward: shape -> nsplit
PF_FWD = {
    (1, 255, 2, 3): 1, (1, 256, 2, 3): 2, (1, 512, 2, 3): 4, (1, 1024, 2, 3): 8,      # the smallest C of each split
    (2, 512, 64, 64): 2,                                                               # C allows 4; 128 pixel blocks stop at 2
    (2, 5, 7, 9): 1, (3, 5, 3, 5): 1,                                                  # C < 16: empty channel groups; a block across samples
    (2, 20, 1, 37): 1, (2, 20, 37, 1): 1,                                              # H = 1, W = 1
}
# bias / ReLU backward: (N, C, H, W), misaligned top_diff? -> (VEC4, one-launch form)
BIAS_BWD = [
    ((2, 6, 8, 10), False, (True, False)),
    ((2, 6, 7, 9), False, (False, False)),                    # hw % 4 != 0
    ((2, 6, 8, 10), True, (False, False)),                    # a 4-byte aligned pointer
    ((1, 3, 1, 2051), False, (False, False)),                 # hw > 2048: a second trip inside a plane
    ((1, 2, 2, 4100), False, (True, False)),                  # hw / 4 > 2048: the same with 16-byte loads
    ((9, 5, 3, 4), False, (True, False)),                     # N = 9: 72 partials, a second trip in bias_diff_finalize; C % 4 != 0
    ((2, 127, 100, 100), False, (True, False)),               # small_map: C = 127 | 128, N hw = 20000 | 20001
    ((2, 128, 100, 100), False, (True, True)),
    ((3, 128, 59, 113), False, (False, False)),
    ((16, 128, 25, 50), False, (False, True)),                # the one-launch form, scalar (hw % 4 = 2), N hw = 20000
    ((16, 128, 25, 50), True, (False, True)),
    ((2, 130, 4, 6), True, (False, True)),                    # the one-launch form, scalar for the pointer alone
]
BIAS_FWD = [
    ((2, 5, 4, 6), False, (True, False, 1)),                  # -> (VEC4, grid-stride trip, chunks)
    ((2, 5, 3, 5), False, (False, False, 1)),
    ((2, 5, 4, 6), True, (False, False, 1)),
    ((1, 2, 1, 65540), False, (True, True, 1)),               # 65 > 64 blocks of 16-byte loads
    ((1, 1, 1, 16387), False, (False, True, 1)),              # 65 > 64 scalar blocks
    ((514, 255, 1, 1), False, (False, False, 2)),             # N C = 2 * 65535: a second chunk
    ((514, 255, 2, 2), False, (True, False, 2)),
]
SCALE_SHIFT = [
    ((2, 3, 4, 6), False, (True, False)),                     # -> (VEC4, grid-stride trip)
    ((2, 3, 3, 5), False, (False, False)),
    ((2, 3, 4, 6), True, (False, False)),
    ((1, 1, 513, 512), False, (True, True)),                  # 257 > 256 blocks
    ((1, 1, 127, 131), False, (False, True)),                 # 65 > 64 scalar blocks
]
SLOPES = [0.0, 0.1, 1.0]


def ids(cases):
    return [str(c).replace(" ", "") for c in cases]


# ---- inputs and statements: computed once per shape, shared by the CPU and the GPU tests, never written to ---------------------------------

def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pf_bwd_inputs(shape):
    N, Cc, H, W = shape
    x, w, g = frozen(rand(shape, 700), rand((2, Cc, 3, 3), 701, 0.1), rand((N, 2, H, W), 702))
    return x, w, g, B.pf_backward_statement(x, w, g)


@functools.lru_cache(maxsize=None)
def uf_inputs(shape):
    N, H, W = shape
    x, w, b, g = frozen(rand((N, 2, H, W), 710), rand((2, 2, 4, 4), 711, 0.3), rand((2,), 712), rand((N, 2, 2 * H, 2 * W), 713))
    return x, w, b, g


@functools.lru_cache(maxsize=None)
def uf_bwd_statement(shape):
    x, w, _, g = uf_inputs(shape)
    return B.uf_backward_statement(x, w, g)


@functools.lru_cache(maxsize=None)
def pf_fwd_inputs(shape):
    N, Cc, H, W = shape
    return frozen(rand(shape, 720), rand((2, Cc, 3, 3), 721, 0.1), rand((2,), 722))


def relu_inputs(shape, seed=730):
    """top_data with + 0.0 and - 0.0 planted among its values, and top_diff."""
    y, g = rand(shape, seed), rand(shape, seed + 1)
    flat = y.reshape(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    assert (B.bits(flat) == 0x80000000).any() and (B.bits(flat) == 0).any()
    return y, g


def named(name, form):
    """The kernel form a ratio is recorded under; None (not recorded) for the CPU checks."""
    return None if form is None else name + form


def check_pf_backward(shape, dx, dw, db, what, start=None, form=None):
    """The three gradients of predict_flow against the statement; `start` = (dw, db) before an accumulating call."""
    st = pf_bwd_inputs(shape)[3]
    if dx is not None:
        B.bounded(dx, st["dx"], st["Adx"], B.CHAIN_PF_DGRAD, f"{what} bottom_diff", named(f"pf_dgrad cpb {B.pf_cpb(*shape)}", form))
    if dw is not None:
        B.bounded(dw, st["dw"], st["Adw"], B.chain_pf_wgrad(*shape), f"{what} weight_diff", named("pf_wgrad + pf_finalize", form),
                  None if start is None else start[0])
    if db is not None:
        B.bounded(db, st["db"], st["Adb"], B.chain_pf_bias(*shape), f"{what} bias_diff", named("predict_flow bias gradient", form),
                  None if start is None else start[1])


def check_uf_backward(shape, dx, dw, db, what, start=None, form=None):
    st = uf_bwd_statement(shape)
    if dx is not None:
        B.bounded(dx, st["dx"], st["Adx"], B.CHAIN_UF_DGRAD, f"{what} bottom_diff", named("uf_backward bottom gradient", form))
    if dw is not None:
        B.bounded(dw, st["dw"], st["Adw"], B.chain_uf_wgrad(*shape), f"{what} weight_diff", named("uf_backward + uf_finalize weights", form),
                  None if start is None else start[0])
    if db is not None:
        B.bounded(db, st["db"], st["Adb"], B.chain_uf_bias(*shape), f"{what} bias_diff", named("uf_backward + uf_finalize bias", form),
                  None if start is None else start[1])


def check_pf_forward(shape, out, bias, what, form=None):
    x, w, b = pf_fwd_inputs(shape)
    ref, A = B.pf_forward_statement(x, w, b if bias else None)
    B.bounded(out, ref, A, B.chain_pf_forward(*shape), what, named(f"predict_flow forward nsplit {B.head_splits(*shape)}", form))


def check_uf_forward(shape, out, bias, what, form=None):
    x, w, b, _ = uf_inputs(shape)
    ref, A = B.uf_forward_statement(x, w, b if bias else None)
    B.bounded(out, ref, A, B.CHAIN_UF_FORWARD, what, named("upsample_flow forward", form))


def check_bias_grad(shape, vec, db, summed, what, start=None, form=None):
    """db [C] against the fp64 sum of the fp32 blob `summed` [N,C,H,W] in the launch form the shape selects."""
    N, Cc, H, W = shape
    ref, A = B.bias_sum_statement(summed)
    name = ("one-launch" if B.small_map(N, Cc, H * W) else "two-launch") + (" VEC4" if vec else " scalar")
    B.bounded(db, ref, A, B.chain_bias_grad(N, Cc, H * W, vec), what, named(f"bias gradient {name}", form), start)


# ---- CPU: the plans ---------------------------------------------------------------------------------------------------------------------------

def test_cases_select_their_branches():
    for shape, (rb, bands, cpb) in PF_BWD.items():
        assert (B.pf_rb(*shape), B.pf_bands(*shape), B.pf_cpb(*shape)) == (rb, bands, cpb), shape
        assert shape[1] % cpb != 0 or cpb == 8
    assert 70 % 8 == 6 and 20 % 16 == 4 and 64 % 32 == 0 and 63 % 32 == 31       # the last bands of the multi-band shapes: ragged, ragged, full, ragged
    assert B.pf_parts(9, 17, 70, 65) == 81 > 64                                  # the second trip of pf_finalize
    assert {s[3] for s in PF_BWD} >= {1, 64, 65} and 64 // 65 == 0               # the lane walk: step_rows 64, 1 and 0
    assert all(s in PF_BWD for s in PF_BWD_SLICE)
    for shape, parts in UF_BWD.items():
        assert B.uf_parts(*shape) == parts, shape
    assert B.uf_parts(70, 3, 5) > 64                                             # the second trip of uf_finalize
    assert [B.uf_forward_blocks(*s)[1] for s in UF_FWD] == [False] * 5 + [True]
    for shape, nsplit in PF_FWD.items():
        assert B.head_splits(*shape) == nsplit, shape
    assert B.head_splits(1, 511, 2, 3) == 2 and B.head_splits(1, 1023, 2, 3) == 4 and B.head_splits(2, 512, 64, 63) == 4
    assert B.head_splits(4, 1024, 2, 3, batch_invariant=True) == B.head_splits(1, 1024, 2, 3)
    for (N, Cc, Hh, W), mis, (vec, one) in BIAS_BWD:
        assert (B.vec4(Hh * W, 4 if mis else 0), B.small_map(N, Cc, Hh * W)) == (vec, one), (N, Cc, Hh, W)
    assert B.small_map(2, 128, 10000) and not B.small_map(2, 127, 10000) and not B.small_map(3, 128, 6667) and 3 * 6667 == 20001
    assert B.chain_bias_grad(9, 5, 12, True) - B.chain_bias_grad(8, 5, 12, True) == 1          # N = 9: the second trip of the finalize
    assert B.chain_bias_grad(1, 3, 2051, False) == 2 + 6 + 2 + 1 + 6 and B.chain_bias_grad(1, 2, 8200, True) == 3 * 2 + 6 + 2 + 1 + 6
    for (N, Cc, Hh, W), mis, (vec, stride, chunks) in BIAS_FWD:
        assert B.vec4(Hh * W, 4 if mis else 0) == vec
        assert B.bias_forward_plan(N, Cc, Hh * W, vec)[1:] == (stride, chunks, True), (N, Cc, Hh, W)
    assert B.bias_forward_plan(2, 40000, 1, False)[3] is False and B.bias_forward_plan(1, 65535, 1, False)[3] is True
    for (N, Cc, Hh, W), mis, (vec, stride) in SCALE_SHIFT:
        assert B.vec4(Hh * W, 4 if mis else 0) == vec and B.scale_shift_plan(Hh * W, vec)[1] == stride, (N, Cc, Hh, W)


PLAN_SHAPES = list(PF_BWD) + [(8, 194, 128, 256), (8, 194, 80, 112), (1, 18, 12, 1000), (2, 194, 24, 40), (1, 1026, 10, 14), (1, 20, 40, 300),
                              (64, 256, 33, 9), (3, 700, 130, 40), (5, 40, 40, 223), (5, 40, 40, 224), (5, 40, 40, 424), (5, 40, 40, 425),
                              (1, 16, 20, 766), (1, 16, 20, 767), (1, 16, 200, 1278), (1, 16, 9, 1279)]


def test_plans_match_the_c_api():
    """What the C API shows of the plans: parts (hence bands) through the backward's workspace, nsplit through the forward's, and the
    widest supported row."""
    L = _lib.lib()
    for shape in PLAN_SHAPES:
        N, Cc, H, W = shape
        nbytes = L.fn2_predict_flow_conv_backward_workspace_bytes(*shape)
        assert nbytes == B.pf_backward_workspace_bytes(*shape), shape
        assert nbytes // (4 * (18 * Cc + 2)) == N * B.pf_bands(*shape)
        assert L.fn2_predict_flow_conv_backward_supported(*shape) == int(B.pf_backward_supported(*shape)) == 1
    assert {B.pf_rb(*s) for s in PLAN_SHAPES} == {32, 16, 8, 4, 2, 1}
    for shape in list(PF_FWD) + [(1, 511, 2, 3), (1, 1023, 2, 3), (2, 512, 64, 63), (8, 194, 80, 112), (1, 1026, 10, 14), (4, 386, 24, 32)]:
        N, Cc, H, W = shape
        assert L.fn2_predict_flow_conv_workspace_bytes(*shape) == 4 * B.head_splits(*shape) * N * 18 * H * W, shape
    assert B.pf_rb(1, 16, 8, 2558) == 1 and B.pf_rb(1, 16, 8, 2559) == 0
    assert L.fn2_predict_flow_conv_backward_supported(1, 16, 8, 2558) == 1 and L.fn2_predict_flow_conv_backward_supported(1, 16, 8, 2559) == 0
    assert not B.pf_backward_supported(1, 16, 8, 2559) and not B.pf_backward_supported(0, 16, 8, 8)
    assert L.fn2_predict_flow_conv_backward_supported(65535, 1, 1, 1) == int(B.pf_backward_supported(65535, 1, 1, 1)) == 1
    assert L.fn2_predict_flow_conv_backward_supported(40000, 1, 64, 1) == int(B.pf_backward_supported(40000, 1, 64, 1)) == 0     # N bands > 65535
    for N, H, W in UF_BWD:
        assert L.fn2_upsample_flow_deconv_backward_workspace_bytes(N, H, W) == 4 * 66 * B.uf_parts(N, H, W)
    assert L.fn2_bias_leaky_relu_backward_workspace_bytes(9, 5, 3, 4) == 4 * 9 * 5 * B.K_BWD_CHUNKS


# ---- CPU: the statements against the C oracle, within the same bounds ------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(PF_BWD), ids=ids(PF_BWD))
def test_oracle_predict_flow_backward(shape):
    x, w, g, _ = pf_bwd_inputs(shape)
    check_pf_backward(shape, *oracle.predict_flow_conv_backward(x, w, g), f"oracle {shape}")


@pytest.mark.parametrize("shape", list(UF_BWD), ids=ids(UF_BWD))
def test_oracle_upsample_flow(shape):
    x, w, b, g = uf_inputs(shape)
    check_uf_backward(shape, *oracle.upsample_flow_deconv_backward(x, w, g), f"oracle {shape}")
    check_uf_forward(shape, oracle.upsample_flow_deconv_forward(x, w, b), True, f"oracle forward {shape}")
    check_uf_forward(shape, oracle.upsample_flow_deconv_forward(x, w, None), False, f"oracle forward {shape}, no bias")


@pytest.mark.parametrize("shape", list(PF_FWD), ids=ids(PF_FWD))
def test_oracle_predict_flow_forward(shape):
    x, w, b = pf_fwd_inputs(shape)
    check_pf_forward(shape, oracle.predict_flow_conv_forward(x, w, b), True, f"oracle {shape}")
    check_pf_forward(shape, oracle.predict_flow_conv_forward(x, w, None), False, f"oracle {shape}, no bias")


@pytest.mark.parametrize("slope", SLOPES)
def test_oracle_bias_relu_and_scale_shift(slope):
    shape = (9, 5, 3, 4)
    y, g = relu_inputs(shape)
    bias = rand((5,), 740)
    same_bits(oracle.bias_leaky_relu_forward(y, bias, slope), B.bias_leaky_relu_statement(y, bias, slope), "oracle bias forward")
    same_bits(oracle.bias_leaky_relu_forward(y, None, slope), B.bias_leaky_relu_statement(y, None, slope), "oracle bias forward, no bias")
    d, db = oracle.bias_leaky_relu_backward(y, g, slope)
    same_bits(d, B.relu_backward_statement(y, g, slope), "oracle bottom_diff")
    zero = y == 0
    same_bits(d[zero], (g[zero] * np.float32(slope)).astype(np.float32), "a zero of either sign takes the slope")
    check_bias_grad(shape, True, db, d, "oracle bias_diff")
    acc = rand((5,), 741)
    start = acc.copy()
    assert oracle.lib().fn2_conv_backward_bias_cpu(oracle._p(g), 5, 0, oracle._p(acc), 9, 5, 3, 4, 1) == 0
    check_bias_grad(shape, True, acc, g, "oracle conv_backward_bias, accumulate", start=start)
    x = np.random.default_rng(742).integers(0, 256, shape).astype(np.float32)
    same_bits(oracle.scale_shift_forward(x, 1.0 / 255.0, -bias), B.scale_shift_statement(x, 1.0 / 255.0, -bias), "oracle scale_shift")
    same_bits(oracle.scale_shift_forward(x, 1.0 / 255.0, None), B.scale_shift_statement(x, 1.0 / 255.0, None), "oracle scale_shift, no shift")


def test_scale_shift_statement_is_two_roundings():
    """The statement differs from a fused multiply-add somewhere: the check can tell the two apart."""
    x = np.random.default_rng(743).integers(0, 256, (1, 3, 64, 64)).astype(np.float32)
    sh = -rand((3,), 744, 0.3)
    fused = (x.astype(np.float64) * np.float64(np.float32(1.0 / 255.0)) + sh.astype(np.float64).reshape(1, 3, 1, 1)).astype(np.float32)
    assert (B.bits(fused) != B.bits(B.scale_shift_statement(x, 1.0 / 255.0, sh))).any()


# ---- CPU: the bounds have teeth -------------------------------------------------------------------------------------------------------------

def test_bound_notices_a_dropped_term():
    shape = (3, 33, 40, 1)
    x, w, g, _ = pf_bwd_inputs(shape)
    _, dw, _ = oracle.predict_flow_conv_backward(x, w, g)
    n, c, y = np.unravel_index(int(np.argmax(np.abs(x[:, :, :, 0] * g[:, 1:2, :, 0]))), (3, 33, 40))
    dw = dw.copy()
    dw[1, c, 1, 1] -= x[n, c, y, 0] * g[n, 1, y, 0]                   # the centre tap pairs a pixel with itself
    with pytest.raises(AssertionError):
        check_pf_backward(shape, None, dw, None, "dropped term")
    shape = (70, 3, 5)
    x, w, _, g = uf_inputs(shape)
    _, dw, _ = oracle.upsample_flow_deconv_backward(x, w, g)
    terms = x[:, 1] * g[:, 0, 0::2, 1::2]                             # dw[ci 1][co 0][ky 1][kx 2]: bottom (y, x) with top_diff (2 y, 2 x + 1)
    dw = dw.copy()
    dw[1, 0, 1, 2] -= terms.reshape(-1)[int(np.argmax(np.abs(terms)))]
    with pytest.raises(AssertionError):
        check_uf_backward(shape, None, dw, None, "dropped term")


@pytest.mark.parametrize("shape", [(25, 100, 20, 3), (9, 17, 70, 65), (1, 3, 5, 1500)], ids=str)
def test_bound_notices_a_dropped_halo_row(shape):
    """A band that forgets the top_diff row above its first row: bottom row y0 then misses its ky = 2 terms (top_diff row y0 - 1)."""
    x, w, g, _ = pf_bwd_inputs(shape)
    N, Cc, H, W = shape
    rb = B.pf_rb(*shape)
    y0 = rb * (B.pf_bands(*shape) - 1)                                 # the last band, ragged where the shape makes it so
    assert 0 < y0 < H
    _, dw, _ = oracle.predict_flow_conv_backward(x, w, g)
    dw = dw.astype(np.float64)
    xr, gr = x[:, :, y0].astype(np.float64), g[:, :, y0 - 1].astype(np.float64)            # [N,C,W], [N,2,W]
    for kx in range(3):                                                # bottom column xb pairs with top_diff column xb + 1 - kx
        lo, hi = max(0, kx - 1), min(W, W + kx - 1)
        dw[:, :, 2, kx] -= np.einsum("ncx,nox->oc", xr[:, :, lo:hi], gr[:, :, lo + 1 - kx:hi + 1 - kx])
    with pytest.raises(AssertionError):
        check_pf_backward(shape, None, dw, None, "dropped halo row")


def test_bound_notices_a_dropped_part():
    shape = (9, 17, 70, 65)                                             # part = (sample 8, the ragged last band): rows 64 .. 69
    x, w, g, _ = pf_bwd_inputs(shape)
    x2, g2 = x.copy(), g.copy()
    x2[8, :, 64:] = 0
    _, dw, _ = oracle.predict_flow_conv_backward(x2, w, g)              # the weight gradient is linear in the bottom rows of a part
    with pytest.raises(AssertionError):
        check_pf_backward(shape, None, dw, None, "dropped part")
    g2[8, :, 64:] = 0
    _, _, db = oracle.predict_flow_conv_backward(x, w, g2)
    with pytest.raises(AssertionError):
        check_pf_backward(shape, None, None, db, "dropped part")
    shape = (70, 3, 5)                                                  # part = sample 69
    x, w, _, g = uf_inputs(shape)
    x2, g2 = x.copy(), g.copy()
    x2[69], g2[69] = 0, 0
    with pytest.raises(AssertionError):
        check_uf_backward(shape, None, oracle.upsample_flow_deconv_backward(x2, w, g)[1], None, "dropped part")
    with pytest.raises(AssertionError):
        check_uf_backward(shape, None, None, oracle.upsample_flow_deconv_backward(x, w, g2)[2], "dropped part")
    shape = (9, 5, 3, 4)                                                # the partials of one plane (the second trip of the finalize)
    _, g = relu_inputs(shape)
    db = g.astype(np.float64).sum((0, 2, 3))
    db[4] -= g[8, 4].astype(np.float64).sum()
    with pytest.raises(AssertionError):
        check_bias_grad(shape, True, db, g, "dropped partial")


def test_bound_notices_a_weight_off_by_2_to_the_minus_10():
    shape = (2, 21, 3, 64)
    x, w, g, _ = pf_bwd_inputs(shape)
    w2 = w.copy()
    w2[1, 20, 0, 2] *= np.float32(1 + 2.0 ** -10)
    with pytest.raises(AssertionError):
        check_pf_backward(shape, oracle.predict_flow_conv_backward(x, w2, g)[0], None, None, "tap off")
    shape = (2, 5, 7, 9)
    x, w, b = pf_fwd_inputs(shape)
    w2 = w.copy()
    w2[0, 4, 2, 0] *= np.float32(1 + 2.0 ** -10)
    with pytest.raises(AssertionError):
        check_pf_forward(shape, oracle.predict_flow_conv_forward(x, w2, b), True, "tap off")
    shape = (2, 1, 300)
    x, w, b, g = uf_inputs(shape)
    w2 = w.copy()
    w2[1, 0, 2, 1] *= np.float32(1 + 2.0 ** -10)                       # (H = 1: rows ky 1 and 2 are the ones in use)
    with pytest.raises(AssertionError):
        check_uf_backward(shape, oracle.upsample_flow_deconv_backward(x, w2, g)[0], None, None, "tap off")
    with pytest.raises(AssertionError):
        check_uf_forward(shape, oracle.upsample_flow_deconv_forward(x, w2, b), True, "tap off")


def test_accumulate_bound_is_about_the_sum():
    """With `start` the statement is start + gradient: a result that forgot the start, or added it twice, leaves the bound."""
    shape = (25, 100, 20, 3)
    x, w, g, st = pf_bwd_inputs(shape)
    _, dw, db = oracle.predict_flow_conv_backward(x, w, g)
    start = (rand(dw.shape, 750), rand(db.shape, 751))
    check_pf_backward(shape, None, (start[0].astype(np.float64) + st["dw"]).astype(np.float32),
                      (start[1].astype(np.float64) + st["db"]).astype(np.float32), "accumulated", start=start)
    with pytest.raises(AssertionError):
        check_pf_backward(shape, None, dw, None, "start forgotten", start=start)
    with pytest.raises(AssertionError):
        check_pf_backward(shape, None, None, db + 2 * start[1], "start twice", start=start)


# ---- GPU: predict_flow backward ------------------------------------------------------------------------------------------------------------------

NEEDS = [(True, False, False), (False, True, False), (False, False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(PF_BWD), ids=ids(PF_BWD))
def test_predict_flow_backward(shape):
    rb, bands, cpb = PF_BWD[shape]
    assert (B.pf_rb(*shape), B.pf_bands(*shape), B.pf_cpb(*shape)) == (rb, bands, cpb)
    x, w, g, _ = pf_bwd_inputs(shape)
    xd, wd, gd = dev(x), dev(w), dev(g)
    both = ops.predict_flow_conv_backward(xd, wd, gd)
    check_pf_backward(shape, *map(host, both), f"{shape}", form="")
    for needs in NEEDS:                                                 # each gradient on its own: the bits of the joint call
        one = ops.predict_flow_conv_backward(xd, wd, gd, *needs)
        for need, a, b in zip(needs, one, both):
            assert (a is None) == (not need) and (a is None or torch.equal(a, b)), (shape, needs)
    again = ops.predict_flow_conv_backward(xd, wd, gd)
    assert all(torch.equal(a, b) for a, b in zip(again, both)), "not the same bits on a second run"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PF_BWD_SLICE, ids=str)
def test_predict_flow_backward_slice_and_accumulate(shape):
    N, Cc, H, W = shape
    x, w, g, _ = pf_bwd_inputs(shape)
    blob = rand((N, Cc + 3, H, W), 760)
    blob[:, 2:2 + Cc] = x
    wd, gd = dev(w), dev(g)
    plain = ops.predict_flow_conv_backward(dev(x), wd, gd)
    sliced = ops.predict_flow_conv_backward((dev(blob), 2, Cc), wd, gd)
    assert all(torch.equal(a, b) for a, b in zip(sliced, plain)), "a channel slice read in place gives other bits"
    check_pf_backward(shape, *map(host, sliced), f"slice {shape}", form="")
    start = (rand(w.shape, 761), rand((2,), 762))
    for accumulate in (False, True):
        out = (torch.full((N, Cc, H, W), 5.0, device="cuda"), dev(start[0]), dev(start[1]))
        got = ops.predict_flow_conv_backward(dev(x), wd, gd, out=out, accumulate=accumulate)
        assert all(a is b for a, b in zip(got, out))
        assert torch.equal(out[0], plain[0])                            # the bottom gradient is written, never added to
        if accumulate:
            check_pf_backward(shape, None, host(out[1]), host(out[2]), f"accumulate {shape}", start=start, form=", accumulate")
            same_bits(host(out[1]), host(dev(start[0]) + plain[1]), "accumulate: start + the gradient, one rounding")
            same_bits(host(out[2]), host(dev(start[1]) + plain[2]), "accumulate: start + the gradient, one rounding")
        else:
            assert torch.equal(out[1], plain[1]) and torch.equal(out[2], plain[2]), "accumulate = 0 must overwrite"
    only_b = (None, None, dev(start[1]))
    ops.predict_flow_conv_backward(dev(x), wd, gd, False, False, True, out=only_b, accumulate=True)
    check_pf_backward(shape, None, None, host(only_b[2]), f"accumulate bias alone {shape}", start=start, form=", accumulate")


# ---- GPU: upsample_flow ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(UF_BWD), ids=ids(UF_BWD))
def test_upsample_flow_backward(shape):
    N, H, W = shape
    assert B.uf_parts(*shape) == UF_BWD[shape]
    x, w, _, g = uf_inputs(shape)
    xd, wd, gd = dev(x), dev(w), dev(g)
    both = ops.upsample_flow_deconv_backward(xd, wd, gd)
    check_uf_backward(shape, *map(host, both), f"{shape}", form="")
    for needs in NEEDS:                                                 # (True, False, False) is the want_w = 0 early return
        one = ops.upsample_flow_deconv_backward(xd, wd, gd, *needs)
        for need, a, b in zip(needs, one, both):
            assert (a is None) == (not need) and (a is None or torch.equal(a, b)), (shape, needs)
    again = ops.upsample_flow_deconv_backward(xd, wd, gd)
    assert all(torch.equal(a, b) for a, b in zip(again, both)), "not the same bits on a second run"
    start = (rand((2, 2, 4, 4), 770), rand((2,), 771))
    for accumulate in (False, True):
        out = (torch.full((N, 2, H, W), 5.0, device="cuda"), dev(start[0]), dev(start[1]))
        ops.upsample_flow_deconv_backward(xd, wd, gd, out=out, accumulate=accumulate)
        assert torch.equal(out[0], both[0])
        if accumulate:
            check_uf_backward(shape, None, host(out[1]), host(out[2]), f"accumulate {shape}", start=start, form=", accumulate")
        else:
            assert torch.equal(out[1], both[1]) and torch.equal(out[2], both[2]), "accumulate = 0 must overwrite"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", UF_FWD, ids=str)
def test_upsample_flow_forward(shape):
    N, H, W = shape
    assert B.uf_forward_blocks(*shape)[1] == (shape == (1, 520, 520))
    x, w, b, _ = uf_inputs(shape)
    xd, wd = dev(x), dev(w)
    out = ops.upsample_flow_deconv_forward(xd, wd, dev(b))
    check_uf_forward(shape, host(out), True, f"{shape}", form="")
    check_uf_forward(shape, host(ops.upsample_flow_deconv_forward(xd, wd, None)), False, f"{shape}, no bias", form="")
    top = torch.full((N, 5, 2 * H, 2 * W), -9.0, device="cuda")        # the _into form: channels 2, 3 of five; the others keep the sentinel
    view = ops.upsample_flow_deconv_forward(xd, wd, dev(b), out=top, out_c0=2)
    assert torch.equal(view, out) and torch.equal(top[:, 2:4], out), "the channel-slice form gives other bits"
    assert bool((top[:, :2] == -9.0).all()) and bool((top[:, 4:] == -9.0).all()), "the channel-slice form wrote outside its slice"


# ---- GPU: predict_flow forward -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(PF_FWD), ids=ids(PF_FWD))
def test_predict_flow_forward(shape):
    assert B.head_splits(*shape) == PF_FWD[shape] and not ops.get_batch_invariant()
    x, w, b = pf_fwd_inputs(shape)
    xd, wd = dev(x), dev(w)
    out = ops.predict_flow_conv_forward(xd, wd, dev(b))
    check_pf_forward(shape, host(out), True, f"{shape}", form="")
    check_pf_forward(shape, host(ops.predict_flow_conv_forward(xd, wd, None)), False, f"{shape}, no bias", form="")
    assert torch.equal(out, ops.predict_flow_conv_forward(xd, wd, dev(b))), "not the same bits on a second run"


# ---- GPU: bias / ReLU backward, conv_backward_bias -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", BIAS_BWD, ids=ids(BIAS_BWD))
def test_bias_relu_backward_and_conv_backward_bias(case):
    shape, misaligned, (vec, one_launch) = case
    N, Cc, H, W = shape
    y, g = relu_inputs(shape)
    yd, gd = dev(y), (dev_misaligned if misaligned else dev)(g)
    assert (B.vec4(H * W, yd.data_ptr(), gd.data_ptr()), B.small_map(N, Cc, H * W)) == (vec, one_launch)
    for slope in SLOPES:
        d, db = ops.bias_leaky_relu_backward(yd, gd, slope)
        assert d.data_ptr() % 16 == 0
        want = B.relu_backward_statement(y, g, slope)
        same_bits(host(d), want, f"bottom_diff {case}, slope {slope}")
        check_bias_grad(shape, vec, host(db), want, f"bias_diff {case}, slope {slope}", form=" (ReLU)")
        d2, none = ops.bias_leaky_relu_backward(yd, gd, slope, need_bias_diff=False)
        assert none is None and torch.equal(d2, d)
    # the bias gradient alone; its VEC4 condition looks at top_diff only
    db = ops.conv_backward_bias(gd, Cc)
    check_bias_grad(shape, vec, host(db), g, f"conv_backward_bias {case}", form=" (bias alone)")
    assert torch.equal(db, ops.conv_backward_bias(gd, Cc)), "not the same bits on a second run"
    start = rand((Cc,), 780)
    acc = dev(start)
    ops.conv_backward_bias(gd, Cc, out=acc, accumulate=True)
    check_bias_grad(shape, vec, host(acc), g, f"conv_backward_bias accumulate {case}", start=start, form=" (bias alone), accumulate")
    same_bits(host(acc), host(dev(start) + db), "accumulate: start + the gradient, one rounding")
    over = dev(start)
    ops.conv_backward_bias(gd, Cc, out=over, accumulate=False)
    assert torch.equal(over, db), "accumulate = 0 must overwrite"


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in BIAS_BWD if not c[1] and c[0][1] <= 128 and c[0] != (3, 128, 59, 113)], ids=str)
def test_bias_relu_backward_channel_slices(case):
    """Both blobs as channel slices of wider blobs: the bits of the copied-out slices, so every bound above holds for them."""
    shape, _, (vec, one_launch) = case
    N, Cc, H, W = shape
    y, g = relu_inputs(shape)
    ywide, gwide = rand((N, Cc + 3, H, W), 790), rand((N, Cc + 5, H, W), 791)
    ywide[:, 1:1 + Cc], gwide[:, 4:4 + Cc] = y, g
    yw, gw = dev(ywide), dev(gwide)
    d0, b0 = ops.bias_leaky_relu_backward(dev(y), dev(g), 0.1)
    d1, b1 = ops.bias_leaky_relu_backward((yw, 1, Cc), (gw, 4, Cc), 0.1)
    assert torch.equal(d0, d1) and torch.equal(b0, b1)
    same_bits(host(d1), B.relu_backward_statement(y, g, 0.1), f"bottom_diff of slices {case}")
    check_bias_grad(shape, vec, host(b1), host(d1), f"bias_diff of slices {case}", form=" (ReLU)")
    assert torch.equal(ops.conv_backward_bias(gw, Cc, top_c0=4), ops.conv_backward_bias(dev(g), Cc))


# ---- GPU: bias forward ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", BIAS_FWD, ids=ids(BIAS_FWD))
def test_bias_forward(case):
    shape, misaligned, (vec, stride, chunks) = case
    N, Cc, H, W = shape
    x, _ = relu_inputs(shape, 800)
    bias = rand((Cc,), 801)
    bias[::3] = 0.0                                                     # x = -0.0 meets b = +0.0 and x = 0 meets b = 0
    put = dev_misaligned if misaligned else dev
    for slope in SLOPES:
        for b in (bias, None):
            t = put(x)
            assert B.vec4(H * W, t.data_ptr()) == vec and B.bias_forward_plan(N, Cc, H * W, vec)[1:] == (stride, chunks, True)
            assert ops.bias_leaky_relu_(t, None if b is None else dev(b), slope) is t
            same_bits(host(t), B.bias_leaky_relu_statement(x, b, slope), f"bias forward {case}, slope {slope}, bias {b is not None}")


@pytest.mark.gpu
def test_bias_forward_refused_chunking_leaves_the_blob():
    """N C > 65535 with a C that does not divide 65535: refused before anything is launched, the blob keeps its bits."""
    shape = (2, 40000, 1, 1)
    assert B.bias_forward_plan(2, 40000, 1, False)[2:] == (2, False)
    x = rand(shape, 810)
    t = dev(x)
    with pytest.raises(_lib.Fn2Error) as e:
        ops.bias_leaky_relu_(t, dev(rand((40000,), 811)), 0.1)
    assert e.value.args and "65535" in str(e.value)
    torch.cuda.synchronize()
    same_bits(host(t), x, "the refused blob")


# ---- GPU: scale_shift ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", SCALE_SHIFT, ids=ids(SCALE_SHIFT))
def test_scale_shift(case):
    shape, misaligned, (vec, stride) = case
    N, Cc, H, W = shape
    x = np.random.default_rng(820).integers(0, 256, shape).astype(np.float32)
    sh = -rand((Cc,), 821, 0.3)
    xd = (dev_misaligned if misaligned else dev)(x)
    out = ops.scale_shift_forward(xd, 1.0 / 255.0, dev(sh))
    assert B.vec4(H * W, xd.data_ptr(), out.data_ptr()) == vec and B.scale_shift_plan(H * W, vec)[1] == stride
    want = B.scale_shift_statement(x, 1.0 / 255.0, sh)
    same_bits(host(out), want, f"scale_shift {case}")
    same_bits(host(ops.scale_shift_forward(xd, 1.0 / 255.0, None)), B.scale_shift_statement(x, 1.0 / 255.0, None), f"scale_shift {case}, no shift")
    top = torch.full((N, Cc + 4, H, W), 7.0, device="cuda")            # a slice of a wider top: the neighbours keep the sentinel
    ops.scale_shift_forward(xd, 1.0 / 255.0, dev(sh), out=top, out_c0=3)
    same_bits(host(top[:, 3:3 + Cc]), want, f"scale_shift into a slice {case}")
    assert bool((top[:, :3] == 7.0).all()) and bool((top[:, 3 + Cc:] == 7.0).all()), "scale_shift wrote outside its slice"


@pytest.mark.gpu
def test_scale_shift_refuses_too_many_planes():
    x = dev(rand((65536, 1, 1, 1), 830))
    out = torch.full_like(x, 7.0)
    with pytest.raises(_lib.Fn2Error):
        ops.scale_shift_forward(x, 0.5, None, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
