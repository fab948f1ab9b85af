"""Plans, chain lengths, fp64 statements and elementwise bounds for the flow heads (csrc/flow_head.hip, csrc/flow_head_bwd.hip) and the
bias / ReLU kernels (csrc/bias_act.hip).  CPU only: the statements are torch float64 on the CPU and numpy; nothing here touches a GPU.
tests/test_flow_heads_bias.py holds the derivations of the chains (its docstring) and the cases."""
import numpy as np
import torch

U = 2.0 ** -24
C_SLACK = 2                      # see the docstring of test_flow_heads_bias.py
MAX_CHAIN = 4096                 # d^2 u^2 / 2 < u for every chain below this length


def cdiv(a, b):
    return -(-a // b)


# ---- plans: the host functions' selections, restated from their formulas -----------------------------------------------------------------

K_CG, K_RB_MAX, PF_LDS_MAX = 16, 32, 60 * 1024          # kCG, kRBMax, kPfLdsMax (flow_head_bwd.hip)
K_HEAD_PIX, K_HEAD_G = 64, 16                            # kHeadPix, kHeadG (flow_head.hip)
K_BWD_CHUNKS = 8                                         # kBwdChunks (bias_act.hip)


def pf_lds(rb, W):
    return 4 * 2 * (rb + 2) * (W + 2)


def pf_rb(N, C, H, W):
    """Rows per band of pf_wgrad; 0 where not even one row fits the LDS."""
    best, best_cost = 0, -1
    rb = K_RB_MAX
    while rb >= 1:
        if pf_lds(rb, W) <= PF_LDS_MAX:
            if rb < 8 and best > 0:
                break
            blocks = N * cdiv(H, rb) * cdiv(C, K_CG)
            cost = cdiv(blocks, 512) * (min(rb, H) + 2)
            if best_cost < 0 or cost < best_cost:
                best_cost, best = cost, rb
        rb //= 2
    return best


def pf_bands(N, C, H, W):
    rb = pf_rb(N, C, H, W)
    return cdiv(H, rb) if rb > 0 else 0


def pf_parts(N, C, H, W):
    return N * pf_bands(N, C, H, W)


def pf_backward_supported(N, C, H, W):
    if N <= 0 or C <= 0 or H <= 0 or W <= 0 or H * W >= 2 ** 31 or N > 65535:
        return False
    return 0 < pf_parts(N, C, H, W) <= 65535


def pf_backward_workspace_bytes(N, C, H, W):
    parts = pf_parts(N, C, H, W)
    return 4 * (parts * 18 * C + parts * 2)


def pf_cpb(N, C, H, W):
    """Channels per block of pf_dgrad."""
    bx, cpb = cdiv(H * W, 256), 8
    while cpb < 64 and bx * cdiv(C, cpb) * N >= 4096:
        cpb *= 2
    return cpb


def head_splits(N, C, H, W, batch_invariant=False):
    """Channel splits of the predict_flow forward (1, 2, 4 or 8)."""
    blocks = cdiv((1 if batch_invariant else N) * H * W, K_HEAD_PIX)
    nsplit = 1
    while nsplit < 8 and blocks * K_HEAD_G * nsplit < 4096 and C >= 8 * K_HEAD_G * nsplit * 2:
        nsplit *= 2
    return nsplit


def pf_forward_workspace_bytes(N, C, H, W):
    return 4 * head_splits(N, C, H, W) * N * 18 * H * W


def uf_parts(N, H, W):
    return N * cdiv(H * W, 256)


def uf_forward_blocks(N, H, W):
    """(blocks of deconv4x4s2_c2, whether a thread takes a second output)."""
    need = cdiv(N * 4 * H * W, 256)
    return min(need, 4096), need > 4096


def small_map(N, C, hw):
    """The one-launch form of the bias gradient."""
    return C >= 128 and N * hw <= 20000


def vec4(hw, *ptrs):
    """16-byte loads and stores: rows of a multiple of 4 floats and every blob on a 16-byte boundary."""
    return hw % 4 == 0 and all(int(p) % 16 == 0 for p in ptrs)


def bias_forward_plan(N, C, hw, vec):
    """(blocks over a plane, grid-stride trip?, chunks of 65535 planes, supported?)."""
    per = hw // 4 if vec else hw
    need = cdiv(per, 256)
    planes = N * C
    return min(need, 64), need > 64, cdiv(planes, 65535), planes <= 65535 * 32 and (planes <= 65535 or 65535 % C == 0)


def scale_shift_plan(hw, vec):
    """(blocks over a plane, grid-stride trip?)."""
    need, cap = (cdiv(hw // 4, 256), 256) if vec else (cdiv(hw, 256), 64)
    return min(need, cap), need > cap


# ---- chains: the longest run of dependent roundings behind one output, in the decomposition that runs -----------------------------------

CHAIN_PF_DGRAD = 18
CHAIN_UF_DGRAD = 32
CHAIN_UF_FORWARD = 8


def chain_pf_wgrad(N, C, H, W):
    rows = min(pf_rb(N, C, H, W), H)
    return cdiv(rows * W, 64) + 6 + cdiv(pf_parts(N, C, H, W), 64) + 6


def chain_pf_bias(N, C, H, W):
    rows = min(pf_rb(N, C, H, W), H)
    return cdiv(rows * W, 256) + 6 + 3 + cdiv(pf_parts(N, C, H, W), 64) + 6


def chain_pf_forward(N, C, H, W, batch_invariant=False):
    nsplit = head_splits(N, C, H, W, batch_invariant)
    return cdiv(C, K_HEAD_G * nsplit) + 15 + 9 * nsplit


def chain_uf_wgrad(N, H, W):
    return 1 + 6 + 3 + cdiv(uf_parts(N, H, W), 64) + 6


def chain_uf_bias(N, H, W):
    return 2 + 6 + 3 + cdiv(uf_parts(N, H, W), 64) + 6


def chain_bias_grad(N, C, hw, vec):
    """The bias gradient of bias_leaky_relu_bwd + bias_diff_finalize, or of bias_leaky_relu_bwd_channel (small_map)."""
    if small_map(N, C, hw):
        own = 3 * cdiv(N * (hw // 4), 256) if vec else cdiv(N * hw, 256)
        return own + 6 + 2
    own = 3 * cdiv(hw // 4, 256 * K_BWD_CHUNKS) if vec else cdiv(hw, 256 * K_BWD_CHUNKS)
    return own + 6 + 2 + cdiv(N * K_BWD_CHUNKS, 64) + 6


# ---- fp64 statements (torch on the CPU) ---------------------------------------------------------------------------------------------------

def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _conv_backward(g, x, w, transposed, stride, mask=(True, True, True)):
    dx, dw, db = torch.ops.aten.convolution_backward(t64(g), t64(x), t64(w), [2], [stride, stride], [1, 1], [1, 1], transposed, [0, 0], 1,
                                                     list(mask))
    return tuple(None if t is None else t.numpy() for t in (dx, dw, db))


def _backward_statement(x, w, g, transposed, stride):
    ref = _conv_backward(g, x, w, transposed, stride)
    A = _conv_backward(np.abs(g), np.abs(x), np.abs(w), transposed, stride)
    return {"dx": ref[0], "dw": ref[1], "db": ref[2], "Adx": A[0], "Adw": A[1], "Adb": A[2]}


def pf_backward_statement(x, w, g):
    """Convolution{3,1,1} C -> 2: bottom, weight and bias gradients in fp64 and the sums of the absolute values of their terms."""
    return _backward_statement(x, w, g, False, 1)


def uf_backward_statement(x, w, g):
    """Deconvolution{4,2,1} 2 -> 2, likewise."""
    return _backward_statement(x, w, g, True, 2)


def pf_forward_statement(x, w, b=None):
    F = torch.nn.functional
    ref = F.conv2d(t64(x), t64(w), None if b is None else t64(b), padding=1).numpy()
    A = F.conv2d(t64(np.abs(x)), t64(np.abs(w)), None if b is None else t64(np.abs(b)), padding=1).numpy()
    return ref, A


def uf_forward_statement(x, w, b=None):
    F = torch.nn.functional
    ref = F.conv_transpose2d(t64(x), t64(w), None if b is None else t64(b), stride=2, padding=1).numpy()
    A = F.conv_transpose2d(t64(np.abs(x)), t64(np.abs(w)), None if b is None else t64(np.abs(b)), stride=2, padding=1).numpy()
    return ref, A


def bias_sum_statement(d):
    """[C] fp64 sums over n, y, x of the fp32 blob d [N,C,H,W], and of its absolute values."""
    d = np.asarray(d, np.float64)
    return d.sum((0, 2, 3)), np.abs(d).sum((0, 2, 3))


# ---- the bit-exact statements (numpy fp32: every operation is one rounding) -----------------------------------------------------------------

def bias_leaky_relu_statement(x, bias, slope):
    x = np.asarray(x, np.float32)
    b = np.zeros(x.shape[1], np.float32) if bias is None else np.asarray(bias, np.float32)      # no bias: the kernel adds + 0.0f
    t = (x + b.reshape(1, -1, 1, 1)).astype(np.float32)
    return np.where(t > 0, t, (t * np.float32(slope)).astype(np.float32)).astype(np.float32)


def relu_backward_statement(y, g, slope):
    y, g = np.asarray(y, np.float32), np.asarray(g, np.float32)
    return (g * np.where(y > 0, np.float32(1), np.float32(slope)).astype(np.float32)).astype(np.float32)


def scale_shift_statement(x, scale, shift):
    prod = (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float32)
    sh = np.zeros(x.shape[1], np.float32) if shift is None else np.asarray(shift, np.float32)
    return (prod + sh.reshape(1, -1, 1, 1)).astype(np.float32)


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


RATIOS = {}                      # kernel form -> worst error / bound seen in this process (printed by the tests)


def bounded(got, ref, A, d, what, form=None, start=None):
    """Every element: |got - ref| <= (d + C_SLACK) u A; with `start` (accumulate) ref becomes start + ref and the bound gains u |ref|.
    Returns the worst error / bound."""
    got, ref, A = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(A, np.float64)
    assert got.shape == ref.shape == A.shape, (what, got.shape, ref.shape, A.shape)
    assert 0 < d < MAX_CHAIN, (what, d)
    bound = (d + C_SLACK) * U * A
    if start is not None:
        ref = np.asarray(start, np.float64) + ref
        bound = bound + U * np.abs(ref)
    assert np.isfinite(ref).all() and np.isfinite(got).all(), f"{what}: non-finite value"
    err = np.abs(got - ref)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err - bound, -np.inf))), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} elements over the bound (d = {d}); at {list(map(int, i))}: "
                             f"|{got[i]!r} - {ref[i]!r}| = {err[i]:.3e} > {bound[i]:.3e}")
    ratio = float((err / np.where(bound > 0, bound, 1)).max()) if err.size else 0.0
    if form is not None:
        RATIOS[form] = max(RATIOS.get(form, 0.0), ratio)
        print(f"ratio [{form}] {what}: {ratio:.3g} (d = {d})")
    return ratio
