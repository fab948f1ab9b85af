"""What the tests of the general-geometry convolution (csrc/conv_general.hip) share: the geometry rows, the fp64 reference (torch's double
conv2d / conv_transpose2d and their autograd on the CPU, computed once per row) and a NumPy statement of the packed operand and of the two
gathers."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# (N, Cin, H, W, Cout, kernel, stride, pad)
CONV = [
    (1, 1, 5, 7, 1, 1, 1, 0),          # K = 1, below one k-step; one output channel
    (2, 3, 11, 13, 7, 3, 1, 2),        # pad beyond half the taps; Cout and K tails
    (3, 5, 9, 12, 33, 4, 2, 1),        # even taps; two channel groups plus one; three samples
    (1, 17, 23, 19, 20, 11, 4, 0),     # 11x11 / 4; K = 2057
    (2, 6, 8, 8, 16, 2, 3, 0),         # stride beyond the taps; bottom pixels with zero gradient
    (2, 40, 9, 12, 33, 3, 2, 2),       # the geometry the backward dispatcher is pinned to refuse
    (2, 64, 16, 24, 96, 5, 2, 2),      # the geometry the forward dispatcher is pinned to refuse
    (1, 4, 3, 3, 8, 5, 1, 2),          # taps larger than the image
    (1, 2, 4, 4, 3, 3, 1, 3),          # output rows that see only padding
    (1, 8, 6, 70, 4, 1, 2, 0),         # 1x1 stride 2; a pixel tile that wraps rows
]
DECONV = [                             # weight [Cin, Cout, k, k]
    (2, 5, 4, 6, 3, 4, 2, 1),          # FlowNet's taps with fewer than 64 inputs
    (1, 7, 5, 5, 9, 3, 1, 1),          # stride 1
    (2, 3, 4, 5, 6, 2, 2, 0),          # taps that do not overlap
    (1, 6, 3, 4, 5, 5, 3, 2),          # stride 3
    (1, 2, 6, 6, 2, 3, 2, 2),          # pad that cuts a border
]
ROWS = [(False,) + r for r in CONV] + [(True,) + r for r in DECONV]          # (transposed, N, Cin, H, W, Cout, k, s, p)
# FlowNet's own layer classes (the general kernels take them too): stem, 5x5 / 2, 3x3 / 1, 3x3 / 2, 1x1, and the 4x4 / 2 deconvolution
FLOWNET = [(False, 8, 3, 320, 448, 64, 7, 2, 3), (False, 8, 64, 160, 224, 128, 5, 2, 2), (False, 8, 256, 40, 56, 256, 3, 1, 1),
           (False, 8, 256, 40, 56, 512, 3, 2, 1), (False, 8, 256, 40, 56, 32, 1, 1, 0), (True, 8, 1024, 5, 7, 512, 4, 2, 1)]
# what the kernels refuse: empty output (conv, deconv), kernel 0, stride 0, negative pad, no channels, no samples
INVALID = [(False, 1, 3, 4, 4, 8, 7, 1, 1), (True, 1, 3, 1, 1, 8, 2, 1, 1), (False, 1, 3, 8, 8, 8, 0, 1, 0), (False, 1, 3, 8, 8, 8, 3, 0, 1),
           (False, 1, 3, 8, 8, 8, 3, 1, -1), (False, 1, 0, 8, 8, 8, 3, 1, 1), (True, 1, 3, 8, 8, 0, 3, 1, 1), (False, 0, 3, 8, 8, 8, 3, 1, 1),
           (False, 1, 3, 1 << 20, 1 << 20, 8, 3, 1, 1)]


def row_id(row):
    return ("deconv" if row[0] else "conv") + "-" + "x".join(str(v) for v in row[1:])


def out_hw(row):
    tr, N, Cin, H, W, Cout, k, s, p = row
    return (s * (H - 1) + k - 2 * p, s * (W - 1) + k - 2 * p) if tr else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)


def rand(shape, seed, scale=1.0):      # the conventions of tests/test_conv_backward_routes.py: unit normal data, weights scaled by 0.1
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def scale_of(ref):
    return max(1.0, float(np.abs(ref).max()))


def layer64(x, w, b, tr, s, p):
    return (F.conv_transpose2d if tr else F.conv2d)(x, w, b, stride=s, padding=p)


@functools.lru_cache(maxsize=None)
def case(row):
    """float32 inputs of the row and the fp64 results: dict(x, w, b, g, top (with bias, no activation), top_nobias, gx, gw, gb)."""
    tr, N, Cin, H, W, Cout, k, s, p = row
    Ho, Wo = out_hw(row)
    x, w, b = rand((N, Cin, H, W), 1), rand((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), 2, 0.1), rand((Cout,), 3)
    g = rand((N, Cout, Ho, Wo), 4)
    xt, wt, bt = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, b))
    top = layer64(xt, wt, bt, tr, s, p)
    assert tuple(top.shape) == (N, Cout, Ho, Wo)
    gx, gw, gb = torch.autograd.grad(top, (xt, wt, bt), torch.from_numpy(g).double())
    out = dict(x=x, w=w, b=b, g=g, top=top.detach().numpy(), top_nobias=(top.detach() - bt.detach().view(1, -1, 1, 1)).numpy(), gx=gx.numpy(),
               gw=gw.numpy(), gb=gb.numpy())
    for a in out.values():
        a.setflags(write=False)
    return out


def leaky(v, slope):
    return np.where(v > 0, v, v * slope)


# ---------------------------------------------------------------------------------------------- the packed operand, restated
def gemm_view(w, transposed, backward):
    """The weight blob as the matrix Wp[M x K] of the pass: the forward gather (Convolution forward, Deconvolution data gradient) reads the
    blob [rows][reduction channels][taps] as it is; the transposed gather (Convolution data gradient, Deconvolution forward) reads it with
    its two channel axes swapped.  K runs over (reduction channel, ky, kx), taps fastest."""
    swapped = bool(backward) != bool(transposed)
    m = w.transpose(1, 0, 2, 3) if swapped else w
    return np.ascontiguousarray(m).reshape(m.shape[0], -1)


def padded_dims(M, K):
    """(16-row groups, k-steps) of the operand: M rounded up to 16, K to 16 (whole chunks of four k-steps of 4)."""
    return -(-M // 16), 4 * -(-K // 16)


def pack_np(w, transposed, backward):
    """[groups][k-steps][64 lanes]: lane l of k-step ks of group g holds Wp[16 g + (l & 15)][4 ks + (l >> 4)], zero beyond M and K."""
    m = gemm_view(w, transposed, backward)
    G, ksteps = padded_dims(*m.shape)
    full = np.zeros((16 * G, 4 * ksteps), np.float32)
    full[:m.shape[0], :m.shape[1]] = m
    return np.ascontiguousarray(full.reshape(G, 16, ksteps, 4).transpose(0, 2, 3, 1)).reshape(G, ksteps, 64)


def unpack_np(packed, M, K):
    G, ksteps, _ = packed.shape
    full = packed.reshape(G, ksteps, 4, 16).transpose(0, 3, 1, 2).reshape(16 * G, 4 * ksteps)
    assert not full[M:].any() and not full[:, K:].any()
    return full[:M, :K]


def col_forward(inp, k, s, p, OH, OW):
    """[C k k, OH OW] of one sample: col[(c, ky, kx)][(y, x)] = inp[c][y s - p + ky][x s - p + kx], zero outside."""
    C, H, W = inp.shape
    col = np.zeros((C, k, k, OH, OW), inp.dtype)
    for ky in range(k):
        for kx in range(k):
            for y in range(OH):
                for x in range(OW):
                    yi, xi = y * s - p + ky, x * s - p + kx
                    if 0 <= yi < H and 0 <= xi < W:
                        col[:, ky, kx, y, x] = inp[:, yi, xi]
    return col.reshape(C * k * k, OH * OW)


def col_transposed(inp, k, s, p, OH, OW):
    """col[(c, ky, kx)][(y, x)] = inp[c][(y + p - ky) / s][(x + p - kx) / s] where both divisions are exact and inside the map."""
    C, H, W = inp.shape
    col = np.zeros((C, k, k, OH, OW), inp.dtype)
    for ky in range(k):
        for kx in range(k):
            for y in range(OH):
                for x in range(OW):
                    ty, tx = y + p - ky, x + p - kx
                    if ty >= 0 and tx >= 0 and ty % s == 0 and tx % s == 0 and ty // s < H and tx // s < W:
                        col[:, ky, kx, y, x] = inp[:, ty // s, tx // s]
    return col.reshape(C * k * k, OH * OW)
