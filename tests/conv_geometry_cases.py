"""What the tests of the widened general convolution (include/flownet2_hip_conv_geometry.h: rectangular taps, per-axis stride / pad /
dilation, groups) share: the geometry rows, the fp64 reference (torch's double conv2d / conv_transpose2d with stride, padding, dilation and
groups and their autograd on the CPU, computed once per row) and a NumPy statement of the packed operand per group and of the two gathers.
Data conventions are those of tests/conv_general_cases.py: unit-normal data, weights x 0.1, fixed seeds."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_general_cases import rand

# (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group)
CONV = [
    (2, 3, 6, 11, 5, 1, 7, 1, 1, 0, 3, 1, 1, 1),        # 1x7 taps, pad on one axis only
    (2, 5, 9, 13, 18, 3, 2, 2, 3, 1, 0, 1, 1, 1),       # kh != kw, sh != sw, ph != pw; bottom pixels no tap reads; M tail over two row groups
    (1, 6, 9, 10, 7, 3, 3, 1, 1, 2, 2, 2, 2, 1),        # dilation 2, "same" padding
    (2, 4, 12, 9, 20, 3, 3, 2, 2, 1, 1, 3, 1, 1),       # dh != dw with stride 2: the transposed gather's divisibility test per axis
    (1, 2, 4, 4, 3, 3, 3, 1, 1, 4, 4, 4, 4, 1),         # dilated extent (9) larger than the image
    (2, 6, 7, 8, 10, 3, 3, 1, 1, 1, 1, 1, 1, 2),        # group 2, 5 rows per group: two groups must not share a row group
    (1, 8, 6, 6, 40, 3, 3, 2, 2, 1, 1, 1, 1, 2),        # 20 rows per group: two row groups per group, the second ragged
    (2, 19, 8, 9, 19, 3, 3, 1, 1, 1, 1, 1, 1, 19),      # depthwise: M = 1, K = 9, below one chunk
    (1, 4, 6, 7, 12, 5, 5, 2, 2, 2, 2, 1, 1, 4),        # depthwise with channel multiplier 3
    (2, 6, 11, 14, 9, 2, 3, 2, 1, 1, 2, 2, 3, 3),       # everything at once
    (1, 4, 3, 70, 4, 1, 3, 1, 2, 0, 1, 1, 1, 2),        # a 64-pixel tile that wraps rows, with groups
]
DECONV = [                                              # weight [Cin, Cout / group, kh, kw]
    (2, 5, 4, 6, 3, 4, 2, 2, 1, 1, 0, 1, 1, 1),         # rectangular taps and strides
    (1, 3, 5, 5, 4, 3, 3, 2, 2, 1, 1, 2, 2, 1),         # dilation 2
    (2, 4, 4, 5, 6, 4, 4, 2, 2, 1, 1, 1, 1, 2),         # FlowNet's taps, group 2
    (1, 6, 3, 4, 9, 3, 2, 3, 2, 0, 1, 1, 2, 3),         # stride 3 x 2, dilation on one axis, group 3
    (1, 5, 4, 4, 5, 4, 4, 2, 2, 1, 1, 1, 1, 5),         # FCN bilinear upsampling: group == channels
]
ROWS = [(False,) + r for r in CONV] + [(True,) + r for r in DECONV]
# what the host refuses: group 0, Cin % group, Cout % group, dilation 0, kernel_w 0, stride_h 0, negative pad_w, a convolution whose dilated
# extent exceeds H + 2 pad, a deconvolution with output extent below 1, a blob beyond the 32-bit limits
INVALID = [
    (False, 1, 4, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 0),
    (False, 1, 5, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 2),
    (False, 1, 4, 8, 8, 5, 3, 3, 1, 1, 1, 1, 1, 1, 2),
    (False, 1, 4, 8, 8, 4, 3, 3, 1, 1, 1, 1, 0, 1, 1),
    (False, 1, 4, 8, 8, 4, 3, 0, 1, 1, 1, 1, 1, 1, 1),
    (False, 1, 4, 8, 8, 4, 3, 3, 0, 1, 1, 1, 1, 1, 1),
    (False, 1, 4, 8, 8, 4, 3, 3, 1, 1, 1, -1, 1, 1, 1),
    (False, 1, 4, 8, 8, 4, 3, 3, 1, 1, 1, 1, 5, 1, 1),         # extent 11 > 8 + 2
    (True, 1, 4, 1, 1, 4, 2, 2, 1, 1, 1, 1, 1, 1, 2),          # 1 (1 - 1) + 2 - 2 = 0
    (False, 1, 4, 1 << 20, 1 << 20, 4, 3, 3, 1, 1, 1, 1, 1, 1, 2),
]


def row_id(row):
    return ("deconv" if row[0] else "conv") + "-" + "x".join(str(v) for v in row[1:])


def out_hw(row):
    tr, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group = row
    eh, ew = dh * (kh - 1) + 1, dw * (kw - 1) + 1
    return (sh * (H - 1) + eh - 2 * ph, sw * (W - 1) + ew - 2 * pw) if tr else ((H + 2 * ph - eh) // sh + 1, (W + 2 * pw - ew) // sw + 1)


def weight_shape(row):
    tr, N, Cin, H, W, Cout, kh, kw = row[:8]
    group = row[14]
    return (Cin, Cout // group, kh, kw) if tr else (Cout, Cin // group, kh, kw)


def layer64(x, w, b, row):
    tr, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group = row
    return (F.conv_transpose2d if tr else F.conv2d)(x, w, b, stride=(sh, sw), padding=(ph, pw), dilation=(dh, dw), groups=group)


@functools.lru_cache(maxsize=None)
def case(row):
    """float32 inputs of the row and the fp64 results: dict(x, w, b, g, top (with bias, no activation), top_nobias, gx, gw, gb)."""
    tr, N, Cin, H, W, Cout = row[:6]
    Ho, Wo = out_hw(row)
    x, w, b = rand((N, Cin, H, W), 1), rand(weight_shape(row), 2, 0.1), rand((Cout,), 3)
    g = rand((N, Cout, Ho, Wo), 4)
    xt, wt, bt = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, b))
    top = layer64(xt, wt, bt, row)
    assert tuple(top.shape) == (N, Cout, Ho, Wo)
    gx, gw, gb = torch.autograd.grad(top, (xt, wt, bt), torch.from_numpy(g).double())
    out = dict(x=x, w=w, b=b, g=g, top=top.detach().numpy(), top_nobias=(top.detach() - bt.detach().view(1, -1, 1, 1)).numpy(), gx=gx.numpy(),
               gw=gw.numpy(), gb=gb.numpy())
    for a in out.values():
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- the packed operand, restated per group
def gemm_views(w, transposed, backward, group):
    """The weight blob [Cs][Cl / group][kh][kw] as `group` matrices Wp[Mg x K_g] of the pass.  The rows [g Cs / group, ...) of the blob are
    group g.  The forward gather (Convolution forward, Deconvolution data gradient) reads them as they are: Mg = Cs / group, K_g = (Cl /
    group) kh kw; the transposed gather (Convolution data gradient, Deconvolution forward) with the two channel axes swapped: Mg = Cl /
    group, K_g = (Cs / group) kh kw.  K runs over (reduction channel, ky, kx), taps fastest, ky before kx."""
    swapped = bool(backward) != bool(transposed)
    csg = w.shape[0] // group
    views = []
    for g in range(group):
        m = w[g * csg:(g + 1) * csg]
        m = m.transpose(1, 0, 2, 3) if swapped else m
        views.append(np.ascontiguousarray(m).reshape(m.shape[0], -1))
    return views


def padded_dims(M, K):
    """(16-row groups, k-steps) of one group's operand: M rounded up to 16, K to 16 (whole chunks of four k-steps of 4)."""
    return -(-M // 16), 4 * -(-K // 16)


def pack_np(w, transposed, backward, group):
    """[group][row groups][k-steps][64 lanes]: lane l of k-step ks of row group r holds Wp[16 r + (l & 15)][4 ks + (l >> 4)], zero beyond."""
    out = []
    for m in gemm_views(w, transposed, backward, group):
        G, ksteps = padded_dims(*m.shape)
        full = np.zeros((16 * G, 4 * ksteps), np.float32)
        full[:m.shape[0], :m.shape[1]] = m
        out.append(np.ascontiguousarray(full.reshape(G, 16, ksteps, 4).transpose(0, 2, 3, 1)).reshape(G, ksteps, 64))
    return np.stack(out)


def unpack_np(packed, M, K):
    """One group's [row groups][k-steps][64] back to Wp[M x K]; the padding must be zero."""
    G, ksteps, _ = packed.shape
    full = packed.reshape(G, ksteps, 4, 16).transpose(0, 3, 1, 2).reshape(16 * G, 4 * ksteps)
    assert not full[M:].any() and not full[:, K:].any()
    return full[:M, :K]


def col_forward(inp, kh, kw, sh, sw, ph, pw, dh, dw, OH, OW):
    """[C kh kw, OH OW] of one sample: col[(c, ky, kx)][(y, x)] = inp[c][y sh - ph + ky dh][x sw - pw + kx dw], zero outside."""
    C, H, W = inp.shape
    col = np.zeros((C, kh, kw, OH, OW), inp.dtype)
    for ky in range(kh):
        for kx in range(kw):
            for y in range(OH):
                for x in range(OW):
                    yi, xi = y * sh - ph + ky * dh, x * sw - pw + kx * dw
                    if 0 <= yi < H and 0 <= xi < W:
                        col[:, ky, kx, y, x] = inp[:, yi, xi]
    return col.reshape(C * kh * kw, OH * OW)


def col_transposed(inp, kh, kw, sh, sw, ph, pw, dh, dw, OH, OW):
    """col[(c, ky, kx)][(y, x)] = inp[c][(y + ph - ky dh) / sh][(x + pw - kx dw) / sw] where both divisions are exact and inside the map."""
    C, H, W = inp.shape
    col = np.zeros((C, kh, kw, OH, OW), inp.dtype)
    for ky in range(kh):
        for kx in range(kw):
            for y in range(OH):
                for x in range(OW):
                    ty, tx = y + ph - ky * dh, x + pw - kx * dw
                    if ty >= 0 and tx >= 0 and ty % sh == 0 and tx % sw == 0 and ty // sh < H and tx // sw < W:
                        col[:, ky, kx, y, x] = inp[:, ty // sh, tx // sw]
    return col.reshape(C * kh * kw, OH * OW)
