"""What the tests of the general convolution over three spatial axes (include/flownet2_hip_conv_volume.h) share: the geometry rows, the fp64
reference (torch's double conv3d / conv_transpose3d with stride, padding, dilation and groups and their autograd on the CPU, computed once per
row) and a NumPy statement of the packed operand per group and of the two gathers with the depth digit.  Data conventions are those of
tests/conv_general_cases.py: unit-normal data, weights x 0.1, fixed seeds.

The largest K of a row here is 320 (the 4x4x4 deconvolution forward: 5 channels x 64 taps); the largest K among the rows of
tests/conv_general_cases.py is 2400 (the data gradient of 64 -> 96 with 5x5 taps; 2057 in a forward pass), so the error bounds derived in
tests/test_conv_general.py for those rows stand for these."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_general_cases import rand
from conv_geometry_cases import padded_dims, unpack_np      # (the per-group operand of a matrix does not care where K came from)

# (N, Cin, D, H, W, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw, group)
CONV = [
    (2, 3, 4, 5, 6, 5, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1),        # 3x3x3 / 1 / 1: K = 81 (a K tail); 5 < 16 rows
    (1, 4, 3, 7, 6, 6, 1, 3, 2, 1, 2, 1, 0, 1, 0, 1, 1, 1, 1),        # taps (1, 3, 2), stride (1, 2, 1), pad (0, 1, 0): every per-axis value differs
    (2, 3, 7, 5, 8, 4, 3, 2, 2, 2, 1, 1, 1, 0, 2, 2, 1, 3, 1),        # stride (2, 1, 1) with dilation (2, 1, 3): divisibility on the depth axis alone
    (1, 4, 3, 4, 5, 34, 2, 2, 2, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2),       # group 2 with 17 outputs per group: a row group boundary inside a group
    (2, 3, 4, 4, 5, 3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3),        # depthwise: group == Cin == Cout == 3
    (1, 20, 3, 4, 4, 6, 2, 2, 2, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1),       # 2x2x2 on 20 input channels: K = 160, ten whole chunks
    (2, 2, 3, 5, 7, 3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1),        # output volume of 3x5x7 = 105 voxels at batch 2: a tile straddling the end of a sample
    (1, 2, 3, 6, 5, 3, 5, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1),        # Din + 2 pd == ext: one output plane
]
DECONV = [                                                            # weight [Cin, Cout / group, kd, kh, kw]
    (2, 5, 2, 3, 4, 3, 4, 4, 4, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1),        # 4x4x4 / 2 / 1: a transposed volume layer
    (1, 3, 2, 3, 3, 4, 3, 3, 3, 3, 3, 3, 1, 1, 1, 2, 2, 2, 1),        # stride 3 and dilation 2
    (1, 4, 3, 4, 5, 3, 3, 2, 2, 2, 1, 1, 1, 0, 2, 2, 1, 3, 1),        # stride (2, 1, 1) with dilation (2, 1, 3), transposed
    (1, 4, 2, 3, 3, 6, 2, 3, 2, 1, 2, 1, 0, 1, 0, 1, 1, 1, 2),        # rectangular taps, group 2
]
ROWS = [(False,) + r for r in CONV] + [(True,) + r for r in DECONV]
GROUPED = ROWS[3]
# what the host refuses: Cin % group, Cout % group, dilation_d 0, a convolution whose dilated depth extent exceeds Din + 2 pad, a
# deconvolution with depth extent below 1, kernel_d 0, stride_d 0, negative pad_d, group 0, a blob beyond the 32-bit limits
INVALID = [
    (False, 1, 5, 4, 4, 4, 4, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2),
    (False, 1, 4, 4, 4, 4, 5, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2),
    (False, 1, 4, 4, 4, 4, 4, 3, 3, 3, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1),
    (False, 1, 4, 4, 8, 8, 4, 3, 3, 3, 1, 1, 1, 1, 1, 1, 3, 1, 1, 1),        # extent 7 > 4 + 2
    (True, 1, 4, 1, 4, 4, 4, 2, 2, 2, 1, 1, 1, 1, 0, 0, 1, 1, 1, 2),         # 1 (1 - 1) + 2 - 2 = 0
    (False, 1, 4, 4, 4, 4, 4, 0, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1),
    (False, 1, 4, 4, 4, 4, 4, 3, 3, 3, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1),
    (False, 1, 4, 4, 4, 4, 4, 3, 3, 3, 1, 1, 1, -1, 1, 1, 1, 1, 1, 1),
    (False, 1, 4, 4, 4, 4, 4, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0),
    (False, 1, 4, 1 << 10, 1 << 10, 1 << 10, 4, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2),
]


def row_id(row):
    return ("deconv" if row[0] else "conv") + "-" + "x".join(str(v) for v in row[1:])


def fields(row):
    """(transposed, N, Cin, size, Cout, kernel, stride, pad, dilation, group), the per-axis values as (d, h, w)."""
    return row[0], row[1], row[2], row[3:6], row[6], row[7:10], row[10:13], row[13:16], row[16:19], row[19]


def out_size(row):
    tr, N, Cin, size, Cout, kernel, stride, pad, dilation, group = fields(row)
    out = []
    for n, k, s, p, d in zip(size, kernel, stride, pad, dilation):
        ext = d * (k - 1) + 1
        out.append(s * (n - 1) + ext - 2 * p if tr else (n + 2 * p - ext) // s + 1)
    return tuple(out)


def weight_shape(row):
    tr, N, Cin, size, Cout, kernel, stride, pad, dilation, group = fields(row)
    return ((Cin, Cout // group) if tr else (Cout, Cin // group)) + tuple(kernel)


def layer64(x, w, b, row):
    tr, N, Cin, size, Cout, kernel, stride, pad, dilation, group = fields(row)
    return (F.conv_transpose3d if tr else F.conv3d)(x, w, b, stride=stride, padding=pad, dilation=dilation, groups=group)


@functools.lru_cache(maxsize=None)
def case(row):
    """float32 inputs of the row and the fp64 results: dict(x, w, b, g, top (with bias, no activation), top_nobias, gx, gw, gb)."""
    tr, N, Cin, size, Cout = fields(row)[:5]
    x, w, b = rand((N, Cin) + tuple(size), 1), rand(weight_shape(row), 2, 0.1), rand((Cout,), 3)
    g = rand((N, Cout) + out_size(row), 4)
    xt, wt, bt = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, b))
    top = layer64(xt, wt, bt, row)
    assert tuple(top.shape) == (N, Cout) + out_size(row)
    gx, gw, gb = torch.autograd.grad(top, (xt, wt, bt), torch.from_numpy(g).double())
    out = dict(x=x, w=w, b=b, g=g, top=top.detach().numpy(), top_nobias=(top.detach() - bt.detach().view(1, -1, 1, 1, 1)).numpy(), gx=gx.numpy(),
               gw=gw.numpy(), gb=gb.numpy())
    for a in out.values():
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- the packed operand, restated per group
def gemm_views(w, transposed, backward, group):
    """The weight blob [Cs][Cl / group][kd][kh][kw] as `group` matrices Wp[Mg x K_g] of the pass, as tests/conv_geometry_cases.py states
    them with one more digit: K runs over (reduction channel, kz, ky, kx), taps fastest, kz before ky before kx."""
    swapped = bool(backward) != bool(transposed)
    csg = w.shape[0] // group
    views = []
    for g in range(group):
        m = w[g * csg:(g + 1) * csg]
        m = m.transpose(1, 0, 2, 3, 4) if swapped else m
        views.append(np.ascontiguousarray(m).reshape(m.shape[0], -1))
    return views


def pack_np(w, transposed, backward, group):
    """[group][row groups][k-steps][64 lanes]: lane l of k-step ks of row group r holds Wp[16 r + (l & 15)][4 ks + (l >> 4)], zero beyond."""
    out = []
    for m in gemm_views(w, transposed, backward, group):
        G, ksteps = padded_dims(*m.shape)
        full = np.zeros((16 * G, 4 * ksteps), np.float32)
        full[:m.shape[0], :m.shape[1]] = m
        out.append(np.ascontiguousarray(full.reshape(G, 16, ksteps, 4).transpose(0, 2, 3, 1)).reshape(G, ksteps, 64))
    return np.stack(out)


def col_forward(inp, kernel, stride, pad, dilation, out):
    """[C kd kh kw, OD OH OW] of one sample: col[(c, kz, ky, kx)][(z, y, x)] = inp[c][z sd - pd + kz dd][y sh - ph + ky dh][x sw - pw + kx dw],
    zero outside the volume."""
    C = inp.shape[0]
    col = np.zeros((C,) + tuple(kernel) + tuple(out), inp.dtype)
    for k in np.ndindex(*kernel):
        for o in np.ndindex(*out):
            i = [o[a] * stride[a] - pad[a] + k[a] * dilation[a] for a in range(3)]
            if all(0 <= i[a] < inp.shape[1 + a] for a in range(3)):
                col[(slice(None),) + k + o] = inp[:, i[0], i[1], i[2]]
    return col.reshape(C * int(np.prod(kernel)), int(np.prod(out)))


def col_transposed(inp, kernel, stride, pad, dilation, out):
    """col[(c, kz, ky, kx)][(z, y, x)] = inp[c][(z + pd - kz dd) / sd][(y + ph - ky dh) / sh][(x + pw - kx dw) / sw] where all three
    divisions are exact and inside the volume."""
    C = inp.shape[0]
    col = np.zeros((C,) + tuple(kernel) + tuple(out), inp.dtype)
    for k in np.ndindex(*kernel):
        for o in np.ndindex(*out):
            t = [o[a] + pad[a] - k[a] * dilation[a] for a in range(3)]
            if all(t[a] >= 0 and t[a] % stride[a] == 0 and t[a] // stride[a] < inp.shape[1 + a] for a in range(3)):
                col[(slice(None),) + k + o] = inp[:, t[0] // stride[0], t[1] // stride[1], t[2] // stride[2]]
    return col.reshape(C * int(np.prod(kernel)), int(np.prod(out)))
