"""Independent fp64 re-derivations of the hot-path ops, written from the MATH in SURVEY.md Appendix A
(not from the kernels), used to cross-check the C oracle.  torch.float64 + autograd gives the
gradients the backward kernels must reproduce."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F


def corr_shape(H, W, pad, K, md, s1, s2):
    kr = (K - 1) // 2
    border = md + kr
    topH = math.ceil((H + 2 * pad - 2 * border) / s1)
    topW = math.ceil((W + 2 * pad - 2 * border) / s1)
    ngr = md // s2
    return (2 * ngr + 1) ** 2, topH, topW, ngr


def correlation(b0: torch.Tensor, b1: torch.Tensor, pad, K, md, s1, s2, subtract=False) -> torch.Tensor:
    """top[n,(q,o),y,x] = 1/(K*K*C) * sum_{j,i,c} P0[n,c,y1+j,x1+i] (*|-) P1[n,c,y1+j+q*s2,x1+i+o*s2]
    with y1 = y*s1 + md, x1 = x*s1 + md in PADDED coordinates (Appendix A.1)."""
    N, C, H, W = b0.shape
    topC, topH, topW, ngr = corr_shape(H, W, pad, K, md, s1, s2)
    P0 = F.pad(b0, (pad, pad, pad, pad))
    P1 = F.pad(b1, (pad, pad, pad, pad))
    outs = []
    for q in range(-ngr, ngr + 1):
        for o in range(-ngr, ngr + 1):
            acc = 0
            for j in range(K):
                for i in range(K):
                    ys = md + j
                    xs = md + i
                    a = P0[:, :, ys: ys + (topH - 1) * s1 + 1: s1, xs: xs + (topW - 1) * s1 + 1: s1]
                    b = P1[:, :, ys + q * s2: ys + q * s2 + (topH - 1) * s1 + 1: s1,
                           xs + o * s2: xs + o * s2 + (topW - 1) * s1 + 1: s1]
                    acc = acc + ((a - b).abs().sum(1) if subtract else (a * b).sum(1))
            outs.append(acc / (K * K * C))
    return torch.stack(outs, 1)


def correlation1d(b0: torch.Tensor, b1: torch.Tensor, pad, K, md, s1, s2, single_direction=0, subtract=False) -> torch.Tensor:
    """Horizontal cost volume: top[n,c,y,x] = 1/(K*K*C) * sum_{j,i,ch} P0[n,ch,y*s1+j,x1+i] (*|-) P1[n,ch,y*s1+j,x1+i+(c+x_shift)*s2],
    x1 = x*s1 + md in x-PADDED coordinates (padding in x only); x_shift = -md//s2 (both), 0 (right), -(md//s2 + 1) (left).
    Positions outside the padded row count as zeros (what the reference's flat indexing reads whenever pad >= the overshoot)."""
    N, C, H, W = b0.shape
    kr = (K - 1) // 2
    ngr = md // s2
    ngw = ngr + 1 if single_direction != 0 else 2 * ngr + 1
    xshift = -ngw if single_direction == -1 else (0 if single_direction == 1 else -ngr)
    topW = math.ceil((W + 2 * pad - 2 * (md + kr)) / s1)
    topH = math.ceil((H - 2 * kr) / s1)
    extra = max(0, -(md + xshift * s2))          # left mode starts one grid step beyond the radius
    P0 = F.pad(b0, (pad + extra, pad, 0, 0))
    P1 = F.pad(b1, (pad + extra, pad, 0, 0))
    outs = []
    for c in range(ngw):
        d = (c + xshift) * s2
        acc = 0
        for j in range(K):
            for i in range(K):
                xs = md + i + extra
                a = P0[:, :, j: j + (topH - 1) * s1 + 1: s1, xs: xs + (topW - 1) * s1 + 1: s1]
                b = P1[:, :, j: j + (topH - 1) * s1 + 1: s1, xs + d: xs + d + (topW - 1) * s1 + 1: s1]
                acc = acc + ((a - b).abs().sum(1) if subtract else (a * b).sum(1))
        outs.append(acc / (K * K * C))
    return torch.stack(outs, 1)


def flow_warp(image: torch.Tensor, flow: torch.Tensor, fill=0.0, fp32_positions=False) -> torch.Tensor:
    """Appendix A.3: bilinear sample at (x+u, y+v), right/bottom neighbour clamped, fill outside.
    fp32_positions: x + u and y + v are rounded to fp32 first, as flow_warp_layer.cu:73-74 does; everything after that
    stays in image.dtype (no gradient reaches the flow through the rounding)."""
    N, C, H, W = image.shape
    if fp32_positions:
        x2, y2 = (t.to(image.dtype) for t in _positions_fp32(flow))
    else:
        ys, xs = torch.meshgrid(torch.arange(H, dtype=image.dtype), torch.arange(W, dtype=image.dtype), indexing="ij")
        x2 = xs[None] + flow[:, 0]
        y2 = ys[None] + flow[:, 1]
    inb = (x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H)
    x2c = torch.where(inb, x2, torch.zeros_like(x2))
    y2c = torch.where(inb, y2, torch.zeros_like(y2))
    xl = x2c.detach().floor().long()
    yt = y2c.detach().floor().long()
    xr = torch.clamp(xl + 1, max=W - 1)
    yb = torch.clamp(yt + 1, max=H - 1)
    a = (x2c - xl)[:, None]
    b = (y2c - yt)[:, None]
    flat = image.reshape(N, C, H * W)

    def g(yy, xx):
        idx = (yy * W + xx).reshape(N, 1, H * W).expand(N, C, H * W)
        return torch.gather(flat, 2, idx).reshape(N, C, H, W)

    out = (1 - a) * (1 - b) * g(yt, xl) + a * (1 - b) * g(yt, xr) + (1 - a) * b * g(yb, xl) + a * b * g(yb, xr)
    return torch.where(inb[:, None], out, torch.full_like(out, fill))


def _positions_fp32(flow):
    """x2 = fp32(x + u), y2 = fp32(y + v): the sample positions of flow_warp_layer.cu:73-74 (and :184-185), [N,H,W] each."""
    f = torch.as_tensor(flow).detach().to(torch.float32)
    H, W = f.shape[2:]
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    return xs + f[:, 0], ys + f[:, 1]


def flow_warp_backward(image, flow, g, propagate_image=True, propagate_flow=True):
    """fp64 statement of flow_warp_backward_kernel_no_smem (flow_warp_layer.cu:169-229).  Sample positions are rounded to fp32 as
    the reference does (:184-185); everything after them is fp64.

    image gradient: every in-image source pixel adds g * w_k to each of its four taps (:197-200), clamped right / bottom taps that
                    coincide with another tap included (each is a term of its own: an infinite g on a tap of weight 0 gives NaN);
    flow gradient:  du = sum_c g_c * (gy * (TR - TL) + (1 - gy) * (BR - BL)),  gy = iyB - y2   (:203-214)
                    dv = sum_c g_c * (gx * (BL - TL) + (1 - gx) * (BR - TR)),  gx = ixR - x2   (:216-227)
                    -- at the clamped last row / column this is the reference's formula, not the derivative of the forward;
    pixels whose sample falls outside the image contribute nothing and get a flow gradient of 0.

    Returns (di, df, di_abs, di_terms, df_abs, df_terms) as float64 tensors: the gradients, and for each element the fp64 sum of
    the |terms| that were added into it and their number -- what an elementwise rounding-error bound needs.  In df_abs the factor
    (1 - gy) counts as |1 - gy| + |gy| (and (1 - gx) likewise): fp32 forms it from gy, which is rounded by up to u|gy| when y2 is
    just above an integer, so the absolute error of 1 - gy is not relative to its own size."""
    image = torch.as_tensor(image).detach().to(torch.float64)
    g = torch.as_tensor(g).detach().to(torch.float64)
    N, C, H, W = image.shape
    HW = H * W
    x2, y2 = _positions_fp32(flow)
    inb = (x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H)
    x2 = torch.where(inb, x2.double(), torch.zeros((), dtype=torch.float64))
    y2 = torch.where(inb, y2.double(), torch.zeros((), dtype=torch.float64))
    xl, yt = x2.floor().long(), y2.floor().long()                     # (int) of a non-negative position
    xr, yb = torch.clamp(xl + 1, max=W - 1), torch.clamp(yt + 1, max=H - 1)
    a, b = x2 - xl, y2 - yt
    zero = torch.zeros((), dtype=torch.float64)
    mask = inb[:, None]

    di = torch.zeros((N, C, HW), dtype=torch.float64)
    di_abs = torch.zeros_like(di)
    di_terms = torch.zeros((N, HW), dtype=torch.float64)
    if propagate_image:
        for yy, xx, w in ((yt, xl, (1 - a) * (1 - b)), (yt, xr, a * (1 - b)), (yb, xl, (1 - a) * b), (yb, xr, a * b)):
            idx = (yy * W + xx).reshape(N, HW)
            term = torch.where(mask, g * w[:, None], zero).reshape(N, C, HW)     # where, not *: an outside g never reaches a cell
            ic = idx[:, None].expand(N, C, HW)
            di.scatter_add_(2, ic, term)
            di_abs.scatter_add_(2, ic, term.abs())
            di_terms.scatter_add_(1, idx, inb.reshape(N, HW).double())
    di_terms = di_terms[:, None].expand(N, C, HW)

    df = torch.zeros((N, 2, H, W), dtype=torch.float64)
    df_abs = torch.zeros_like(df)
    df_terms = torch.zeros_like(df)
    if propagate_flow:
        flat = image.reshape(N, C, HW)

        def tap(yy, xx):
            return torch.gather(flat, 2, (yy * W + xx).reshape(N, 1, HW).expand(N, C, HW)).reshape(N, C, H, W)

        TL, TR, BL, BR = tap(yt, xl), tap(yt, xr), tap(yb, xl), tap(yb, xr)
        gy = (yb - y2)[:, None]
        gx = (xr - x2)[:, None]
        for k, (gk, d0, d1) in enumerate(((gy, TR - TL, BR - BL), (gx, BL - TL, BR - TR))):
            # g * (t0 + t1) as the reference groups it (:207-211): an infinite g meets the channel's temp once
            df[:, k] = torch.where(mask, g * (gk * d0 + (1 - gk) * d1), zero).sum(1)
            # fp32 gy = iyB - y2 is rounded (by up to u|gy|) before 1 - gy is formed from it: the second factor counts |1-gy| + |gy|
            df_abs[:, k] = torch.where(mask, g.abs() * (gk.abs() * d0.abs() + ((1 - gk).abs() + gk.abs()) * d1.abs()), zero).sum(1)
            df_terms[:, k] = torch.where(inb, 2.0 * C, 0.0)
    return (di.reshape(N, C, H, W), df, di_abs.reshape(N, C, H, W), di_terms.reshape(N, C, H, W), df_abs, df_terms)


def _tri(t):
    return np.where((t >= -1) & (t < 0), t + 1, np.where((t >= 0) & (t <= 1), 1 - t, 0.0))


def _cub(t):
    x = np.abs(t)
    return np.where(x <= 1, x * x * (1.5 * x - 2.5) + 1, np.where(x < 2, x * (x * (-0.5 * x + 2.5) - 4) + 2, 0.0))


def resample(x: np.ndarray, Hout, Wout, kind="linear", antialias=True) -> np.ndarray:
    """Appendix A.5 in float64 (including the fx/fy swap of the half-pixel offsets)."""
    N, C, Hin, Win = x.shape
    fx = np.float32(Win) / np.float32(Wout)
    fy = np.float32(Hin) / np.float32(Hout)
    fx, fy = float(fx), float(fy)
    out = np.zeros((N, C, Hout, Wout))
    aa = ((fx > 1) or (fy > 1)) and antialias
    ax = 1.0 / (fx if aa else 1.0)
    ay = 1.0 / (fy if aa else 1.0)
    kw = 4 if kind == "cubic" else 2
    rx = 2 if fx < 1 else math.ceil(kw / ax)
    ry = 2 if fy < 1 else math.ceil(kw / ay)
    k = _cub if kind == "cubic" else _tri
    for yo in range(Hout):
        y_in = yo * fy + fx / 2 - 0.5
        yr = int(math.floor(abs(y_in) + 0.5) * (1 if y_in >= 0 else -1))
        for xo in range(Wout):
            x_in = xo * fx + fy / 2 - 0.5
            xr = int(math.floor(abs(x_in) + 0.5) * (1 if x_in >= 0 else -1))
            if kind == "nearest":
                out[:, :, yo, xo] = x[:, :, min(max(yr, 0), Hin - 1), min(max(xr, 0), Win - 1)]
                continue
            ys = np.arange(max(yr - ry, 0), min(yr + ry, Hin - 1) + 1)
            xs = np.arange(max(xr - rx, 0), min(xr + rx, Win - 1) + 1)
            wy = ay * k(ay * (y_in - ys))
            wx = ax * k(ax * (x_in - xs))
            w = wy[:, None] * wx[None, :]
            ws = w.sum()
            if ws == 0:
                continue
            out[:, :, yo, xo] = (x[:, :, ys[0]: ys[-1] + 1, xs[0]: xs[-1] + 1] * w).sum((2, 3)) / ws
    return out


def l1loss(b0: torch.Tensor, b1, l2_per_location, l2_prescale, normalize_by_num_entries, epsilon, plateau):
    """Appendix A.6.  Returns (loss, normalize_coeff)."""
    d = b0 - b1 if b1 is not None else b0
    N, C = d.shape[:2]
    mask = ~torch.isnan(d)
    norm = mask.sum().to(d.dtype) / C if normalize_by_num_entries else torch.tensor(float(N), dtype=d.dtype)
    d = torch.where(mask, d, torch.zeros_like(d))
    if l2_per_location:
        w = 1.0 / C if l2_prescale else 1.0
        s = (d * d).sum(1) * w
        if plateau > 0:
            s = torch.where(s.detach() < plateau * plateau, torch.zeros_like(s), s)
        e = torch.sqrt(s + epsilon)
        return e.sum() / norm, norm
    if plateau > 0:
        d = torch.where(d.detach().abs() < plateau, torch.zeros_like(d), d)
    return d.abs().sum() / norm, norm


def channel_norm(x: torch.Tensor) -> torch.Tensor:
    return torch.sqrt((x * x).sum(1, keepdim=True))


def downsample(x: np.ndarray, Hout, Wout) -> np.ndarray:
    """Appendix A.8."""
    N, C, Hin, Win = x.shape
    if (Hin, Win) == (Hout, Wout):
        return x.astype(np.float64)
    ws = np.float32(Win - 1) / np.float32(Wout - 1)
    hs = np.float32(Hin - 1) / np.float32(Hout - 1)
    wr, hr = math.ceil(ws), math.ceil(hs)
    out = np.zeros((N, C, Hout, Wout))
    for dy in range(Hout):
        boty = float(np.float32(np.float32(dy) / np.float32(Hout - 1)) * np.float32(Hin - 1))
        iy = int(math.floor(boty + 0.5))
        for dx in range(Wout):
            botx = float(np.float32(np.float32(dx) / np.float32(Wout - 1)) * np.float32(Win - 1))
            ix = int(math.floor(botx + 0.5))
            val = np.zeros((N, C))
            wsum = np.zeros((N, C))
            nansum = np.zeros((N, C))
            for by in range(iy - hr, iy + hr + 1):
                for bx in range(ix - wr, ix + wr + 1):
                    if 0 <= bx < Win and 0 <= by < Hin:
                        s = x[:, :, by, bx].astype(np.float64)
                        w = max(0.0, 1 - abs(bx - botx) / float(ws)) * max(0.0, 1 - abs(by - boty) / float(hs))
                        isn = np.isnan(s)
                        nansum += np.where(isn, w, 0.0)
                        val += np.where(isn, 0.0, s * w)
                        wsum += np.where(isn, 0.0, w)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = val / wsum
                r[(nansum / wsum) > 0.5] = np.nan
            out[:, :, dy, dx] = r
    return out


# ---- elementwise fp64 statements of Resample / Downsample / ChannelNorm (tests/test_resample.py, test_downsample_channel_norm.py) ----
# Positions and scale factors are rounded to fp32 exactly as the host functions and kernels round them (so that the statement picks
# the same window and the same taps); coefficients, products, sums and the division are fp64.  Each statement also returns, per
# output element, the quantities an elementwise rounding-error bound needs.

_U = 2.0 ** -24
_F32 = np.float32


def _roundf(v):
    """C roundf (half away from zero) of fp32 values, as int64."""
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def resample_geometry(Hin, Win, Hout, Wout, kind="linear", antialias=True):
    """fx, fy, ax, ay (fp32) and rx, ry as fn2_resample_forward_slices forms them (resample_layer.cu:146-147, :71-74, :179-185)."""
    fx, fy = _F32(Win) / _F32(Wout), _F32(Hin) / _F32(Hout)
    aa = bool((fx > 1) or (fy > 1)) and bool(antialias)
    ax = _F32(1) / (fx if aa else _F32(1))
    ay = _F32(1) / (fy if aa else _F32(1))
    kw = _F32(4 if kind == "cubic" else 2)
    rx = 2 if fx < 1 else int(np.ceil(kw / ax))
    ry = 2 if fy < 1 else int(np.ceil(kw / ay))
    return dict(fx=fx, fy=fy, ax=ax, ay=ay, rx=rx, ry=ry)


def resample_positions(n_out, f_own, f_other):
    """fp32(fp32(fp32(o * f_own) + fp32(f_other / 2)) - 0.5), uncontracted: x_in uses (fx, fy), y_in (fy, fx) -- the reference's swap."""
    o = np.arange(n_out, dtype=_F32)
    return (o * _F32(f_own) + _F32(f_other) / _F32(2)) - _F32(0.5)


def _coeff32(t32, kind):
    """The kernels' fp32 coefficient of an fp32 argument, operation by operation (resample.hip is compiled without contraction, and
    numpy rounds every fp32 operation): bicubic_coeff / triangle_coeff of resample_layer.cu:14-33."""
    t32 = np.asarray(t32, _F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == "cubic":
            x = np.abs(t32)
            p1 = x * x * (_F32(1.5) * x - _F32(2.5)) + _F32(1)
            p2 = x * (x * (_F32(-0.5) * x + _F32(2.5)) - _F32(4)) + _F32(2)
            return np.where(x <= 1, p1, np.where(x < 2, p2, _F32(0)))
        return np.where((t32 >= -1) & (t32 < 0), t32 + _F32(1), np.where((t32 >= 0) & (t32 <= 1), _F32(1) - t32, _F32(0)))


def _axis_table(n_in, n_out, f_own, f_other, a, r, kind):
    """Per output index of one axis: tap indices [n_out, 2r+1] (clamped into the image), their in-image mask, the fp64 coefficient
    a * k(a * (pos - tap)) (0 for a tap outside), the part `e` of its fp32 error that is NOT relative to it (in absolute units), and
    whether fp32 and fp64 disagree on an in-image tap's coefficient being 0 (a tap on a zero of the kernel: |t| = 1 or 2)."""
    pos = resample_positions(n_out, f_own, f_other)
    centre = _roundf(pos)
    taps = centre[:, None] + np.arange(-r, r + 1)[None]
    ok = (taps >= 0) & (taps < n_in)
    a32, a = _F32(a), float(a)
    t = a * (pos.astype(np.float64)[:, None] - taps)
    k = _cub(t) if kind == "cubic" else _tri(t)
    # the coefficient the kernels form from the same fp32 position: k32(fp32(a * fp32(pos - tap))).  e = |k32 - k| is the part of a
    # weight's fp32 error that is not relative to the weight (the argument's two roundings, the cancellation of 1 - |t| and of the
    # cubic polynomial near its zeros); `edge`: fp32 and fp64 disagree on whether the coefficient is 0.
    with np.errstate(over="ignore", invalid="ignore"):
        k32 = _coeff32(a32 * (pos.astype(_F32)[:, None] - taps.astype(_F32)), kind).astype(np.float64)
    e = np.abs(k32 - k)
    edge = (k32 == 0) != (k == 0)
    w = np.where(ok, a * k, 0.0)
    e = np.where(ok, a * e, 0.0)
    live = ok & ((k != 0) | (k32 != 0))                              # a coefficient of exactly 0 adds +0 exactly: no rounding
    return dict(idx=np.clip(taps, 0, n_in - 1), ok=ok, w=w, e=e, edge=(edge & ok).any(1), pos=pos, centre=centre, live=live.sum(1))


def _sep(x, tab, weights, axis):
    """sum_k weights[o, k] * x[..., tap(o, k), ...] along `axis` (taps outside the image contribute a 0 sample, NOT 0 * a clamped one).
    Lines of finite samples go through one matrix product; a line with a NaN / Inf is gathered tap by tap, so that only the taps of
    an output's own window can poison it."""
    x = np.moveaxis(x, axis, -1)
    n_out, K = tab["idx"].shape
    w = np.where(tab["ok"], weights, 0.0)
    M = np.zeros((n_out, x.shape[-1]))
    np.add.at(M, (np.repeat(np.arange(n_out), K), tab["idx"].ravel()), w.ravel())
    fin = np.isfinite(x).all(-1)
    out = np.empty(x.shape[:-1] + (n_out,))
    out[fin] = x[fin] @ M.T
    if not fin.all():
        out[~fin] = (np.where(tab["ok"], x[~fin][..., tab["idx"]], 0.0) * weights).sum(-1)       # [lines, n_out, K]
    return np.moveaxis(out, -1, axis)


def resample_statement(x, Hout, Wout, kind="linear", antialias=True, in_scale=1.0):
    """Resample (resample_layer.cu:39-95) per output element in fp64 over the in-image taps of the kernel's own window.

    fx, fy, ax, ay, rx, ry and the source positions are fp32 as the host function and the kernels form them; `in_scale` rounds every
    tap to fp32(tap * in_scale) first (the folded Eltwise).

    Returns a dict of float64 arrays -- per element [N,C,Hout,Wout]: ref, A = sum |w tap|, Ae = sum |e_w tap| (e_w: the part of a
    weight's fp32 error that is not relative to the weight); hull() -> (min, max) of the window's taps, computed on demand;
    per pixel [Hout,Wout]: ws = sum w, Aw = sum |w|, Awe = sum e_w, m = the number of in-image taps with a non-zero coefficient,
    taps = the number of in-image taps, edge = fp32 and fp64 disagree on whether the weight of some in-image tap is 0 (a tap exactly
    on the edge of the support), xr / yr = the window centres."""
    x = np.ascontiguousarray(x, np.float32)
    if in_scale != 1.0:
        x = x * _F32(in_scale)
    N, C, Hin, Win = x.shape
    g = resample_geometry(Hin, Win, Hout, Wout, kind, antialias)
    tx = _axis_table(Win, Wout, g["fx"], g["fy"], g["ax"], g["rx"], kind)          # x_in takes fy / 2 and y_in fx / 2: the reference's swap
    ty = _axis_table(Hin, Hout, g["fy"], g["fx"], g["ay"], g["ry"], kind)
    xd, xa = x.astype(np.float64), np.abs(x.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        sx = _sep(xd, tx, tx["w"], 3)
        sxa, sxe = _sep(xa, tx, np.abs(tx["w"]), 3), _sep(xa, tx, tx["e"], 3)
        num = _sep(sx, ty, ty["w"], 2)
        A = _sep(sxa, ty, np.abs(ty["w"]), 2)
        Ae = _sep(sxe, ty, np.abs(ty["w"]), 2) + _sep(sxa, ty, ty["e"], 2)
    ws = ty["w"].sum(1)[:, None] * tx["w"].sum(1)[None]
    Aw = np.abs(ty["w"]).sum(1)[:, None] * np.abs(tx["w"]).sum(1)[None]
    Awe = (np.abs(ty["w"]).sum(1)[:, None] * tx["e"].sum(1)[None] + ty["e"].sum(1)[:, None] * np.abs(tx["w"]).sum(1)[None])
    m = ty["live"][:, None] * tx["live"][None]
    taps = ty["ok"].sum(1)[:, None] * tx["ok"].sum(1)[None]

    def hull(fn, fill):
        v = np.moveaxis(xd, 3, -1)
        v = fn(np.where(tx["ok"], v[..., tx["idx"]], fill), -1)          # [N,C,Hin,Wout]
        v = np.moveaxis(v, 2, -1)
        v = fn(np.where(ty["ok"], v[..., ty["idx"]], fill), -1)          # [N,C,Wout,Hout]
        return np.swapaxes(v, 2, 3)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ref = np.where(ws == 0, 0.0, num / np.where(ws == 0, 1.0, ws))
    return dict(ref=ref, ws=ws, A=A, Aw=Aw, Ae=Ae, Awe=Awe, m=m, hull=lambda: (hull(np.min, np.inf), hull(np.max, -np.inf)),
                edge=ty["edge"][:, None] | tx["edge"][None], taps=taps, geometry=g, xr=tx["centre"], yr=ty["centre"])


def resample_nearest(x, Hout, Wout, in_scale=1.0):
    """NEAREST (resample_layer.cu:117-123, the index clamped into the image): a bitwise statement, fp32 in and out."""
    x = np.ascontiguousarray(x, np.float32)
    if in_scale != 1.0:
        x = x * _F32(in_scale)
    Hin, Win = x.shape[2:]
    g = resample_geometry(Hin, Win, Hout, Wout)
    xr = np.clip(_roundf(resample_positions(Wout, g["fx"], g["fy"])), 0, Win - 1)
    yr = np.clip(_roundf(resample_positions(Hout, g["fy"], g["fx"])), 0, Hin - 1)
    return x[:, :, yr[:, None], xr[None]]


def downsample_geometry(Hin, Win, Hout, Wout):
    """widthScale, heightScale (fp32), the radii, and per output column / row botx / boty (fp32), the rounded centre and the clipped
    tap range [x0, x1] / [y0, y1]: down_plan and downsample_thread_body (downsample_layer.cu:104-108, :27-31)."""
    ws, hs = _F32(Win - 1) / _F32(Wout - 1), _F32(Hin - 1) / _F32(Hout - 1)
    wr, hr = int(np.ceil(ws)), int(np.ceil(hs))
    botx = (np.arange(Wout, dtype=_F32) / _F32(Wout - 1)) * _F32(Win - 1)
    boty = (np.arange(Hout, dtype=_F32) / _F32(Hout - 1)) * _F32(Hin - 1)
    ix, iy = _roundf(botx), _roundf(boty)
    return dict(ws=ws, hs=hs, wr=wr, hr=hr, botx=botx, boty=boty,
                x0=np.maximum(ix - wr, 0), x1=np.minimum(ix + wr, Win - 1), y0=np.maximum(iy - hr, 0), y1=np.minimum(iy + hr, Hin - 1))


def downsample_weights(Hin, Win, Hout, Wout):
    """fp64 tap weights of every output row / column from the fp32 positions and scales: wy [Hout,Hin], wx [Wout,Win] (0 outside the
    window), and ey / ex = |w32 - w|, where w32 is the weight the kernels form in fp32 from the same position, operation by operation
    (fmaxf(0, 1 - fabsf(tap - bot) / scale), :52): the rounding of tap - bot, of the division and the cancellation in 1 - q move a
    weight by up to 2u q whatever its size -- the part of its error that is not relative to it."""
    g = downsample_geometry(Hin, Win, Hout, Wout)

    def axis(n_in, bot, lo, hi, scale):
        t = np.arange(n_in)[None]
        q = np.abs(t - bot.astype(np.float64)[:, None]) / float(scale)
        inside = (t >= lo[:, None]) & (t <= hi[:, None])
        w = np.where(inside, np.maximum(0.0, 1 - q), 0.0)
        w32 = np.maximum(_F32(0), _F32(1) - np.abs(np.arange(n_in, dtype=_F32)[None] - bot[:, None]) / _F32(scale)).astype(np.float64)
        return w, np.where(inside, np.abs(w32 - w), 0.0)

    wy, ey = axis(Hin, g["boty"], g["y0"], g["y1"], g["hs"])
    wx, ex = axis(Win, g["botx"], g["x0"], g["x1"], g["ws"])
    return g, wy, wx, ey, ex


def downsample_statement(x, Hout, Wout):
    """Downsample (downsample_layer.cu:15-72) per output element in fp64: weights from the fp32 positions, NaN samples vote with their
    weight and leave the sums.  Returns float64 arrays [N,C,Hout,Wout]: ref (NaN where the vote says so), A = sum |s| w / W,
    Ae = sum |s| e_w / W and Ee = sum e_w / W (e_w: see downsample_weights), W = the valid weight, Wn = the NaN weight, r = Wn / W
    (inf for an all-NaN window), voted = the NaN mask; and Wt = sum w [Hout,Wout].
    value = the quotient without the vote.  The vote is Wn / W > 0.5: strict, over the valid weight only."""
    x = np.ascontiguousarray(x, np.float32)
    N, C, Hin, Win = x.shape
    g, wy, wx, ey, ex = downsample_weights(Hin, Win, Hout, Wout)
    isn = np.isnan(x)
    s = np.where(isn, 0.0, x.astype(np.float64))

    def both(a, my, mx):                                              # sum_{y,x} my[o,y] a[..,y,x] mx[p,x]
        return np.einsum("oy,ncyp->ncop", my, np.einsum("ncyx,px->ncyp", a, mx, optimize=True), optimize=True)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        val = both(s, wy, wx)
        Wn = both(isn.astype(np.float64), wy, wx)
        Wt = wy.sum(1)[:, None] * wx.sum(1)[None]
        W = both((~isn).astype(np.float64), wy, wx)
        sa = np.abs(s)
        A = both(sa, wy, wx) / W
        Ae = (both(sa, ey, wx) + both(sa, wy, ex)) / W
        Ee = (ey.sum(1)[:, None] * wx.sum(1)[None] + wy.sum(1)[:, None] * ex.sum(1)[None])[None, None] / W
        r = Wn / W
        value = val / W
        nan = r > 0.5
        ref = np.where(nan, np.nan, value)
    return dict(ref=ref, value=value, A=A, Ae=Ae, Ee=Ee, W=W, Wn=Wn, r=r, Wt=Wt, voted=nan, geometry=g)


def channel_norm_statement(x, minus=None):
    """sqrt(sum_c v^2) in fp64, v = the fp32 difference x - minus for the folded-subtraction form."""
    v = np.asarray(x, np.float32)
    if minus is not None:
        v = v - np.asarray(minus, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((v.astype(np.float64) ** 2).sum(1, keepdims=True))


def channel_norm_backward_statement(x, top, top_diff):
    """(g * x) / (top + 1e-9) in fp64 with g * x rounded to fp32 first (channel_norm_layer.cu:45)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        gx = np.asarray(top_diff, np.float32) * np.asarray(x, np.float32)
        return gx.astype(np.float64) / (np.asarray(top, np.float32).astype(np.float64) + 1e-9)
