"""torch.autograd glue over the HIP operators (used by the FlowNet graphs in nets.py).

Forward and backward both run the hand-written HIP kernels through the C ABI; autograd only routes
tensors.  Gradient-stopping layers (Resample, Downsample: AllowBackward() == false in the
reference, resample_layer.hpp:25, downsample_layer.hpp:30) return no gradient.
"""
from __future__ import annotations

import collections
import os

import torch

from . import ops


_BATCH_INVARIANT = [False]


def set_batch_invariant(on: bool = True):
    """Make the bits of a sample independent of the batch it is computed in (scripts/run_flownet_many.py: one .flo per pair, whatever
    the batching and the sharding over GPUs -- run-flownet-many.py:27-81).  The own kernels are batch-invariant by construction except
    for the K split of the small-map kernels (fn2_set_batch_invariant fixes it to the one-sample value).  The library convolution that
    remains as the fallback for layer shapes outside FlowNet's families (`fallback_conv2d`: none of the five BASELINE configurations
    reaches it) chooses its kernels -- and with them the summation order -- by problem size, so in this mode it runs sample by sample."""
    _BATCH_INVARIANT[0] = bool(on)
    ops.set_batch_invariant(bool(on))


def batch_invariant() -> bool:
    return _BATCH_INVARIANT[0]


LIBRARY_FALLBACKS = [0]      # calls that left the own kernels (tests and the profile audits assert 0 on the BASELINE configurations)


def _note_fallback(what, x, w):
    LIBRARY_FALLBACKS[0] += 1
    if os.environ.get("FN2_STRICT") == "1":
        raise RuntimeError("flownet2_amd: no own kernel for %s bottom %s weight %s (FN2_STRICT=1)" % (what, tuple(x.shape), tuple(w.shape)))
    if os.environ.get("FN2_TRACE_FALLBACK") == "1":
        print("library fallback: %s bottom %s weight %s" % (what, tuple(x.shape), tuple(w.shape)), flush=True)


def _plain_call(stride, pad, dilation, groups):
    """The arguments lib_conv2d / lib_conv_transpose2d took before they learnt pairs, dilation and groups."""
    return not isinstance(stride, (tuple, list)) and not isinstance(pad, (tuple, list)) and dilation == 1 and groups == 1


def _lib_conv(x, w, b, stride, pad, dilation, groups, transposed, axes=4):
    """lib_conv2d and its kin on blobs of `axes` axes: the general kernels where _general_layer gives them the call, else the library."""
    layer = _general_layer(x, w, b, stride, pad, dilation, groups, transposed, axes)
    if layer is not None:
        return _GeneralConv.apply(x, w, b, layer[0], layer[1], transposed)
    name = "Deconvolution" if transposed else "Convolution"
    if axes == 4 and _plain_call(stride, pad, dilation, groups):
        kw = dict(stride=stride, padding=pad)
        what = "%s{stride %d, pad %d}" % (name, stride, pad)
    else:
        kw = dict(stride=stride, padding=pad, dilation=dilation, groups=groups)
        what = "%s{stride %s, pad %s, dilation %s, group %d}" % (name, stride, pad, dilation, groups)
    if x.is_cuda:
        _note_fallback(what, x, w)
    f = getattr(torch.nn.functional, ("conv_transpose%dd" if transposed else "conv%dd") % (axes - 2))
    if not _BATCH_INVARIANT[0] or not x.is_cuda:
        return f(x, w, b, **kw)
    return torch.cat([f(x[n:n + 1], w, b, **kw) for n in range(x.shape[0])], 0)


def lib_conv2d(x, w, b, stride, pad, dilation=1, groups=1):
    """Last resort for a Convolution no own kernel serves (a layer shape outside FlowNet's families, or CPU tensors): the library's
    convolution through torch, counted in LIBRARY_FALLBACKS for CUDA tensors; sample by sample in batch-invariant mode.  stride, pad and
    dilation: an int or a pair (h, w); w: [Cout, Cin / groups, kh, kw]."""
    return _lib_conv(x, w, b, stride, pad, dilation, groups, False)


def lib_conv_transpose2d(x, w, b, stride, pad, dilation=1, groups=1):
    """The same for a Deconvolution; w: [Cin, Cout / groups, kh, kw]."""
    return _lib_conv(x, w, b, stride, pad, dilation, groups, True)


def lib_conv3d(x, w, b, stride, pad, dilation=1, groups=1):
    """lib_conv2d for a volumetric Convolution: x [N, Cin, D, H, W], w [Cout, Cin / groups, kd, kh, kw]; stride, pad and dilation an int or
    a triple (d, h, w).  Under the same switch: "own" runs the depth tier of the general-geometry kernels, the default the library's
    conv3d through torch, counted in LIBRARY_FALLBACKS."""
    return _lib_conv(x, w, b, stride, pad, dilation, groups, False, axes=5)


def lib_conv_transpose3d(x, w, b, stride, pad, dilation=1, groups=1):
    """The same for a Deconvolution; w: [Cin, Cout / groups, kd, kh, kw]."""
    return _lib_conv(x, w, b, stride, pad, dilation, groups, True, axes=5)


# What lib_conv2d / lib_conv_transpose2d (and lib_conv3d / lib_conv_transpose3d) run CUDA float32 tensors on: "library" (the default: the library convolution through torch, counted
# and refused under FN2_STRICT=1 as above) or "own" (the general-geometry kernels, csrc/conv_general.hip: any taps, per-axis stride, pad and
# dilation, groups; exact fp32, forward and backward; nothing leaves the own kernels, so nothing is counted).  A switch of its own, not one of ARITH_SWITCHES.
_GENERAL_CONVOLUTIONS = ("library", "own")
_GENERAL_CONV = ["library"]


def set_general_convolution(name: str = "library"):
    """Where the last-resort convolutions run: "library" or "own".  Initial value: $FN2_CONV_GENERAL."""
    if name not in _GENERAL_CONVOLUTIONS:
        raise ValueError("general convolution must be one of %s, got %r" % (", ".join(_GENERAL_CONVOLUTIONS), name))
    _GENERAL_CONV[0] = name


def general_convolution() -> str:
    return _GENERAL_CONV[0]


if os.environ.get("FN2_CONV_GENERAL"):
    set_general_convolution(os.environ["FN2_CONV_GENERAL"])


def add_general_convolution_flag(ap):
    ap.add_argument("--general-conv", choices=list(_GENERAL_CONVOLUTIONS), default=None,
                    help="where convolutions outside FlowNet's kernel families run (default: $FN2_CONV_GENERAL, else library); own: the general-geometry kernels")


def apply_general_convolution_flag(args):
    if args.general_conv:
        set_general_convolution(args.general_conv)


def _general_layer(x, w, b, stride, pad, dilation, groups, transposed, axes):
    """(ABI, geometry) of the layer (ops.conv_general_abi and a descriptor for a _plain_call on 4 axes, which keeps to square taps; else
    ops.conv_geometry_abi and the 14 ints on 4 axes, ops.conv_volume_abi and the 19 ints on 5) where the switch is "own" and the general kernels
    take the call, else None."""
    if _GENERAL_CONV[0] != "own" or not (x.is_cuda and w.is_cuda and x.dtype == w.dtype == torch.float32 and x.dim() == w.dim() == axes):
        return None
    if groups < 1 or (b is not None and (not b.is_cuda or b.dtype != torch.float32)):
        return None
    Cout = w.shape[1] * groups if transposed else w.shape[0]
    if (x.shape[1] != w.shape[0]) if transposed else (x.shape[1] != w.shape[1] * groups):
        return None
    N, Cin, size, taps = x.shape[0], x.shape[1], tuple(x.shape[2:]), tuple(w.shape[2:])
    if axes == 5:
        abi, g = ops.conv_volume_abi, ops.conv_volume(N, Cin, size, Cout, taps, stride, pad, dilation, groups)
    elif not _plain_call(stride, pad, dilation, groups):
        abi, g = ops.conv_geometry_abi, ops.conv_geometry(N, Cin, size[0], size[1], Cout, taps, stride, pad, dilation, groups)
    elif taps[0] == taps[1]:
        abi, g = ops.conv_general_abi, ops.conv_desc(N, Cin, size[0], size[1], Cout, taps[0], stride, pad)
    else:
        return None
    return (abi, g) if abi.supported(g, transposed) else None


class _GeneralConv(torch.autograd.Function):
    """Convolution / Deconvolution of any geometry on the general kernels, through the ABI _general_layer chose; the operands are packed
    once per weight version, keyed by the ABI and by what of the geometry they depend on."""

    @staticmethod
    def forward(ctx, x, w, b, abi, g, transposed):
        ctx.layer, ctx.has_bias = (abi, g, transposed), b is not None
        ctx.save_for_backward(x, w)
        packed = _cached_pack(_PACKED_T, w, (abi.tag + "-fwd", transposed) + abi.key(g),
                              lambda: abi.pack_weights(w.detach().contiguous(), g, transposed))
        xb, x0 = _channel_slice(x)
        return abi.forward(xb, packed, b.detach() if b is not None else None, g, transposed, in_c0=x0)

    @staticmethod
    def backward(ctx, d):
        x, w = ctx.saved_tensors
        abi, g, transposed = ctx.layer
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        d = d.contiguous()
        gx = gw = gb = None
        if need_x:
            packed = _cached_pack(_PACKED_T, w, (abi.tag + "-dgrad", transposed) + abi.key(g),
                                  lambda: abi.pack_weights(w.detach().contiguous(), g, transposed, backward=True))
            gx = abi.backward_data(d, packed, g, transposed)
        if need_w or need_b:
            xb, x0 = _channel_slice(x)
            gw, gb = abi.backward_weights(xb, d, g, transposed, bias=bool(need_b), bottom_c0=x0)
        return gx, (gw if need_w else None), gb, None, None, None


def scale_shift(x, scale, shift=None, out=None, out_c0=0):
    """Deploy head in one pass (no autograd): out[:, out_c0:out_c0+C] = x * scale + shift[c], product and sum rounded separately."""
    with torch.no_grad():
        return ops.scale_shift_forward(x.detach().contiguous(), scale, shift, out=out, out_c0=out_c0)


class _Correlation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b0, b1, params):
        ctx.params = params
        ctx.save_for_backward(b0, b1)
        return ops.correlation_forward(params, b0, b1, bf16x3=_bf16x3("corr"))

    @staticmethod
    def backward(ctx, g):
        b0, b1 = ctx.saved_tensors
        d0, d1 = ops.correlation_backward(ctx.params, b0, b1, g.contiguous(),
                                          need0=ctx.needs_input_grad[0], need1=ctx.needs_input_grad[1])
        return d0, d1, None


def correlation(b0, b1, pad=0, kernel_size=1, max_displacement=0, stride_1=1, stride_2=1, correlation_type=ops.MULTIPLY):
    p = ops.corr_params(pad, kernel_size, max_displacement, stride_1, stride_2, correlation_type)
    return _Correlation.apply(b0.contiguous(), b1.contiguous(), p)


class _CorrelationReluInto(torch.autograd.Function):
    """Correlation + ReLU written into a channel slice of the consumer's Concat blob, with autograd: the backward pass undoes the ReLU from the
    activated planes where they lie (csrc/bias_act.hip reads both slices in place) and runs the correlation's own backward kernels."""

    @staticmethod
    def forward(ctx, b0, b1, params, blob, c0, slope):
        ops.correlation_forward(params, b0, b1, out=blob, out_c0=c0, relu=True, negative_slope=slope, bf16x3=_bf16x3("corr"))
        tc = ops.correlation_out_shape(params, b0.shape[1], b0.shape[2], b0.shape[3])[0]
        ctx.cfg = (params, c0, tc, slope)
        ctx.save_for_backward(b0, b1, blob)
        return blob[:, c0:c0 + tc]

    @staticmethod
    def backward(ctx, g):
        b0, b1, blob = ctx.saved_tensors
        params, c0, tc, slope = ctx.cfg
        gb, g0 = _channel_slice(g)
        d, _ = ops.bias_leaky_relu_backward((blob, c0, tc), (gb, g0, tc), slope, False)
        d0, d1 = ops.correlation_backward(params, b0, b1, d, need0=ctx.needs_input_grad[0], need1=ctx.needs_input_grad[1])
        return d0, d1, None, None, None, None


def correlation_relu_into(b0, b1, out, out_c0, negative_slope, pad=0, kernel_size=1, max_displacement=0, stride_1=1, stride_2=1, training=False):
    """Correlation + ReLU{negative_slope} written into the channel slice [out_c0, out_c0 + topC) of `out`: the cost volume lands
    in the [conv_redir | corr] blob conv3_1 reads, without the separate activation and concat passes.  With autograd: only when the caller
    asks for the graph-carrying form (training=True: the returned slice view carries the graph, nets._ConcatInPlace ties it to the blob);
    otherwise None (the caller builds the unfused graph)."""
    p = ops.corr_params(pad, kernel_size, max_displacement, stride_1, stride_2, ops.MULTIPLY)
    if torch.is_grad_enabled() and (b0.requires_grad or b1.requires_grad):
        if not training:
            return None
        return _CorrelationReluInto.apply(b0.contiguous(), b1.contiguous(), p, out, out_c0, negative_slope)
    return ops.correlation_forward(p, b0.contiguous(), b1.contiguous(), out=out, out_c0=out_c0, relu=True, negative_slope=negative_slope,
                                   bf16x3=_bf16x3("corr"))


class _FlowWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, flow, fill_value):
        ctx.save_for_backward(image, flow)
        return ops.flow_warp_forward(image, flow, fill_value)

    @staticmethod
    def backward(ctx, g):
        image, flow = ctx.saved_tensors
        di, df = ops.flow_warp_backward(image, flow, g.contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (di if ctx.needs_input_grad[0] else None), (df if ctx.needs_input_grad[1] else None), None


def flow_warp(image, flow, fill_value=ops.FILL_ZERO):
    return _FlowWarp.apply(image.contiguous(), flow.contiguous(), fill_value)


def resample(x, height, width, type=ops.LINEAR, antialias=True):
    with torch.no_grad():
        return ops.resample_forward(x.detach().contiguous(), height, width, type, antialias)


def resample_slices(x, height, width, type=ops.LINEAR, antialias=True, in_scale=1.0, out=None, out2=None, out2_scale=1.0):
    """Resample(x * in_scale) written into a channel slice (blob, c0, C); out2 = top * out2_scale into a second slice (no autograd)."""
    with torch.no_grad():
        return ops.resample_forward_slices(x.detach().contiguous(), height, width, type, antialias, in_scale, out, out2, out2_scale)


def flow_warp_slices(image, flow, out=None, fill_value=ops.FILL_ZERO):
    """FlowWarp over channel slices (blob, c0, C) of wider blobs (no autograd: deploy graphs)."""
    with torch.no_grad():
        return ops.flow_warp_forward_slices(image, flow, out, fill_value)


def channel_norm_slices(x, minus=None, out=None):
    """ChannelNorm(x - minus) over channel slices, top into one channel of a wider blob (no autograd: deploy graphs)."""
    with torch.no_grad():
        return ops.channel_norm_forward_slices(x, minus, out)


def downsample(x, top_height, top_width):
    with torch.no_grad():
        return ops.downsample_forward(x.detach().contiguous(), top_height, top_width)


def downsample_ahead(x, sizes):
    """Downsample(x) to every (height, width) of `sizes` on the second HIP stream (the one the weight gradients use), for consumers that
    need the result much later: the ground-truth pyramid of a training step depends on the ground truth alone, so it is issued at the START
    of the step and runs beside the first convolutions instead of between the forward and the backward pass (5 launches, 135 us of a
    FlowNetC step on the critical path).  Returns (tensors, event): the consumer's stream must wait for the event (wait_ahead)."""
    with torch.no_grad():
        x = x.detach().contiguous()
        many = (lambda: ops.downsample_forward_multi(x, sizes)) if ops.downsample_multi_supported(x.shape, sizes) and x.shape[0] > 0 else \
            (lambda: [ops.downsample_forward(x, h, w) for h, w in sizes])        # (one launch for the whole pyramid where its sizes allow)
        if not x.is_cuda:
            return [ops.downsample_forward(x, h, w) for h, w in sizes], None
        main = torch.cuda.current_stream(x.device)
        side = _WGRAD_SIDE["streams"].get(x.device)
        if side is None:
            side = _WGRAD_SIDE["streams"][x.device] = torch.cuda.Stream(device=x.device)
        side.wait_stream(main)                    # x was produced under the main stream
        with torch.cuda.stream(side):
            outs = many()
            ev = torch.cuda.Event()
            ev.record(side)
        x.record_stream(side)
        for t in outs:
            t.record_stream(main)
        return outs, ev


def wait_ahead(event):
    if event is not None:
        torch.cuda.current_stream().wait_event(event)


class _ChannelNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        top = ops.channel_norm_forward(x)
        ctx.save_for_backward(x, top)
        return top

    @staticmethod
    def backward(ctx, g):
        x, top = ctx.saved_tensors
        return ops.channel_norm_backward(x, top, g.contiguous())


def channel_norm(x):
    return _ChannelNorm.apply(x.contiguous())


class _L1Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b0, b1, params):
        loss, ws = ops.l1loss_forward(params, b0, b1)
        ctx.params, ctx.ws = params, ws
        ctx.save_for_backward(b0, b1)
        return loss

    @staticmethod
    def backward(ctx, g):
        b0, b1 = ctx.saved_tensors
        # the C ABI takes the loss weight as a host float, like top[0]->cpu_diff()[0] (l1loss_layer.cu:155)
        d0, d1 = ops.l1loss_backward(ctx.params, b0, b1, float(g), ctx.ws)
        return (d0 if ctx.needs_input_grad[0] else None), (d1 if (b1 is not None and ctx.needs_input_grad[1]) else None), None


def l1_loss(b0, b1=None, l2_per_location=False, l2_prescale_by_channels=False, normalize_by_num_entries=False,
            epsilon=1e-2, plateau=0.0):
    p = ops.l1_params(l2_per_location, l2_prescale_by_channels, normalize_by_num_entries, epsilon, plateau)
    return _L1Loss.apply(b0.contiguous(), b1.contiguous() if b1 is not None else None, p)


class _L1LossMulti(torch.autograd.Function):
    """All loss layers of a net: forward and backward one launch each, the weighted sum included; the upstream gradient stays on the
    device (no host read of a device scalar: _L1Loss's float(g) drains the stream once per layer)."""

    @staticmethod
    def forward(ctx, params, weights, n, *blobs):
        b0, b1 = list(blobs[:n]), list(blobs[n:])
        total, losses, ws = ops.l1loss_forward_multi(params, b0, b1, weights)
        ctx.params, ctx.weights, ctx.n, ctx.ws = params, weights, n, ws
        ctx.save_for_backward(*blobs)
        ctx.mark_non_differentiable(losses)
        return total, losses

    @staticmethod
    def backward(ctx, g, _g_losses):
        n = ctx.n
        blobs = ctx.saved_tensors
        b0, b1 = list(blobs[:n]), list(blobs[n:])
        need1 = any(ctx.needs_input_grad[3 + n:])
        d0, d1 = ops.l1loss_backward_multi(ctx.params, b0, b1, ctx.weights, g.contiguous(), ctx.ws, need1=need1)
        grads = [d if ctx.needs_input_grad[3 + k] else None for k, d in enumerate(d0)]
        grads += [d if ctx.needs_input_grad[3 + n + k] else None for k, d in enumerate(d1)]
        return (None, None, None) + tuple(grads)


def l1_loss_multi(preds, targets, weights, l2_per_location=False, l2_prescale_by_channels=False, normalize_by_num_entries=False,
                  epsilon=1e-2, plateau=0.0):
    """sum_k weights[k] * L1Loss(preds[k], targets[k]) -- the loss layers of a training net -- as (total, per-scale losses)."""
    p = ops.l1_params(l2_per_location, l2_prescale_by_channels, normalize_by_num_entries, epsilon, plateau)
    blobs = [t.contiguous() for t in preds] + [t.contiguous() for t in targets]
    return _L1LossMulti.apply(p, tuple(float(w) for w in weights), len(preds), *blobs)


class _LpqLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b0, b1, params):
        loss, ws = ops.lpq_loss_forward(params, b0, b1)
        ctx.params, ctx.ws = params, ws
        ctx.save_for_backward(b0, b1)
        return loss

    @staticmethod
    def backward(ctx, g):
        b0, b1 = ctx.saved_tensors
        # the C ABI takes the loss weight as a host float, like top[0]->cpu_diff()[0] (lpq_loss_layer.cu:215)
        d0, d1 = ops.lpq_loss_backward(ctx.params, b0, b1, float(g), ctx.ws)
        return (d0 if ctx.needs_input_grad[0] else None), (d1 if (b1 is not None and ctx.needs_input_grad[1]) else None), None


def lpq_loss(b0, b1=None, p=1.0, q=1.0, p_epsilon=0.0, q_epsilon=1e-2, l2_prescale_by_channels=False, normalize_by_num_entries=False):
    """LpqLoss: sum over (n, y, x) of (sum_c w (|b0 - b1| + p_epsilon)^p + q_epsilon)^q / normalize_coeff (csrc/lpq_loss.hip);
    p = 2, q = 0.5 is the l2_per_location form of l1_loss.  The defaults are caffe.proto:563-602's."""
    params = ops.lpq_params(p, q, p_epsilon, q_epsilon, l2_prescale_by_channels, normalize_by_num_entries)
    return _LpqLoss.apply(b0.contiguous(), b1.contiguous() if b1 is not None else None, params)


class _LpqLossMulti(torch.autograd.Function):
    """All LpqLoss layers of a net: forward and backward one launch each, the weighted sum included; the upstream gradient stays on
    the device (as _L1LossMulti)."""

    @staticmethod
    def forward(ctx, params, weights, n, *blobs):
        b0, b1 = list(blobs[:n]), list(blobs[n:])
        total, losses, ws = ops.lpq_loss_forward_multi(params, b0, b1, weights)
        ctx.params, ctx.weights, ctx.n, ctx.ws = params, weights, n, ws
        ctx.save_for_backward(*blobs)
        ctx.mark_non_differentiable(losses)
        return total, losses

    @staticmethod
    def backward(ctx, g, _g_losses):
        n = ctx.n
        blobs = ctx.saved_tensors
        b0, b1 = list(blobs[:n]), list(blobs[n:])
        need1 = any(ctx.needs_input_grad[3 + n:])
        d0, d1 = ops.lpq_loss_backward_multi(ctx.params, b0, b1, ctx.weights, g.contiguous(), ctx.ws, need1=need1)
        grads = [d if ctx.needs_input_grad[3 + k] else None for k, d in enumerate(d0)]
        grads += [d if ctx.needs_input_grad[3 + n + k] else None for k, d in enumerate(d1)]
        return (None, None, None) + tuple(grads)


def lpq_loss_multi(preds, targets, weights, p=1.0, q=1.0, p_epsilon=0.0, q_epsilon=1e-2, l2_prescale_by_channels=False,
                   normalize_by_num_entries=False):
    """sum_k weights[k] * LpqLoss(preds[k], targets[k]) -- the loss layers of a training net -- as (total, per-scale losses)."""
    params = ops.lpq_params(p, q, p_epsilon, q_epsilon, l2_prescale_by_channels, normalize_by_num_entries)
    blobs = [t.contiguous() for t in preds] + [t.contiguous() for t in targets]
    return _LpqLossMulti.apply(params, tuple(float(w) for w in weights), len(preds), *blobs)


def flow_metrics(pred, gt, valid=None, occ=None, *, outlier=(3.0, 0.05), bands=(10.0, 40.0), epe_map=False):
    """Error metrics of a predicted flow against ground truth, both [N,2,H,W] (csrc/flow_metrics.hip; the arithmetic is stated in
    include/flownet2_hip_flow_metrics.h): per sample the counted pixels, the EPE sum / sum of squares / max, the outliers (EPE > outlier[0]
    and > outlier[1] |gt|), the angular error, the EPE per band of |gt| (edges `bands`) and inside the `occ` mask.  valid / occ: [N,1,H,W],
    non-zero = use the pixel / occluded.  Returns an evaluate.FlowMetrics of N rows (its summary() gives the quoted numbers), with the
    [N,1,H,W] EPE map (NaN where a pixel is not counted) as .epe_map where epe_map is set.  Not differentiable: a metric, not a loss."""
    from .evaluate import FlowMetrics
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (pred, gt, valid, occ)):
        raise RuntimeError("flow_metrics is not differentiable: detach the inputs or call it under torch.no_grad() (the training loss is "
                           "l1_loss / lpq_loss)")
    results, emap = ops.flow_metrics(pred, gt, valid, occ, outlier=outlier, bands=bands, epe_map=epe_map)
    return FlowMetrics(results[:-1].cpu().numpy(), epe_map=emap)


def flow_consistency(fw, bw, *, alpha=(0.01, 0.5), beta=(0.01, 0.002), flags=False, err=False, warped=False):
    """Forward-backward consistency of two flows [N,2,H,W], fw from frame 0 to frame 1 and bw back (csrc/flow_consistency.hip; the
    arithmetic is stated in include/flownet2_hip_flow_consistency.h): a pixel is occluded where its target lies outside the image, where
    the other flow sampled at its target does not cancel its own (|a + b|^2 > alpha[0] (|a|^2 + |b|^2) + alpha[1]) or where a value is not
    finite; it lies on a motion boundary where |grad u|^2 + |grad v|^2 > beta[0] |a|^2 + beta[1].  Both directions in one launch.  Returns
    an evaluate.FlowConsistency: .occ_fw / .occ_bw [N,1,H,W] float planes of 0 / 1 (what flow_metrics takes as `occ`), the rows per
    direction (summary() gives the fractions), and where asked for the uint8 flag maps, the err maps |a + b| (NaN where there is none) and
    the other flow warped to the pixel.  Not differentiable: a check, not a loss."""
    from .evaluate import FlowConsistency
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (fw, bw)):
        raise RuntimeError("flow_consistency is not differentiable: detach the inputs or call it under torch.no_grad()")
    results, occ, fl, er, wa = ops.flow_consistency(fw, bw, alpha=alpha, beta=beta, flags=flags, err=err, warped=warped)
    rows = results[:, :-1].cpu().numpy()
    return FlowConsistency(rows[0], rows[1], occ=occ, flags=fl, err=er, warped=wa, alpha=alpha, beta=beta)


_SPLAT_MODES = {"sum": ("none", False), "average": ("none", True), "linear": ("linear", True), "softmax": ("softmax", True)}


class _FlowSplat(torch.autograd.Function):
    """Forward three launches, backward one gather launch; out and the denominator stay on the device for the backward."""

    @staticmethod
    def forward(ctx, values, flow, metric, src_valid, t, importance, normalize, fill_value, want_hole):
        _, out, den, hole, _ = ops.flow_splat_forward(values, flow, metric, src_valid, t=t, importance=importance, normalize=normalize,
                                                      fill_value=fill_value, hole=want_hole)
        ctx.cfg = (t, importance, normalize)
        ctx.save_for_backward(values, flow, metric, src_valid, out, den)
        ctx.mark_non_differentiable(*([hole] if want_hole else []))
        return (out, den, hole) if want_hole else (out, den)

    @staticmethod
    def backward(ctx, g, gw, *_):
        values, flow, metric, src_valid, out, den = ctx.saved_tensors
        t, importance, normalize = ctx.cfg
        need = ctx.needs_input_grad
        if g is None:
            g = torch.zeros_like(out)
        dv, df, dz = ops.flow_splat_backward(g.contiguous(), None if gw is None else gw.contiguous(), values, flow, metric, src_valid, out, den,
                                             t=t, importance=importance, normalize=normalize, need_values=need[0], need_flow=need[1],
                                             need_metric=need[2])
        return (dv, df, dz if need[2] else None) + (None,) * 6


def _flow_splat_mode(what, mode, normalize, fill, metric):
    if mode not in _SPLAT_MODES:
        raise ValueError(f'{what}: mode must be "sum", "average", "linear" or "softmax", got {mode!r}')
    importance, norm = _SPLAT_MODES[mode]
    if normalize is not None:
        norm = bool(normalize)
    if importance != "none" and metric is None:
        raise ValueError(f'{what}: mode "{mode}" needs a metric')
    if isinstance(fill, float) and fill != fill:
        fill_value = ops.FILL_NAN
    elif fill == 0:
        fill_value = ops.FILL_ZERO
    else:
        raise ValueError(f"{what}: fill must be 0.0 or nan, got {fill!r}")
    return importance, norm, fill_value


def flow_splat(values, flow, metric=None, *, t=1.0, mode="sum", normalize=None, fill=0.0, src_valid=None, weight=False, hole=False):
    """Forward warping (csrc/flow_splat.hip; the arithmetic is stated in include/flownet2_hip_flow_splat.h): every pixel of values [N,C,H,W]
    is carried along t * flow [N,2,H,W] and spread bilinearly over the four cells around its landing point -- the push that flow_warp's
    pull lacks.  mode (Niklaus and Liu, "Softmax Splatting", CVPR 2020): "sum" the plain sum; "average" the sum divided by the summed
    bilinear weights; "linear" / "softmax" the mean weighted by metric [N,1,H,W] / by exp(metric).  normalize=False with "linear" /
    "softmax" returns the raw numerator (the denominator is `weight`); normalize=True with "sum" is "average".  A cell that nothing reaches
    holds `fill` (0.0 or nan) where the result is normalised.  src_valid [N,1,H,W]: zero leaves the source out.  The sum at a cell runs in
    ascending source index whatever the batch and however many sources meet there: the same bits from run to run.  Returns out, or
    (out, weight, hole) with those asked for: weight [N,1,H,W] the denominator (with "sum" / "average" the range map), hole 1.0 where it is
    0.  Gradients for values, flow and metric (through out and weight); none for t."""
    importance, norm, fill_value = _flow_splat_mode("flow_splat", mode, normalize, fill, metric)
    if isinstance(src_valid, torch.Tensor) and src_valid.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("flow_splat: src_valid gets no gradient (values, flow and metric do): detach it")
    if importance == "none":
        metric = None
    res = _FlowSplat.apply(values.contiguous(), flow.contiguous(), None if metric is None else metric.contiguous(),
                           None if src_valid is None else src_valid.contiguous(), float(t), importance, norm, fill_value, bool(hole))
    picked = (res[0],) + ((res[1],) if weight else ()) + ((res[2],) if hole else ())
    return picked[0] if len(picked) == 1 else picked


def flow_splat_report(values, flow, metric=None, *, t=1.0, mode="sum", normalize=None, fill=0.0, src_valid=None):
    """flow_splat's forward without autograd, as an evaluate.FlowSplat: the rows per sample (masked, non-finite, outside and splatted
    sources, holes, the sum and the maximum of the weight plane) with out / weight / hole / status attached; summary() gives the shares."""
    from .evaluate import FlowSplat
    importance, norm, fill_value = _flow_splat_mode("flow_splat_report", mode, normalize, fill, metric)
    with torch.no_grad():
        results, out, den, hole, status = ops.flow_splat_forward(values, flow, None if importance == "none" else metric, src_valid, t=t,
                                                                 importance=importance, normalize=norm, fill_value=fill_value, hole=True,
                                                                 status=True)
    return FlowSplat(results[:-1].cpu().numpy(), out=out, weight=den, hole=hole, status=status, t=t, mode=mode)


def flow_range_occlusion(fw, bw, *, threshold=0.5):
    """The range-map occlusion of Wang et al., "Occlusion Aware Unsupervised Learning of Optical Flow" (CVPR 2018), of two flows
    [N,2,H,W], fw from frame 0 to frame 1 and bw back: the range map of a flow is a plane of ones splatted along it (flow_splat, "sum",
    t = 1), and a pixel of frame 0 is occluded where the range map of bw is below `threshold` -- nothing of frame 1 maps to it.  Returns
    (occ_fw, occ_bw, range_fw, range_bw), each [N,1,H,W]: occ_fw = 1.0 where range_fw (the range map of bw, on frame 0's grid) <
    threshold, occ_bw likewise from fw.  threshold is the caller's choice (0.5 here; the paper clips the map to [0, 1] instead).  The
    occ planes go where flow_consistency's do: flow_metrics(occ=), unsupervised_loss, census_loss.  Not differentiable."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (fw, bw)):
        raise RuntimeError("flow_range_occlusion is not differentiable: detach the inputs or call it under torch.no_grad()")
    if not (isinstance(fw, torch.Tensor) and isinstance(bw, torch.Tensor)) or fw.shape != bw.shape or fw.dim() != 4 or fw.shape[1] != 2:
        raise ValueError("flow_range_occlusion: fw and bw must both be [N,2,H,W]")
    threshold = float(threshold)
    if not threshold >= 0.0:
        raise ValueError(f"flow_range_occlusion: threshold = {threshold} (need >= 0)")
    with torch.no_grad():
        ones = torch.ones((fw.shape[0], 1, fw.shape[2], fw.shape[3]), dtype=torch.float32, device=fw.device)
        range_fw = ops.flow_splat_forward(ones, bw, out=False)[2]
        range_bw = ops.flow_splat_forward(ones, fw, out=False)[2]
    return (range_fw < threshold).float(), (range_bw < threshold).float(), range_fw, range_bw


def flow_interpolate(img0, img1, fw, bw, t, *, alpha=20.0, intensity_scale=255.0):
    """The frame at time t in (0, 1) between img0 and img1 [N,C,H,W] from the flows fw (frame 0 to 1) and bw (back), by softmax
    splatting: a composition over flow_warp and flow_splat, no network and no refinement.  z0 = -alpha mean_c |img0 - flow_warp(img1, fw)|
    / intensity_scale is the importance of a pixel of frame 0 (a pixel whose brightness the flow does not explain gives way where several
    land on one cell), z1 likewise for img1 and bw; (N0, D0) is the raw softmax splat of img0 along fw at t, (N1, D1) that of img1 along bw
    at 1 - t; the frame is ((1-t) N0 + t N1) / ((1-t) D0 + t D1) where that denominator is positive and (1-t) img0 + t img1 elsewhere.
    alpha is the user's knob and its default is arbitrary: 0 weighs every pixel alike, larger values let the better explained pixel win.
    Images in [0, 255] go with the default intensity_scale.  Not differentiable as it stands (call flow_splat for gradients)."""
    t = float(t)
    if not 0.0 <= t <= 1.0:
        raise ValueError(f"flow_interpolate: t = {t} (need 0 <= t <= 1)")
    with torch.no_grad():
        z0 = -float(alpha) * (img0 - flow_warp(img1, fw)).abs().mean(dim=1, keepdim=True) / float(intensity_scale)
        z1 = -float(alpha) * (img1 - flow_warp(img0, bw)).abs().mean(dim=1, keepdim=True) / float(intensity_scale)
        _, n0, d0, _, _ = ops.flow_splat_forward(img0, fw, z0, t=t, importance="softmax")
        _, n1, d1, _, _ = ops.flow_splat_forward(img1, bw, z1, t=1.0 - t, importance="softmax")
        den = (1.0 - t) * d0 + t * d1
        num = (1.0 - t) * n0 + t * n1
        blend = (1.0 - t) * img0 + t * img1
        return torch.where(den > 0, num / den, blend)


class _UnsupLoss(torch.autograd.Function):
    """Forward two launches, backward one; the normalisers and the upstream gradient stay on the device (as _LpqLossMulti)."""

    @staticmethod
    def forward(ctx, img0, img1, fw, bw, occ_fw, occ_bw, params):
        results, loss = ops.unsup_loss_forward(img0, img1, fw, bw, occ_fw, occ_bw, params)
        ctx.params, ctx.results = params, results
        ctx.save_for_backward(img0, img1, fw, bw, occ_fw, occ_bw)
        return loss

    @staticmethod
    def backward(ctx, g):
        img0, img1, fw, bw, occ_fw, occ_bw = ctx.saved_tensors
        need_bw = bw is not None and ctx.needs_input_grad[3]
        fd, bd = ops.unsup_loss_backward(img0, img1, fw, bw, occ_fw, occ_bw, ctx.params, ctx.results, g.contiguous(), need_bw=need_bw)
        return None, None, (fd if ctx.needs_input_grad[2] else None), (bd if need_bw else None), None, None, None


def _unsup_loss_args(what, img0, img1, fw, bw, occ_fw, occ_bw, kw):
    for name, t in (("img0", img0), ("img1", img1), ("occ_fw", occ_fw), ("occ_bw", occ_bw)):
        if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{what}: {name} gets no gradient (the flows alone do): detach it")
    blobs = tuple(t.contiguous() if t is not None else None for t in (img0, img1, fw, bw, occ_fw, occ_bw))
    return blobs, ops.unsup_loss_params(**kw)


class _CensusLoss(torch.autograd.Function):
    """Forward three launches, backward one; the planes G, Wg, pd, the normalisers and the upstream gradient stay on the device."""

    @staticmethod
    def forward(ctx, img0, img1, fw, bw, occ_fw, occ_bw, params):
        results, loss, saved = ops.census_loss_forward(img0, img1, fw, bw, occ_fw, occ_bw, params)
        ctx.params, ctx.results, ctx.planes = params, results, saved
        ctx.save_for_backward(img0, img1, fw, bw)
        return loss

    @staticmethod
    def backward(ctx, g):
        img0, img1, fw, bw = ctx.saved_tensors
        need_bw = bw is not None and ctx.needs_input_grad[3]
        fd, bd = ops.census_loss_backward(img0, img1, fw, bw, ctx.params, ctx.results, ctx.planes, g.contiguous(), need_bw=need_bw)
        return None, None, (fd if ctx.needs_input_grad[2] else None), (bd if need_bw else None), None, None, None


def _census_loss_args(what, img0, img1, fw, bw, occ_fw, occ_bw, kw):
    for name, t in (("img0", img0), ("img1", img1), ("occ_fw", occ_fw), ("occ_bw", occ_bw)):
        if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{what}: {name} gets no gradient (the flows alone do): detach it")
    blobs = tuple(t.contiguous() if t is not None else None for t in (img0, img1, fw, bw, occ_fw, occ_bw))
    return blobs, ops.census_loss_params(**kw)


def census_loss(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, *, data_weight=1.0, charbonnier=(1e-3, 0.45), radius=3,
                census_eps=(0.81, 0.1), intensity_scale=255.0, flow_mult=1.0):
    """The census data term of UnFlow (csrc/census_loss.hip; the arithmetic is stated in include/flownet2_hip_census_loss.h) of a forward
    flow fw [N,2,H,W] (frame 0 to frame 1) and, where given, a backward flow bw on the images img0, img1 [N,C,H,W], C up to 4: per
    direction data_weight times the mean over the counted pixels of psi(dist), dist the soft Hamming distance between the ternary census
    signatures, over a (2 radius + 1)^2 patch, of the own image and of the other image warped by the flow (grey values: the channel mean
    times intensity_scale; census_eps = (c_t, c_h)), psi(t) = (t^2 + eps^2)^gamma with (eps, gamma) = charbonnier.  An additive change of
    brightness between the frames leaves it unchanged.  occ_fw / occ_bw [N,1,H,W]: non-zero leaves the pixel's own term out
    (flow_consistency's .occ_fw / .occ_bw go in as they are).  The flows are multiplied by flow_mult first.  Returns the 0-axis device
    loss; gradients for fw and bw only."""
    blobs, params = _census_loss_args("census_loss", img0, img1, fw, bw, occ_fw, occ_bw, dict(
        data_weight=data_weight, charbonnier=charbonnier, radius=radius, census_eps=census_eps, intensity_scale=intensity_scale,
        flow_mult=flow_mult))
    return _CensusLoss.apply(*blobs, params)


def census_loss_report(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, *, data_weight=1.0, charbonnier=(1e-3, 0.45), radius=3,
                       census_eps=(0.81, 0.1), intensity_scale=255.0, flow_mult=1.0):
    """census_loss's forward without autograd, as an evaluate.CensusLoss: the rows per direction and sample (counted, occluded, outside and
    non-finite pixels, the data sum, the pairs and the sum of the distances) and the loss; summary() gives the means and shares."""
    from .evaluate import CensusLoss
    with torch.no_grad():
        blobs, params = _census_loss_args("census_loss_report", img0, img1, fw, bw, occ_fw, occ_bw, dict(
            data_weight=data_weight, charbonnier=charbonnier, radius=radius, census_eps=census_eps, intensity_scale=intensity_scale,
            flow_mult=flow_mult))
        results, loss, _ = ops.census_loss_forward(*blobs, params, save=False)
    rows = results[:, :-1].cpu().numpy()
    return CensusLoss(rows[0], rows[1], loss=float(loss), data_weight=data_weight, radius=radius)


def _data_term(what, data_term, census):
    if data_term not in ("brightness", "census"):
        raise ValueError('%s: data_term must be "brightness" or "census", got %r' % (what, data_term))
    if census is not None and data_term != "census":
        raise ValueError(f'{what}: census= is given but data_term is "brightness"')
    census = dict(census or {})
    unknown = set(census) - {"radius", "census_eps", "intensity_scale"}
    if unknown:
        raise ValueError(f"{what}: census= takes radius, census_eps and intensity_scale, not {sorted(unknown)}")
    return census


def unsupervised_loss(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, *, data_weight=1.0, smooth_weight=1.0, charbonnier=(1e-3, 0.45),
                      smooth_charbonnier=(1e-3, 0.45), edge_weight=10.0, smooth_order=2, flow_mult=1.0, data_term="brightness", census=None):
    """The unsupervised training loss (csrc/unsup_loss.hip; the arithmetic is stated in include/flownet2_hip_unsup_loss.h) of a forward
    flow fw [N,2,H,W] (frame 0 to frame 1) and, where given, a backward flow bw on the images img0, img1 [N,C,H,W], C up to 4: per
    direction data_weight times the mean over the counted pixels of sum_c psi(I_own - I_other warped by the flow) plus smooth_weight times
    the mean of the smoothness terms exp(-edge_weight mean_c |dI|) (psi(d u) + psi(d v)) of first or second order, psi(t) =
    (t^2 + eps^2)^gamma with (eps, gamma) = charbonnier for the data and smooth_charbonnier for the smoothness term.  occ_fw / occ_bw
    [N,1,H,W]: non-zero leaves the pixel out of the data term (flow_consistency's .occ_fw / .occ_bw go in as they are).  The flows are
    multiplied by flow_mult first.  Returns the 0-axis device loss; gradients for fw and bw only.

    data_term="census" replaces the brightness-constancy data term by census_loss (census=dict(radius=, census_eps=, intensity_scale=)
    where its defaults are not wanted; data_weight and charbonnier go to it): the sum of census_loss(...) and of this call with
    data_weight=0.0, which is the smoothness term.  The default leaves everything as it was."""
    census = _data_term("unsupervised_loss", data_term, census)
    if data_term == "census":
        data = census_loss(img0, img1, fw, bw, occ_fw, occ_bw, data_weight=data_weight, charbonnier=charbonnier, flow_mult=flow_mult, **census)
        return data + unsupervised_loss(img0, img1, fw, bw, occ_fw, occ_bw, data_weight=0.0, smooth_weight=smooth_weight, charbonnier=charbonnier,
                                        smooth_charbonnier=smooth_charbonnier, edge_weight=edge_weight, smooth_order=smooth_order,
                                        flow_mult=flow_mult)
    blobs, params = _unsup_loss_args("unsupervised_loss", img0, img1, fw, bw, occ_fw, occ_bw, dict(
        data_weight=data_weight, smooth_weight=smooth_weight, charbonnier=charbonnier, smooth_charbonnier=smooth_charbonnier,
        edge_weight=edge_weight, smooth_order=smooth_order, flow_mult=flow_mult))
    return _UnsupLoss.apply(*blobs, params)


def unsupervised_loss_report(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, *, data_weight=1.0, smooth_weight=1.0,
                             charbonnier=(1e-3, 0.45), smooth_charbonnier=(1e-3, 0.45), edge_weight=10.0, smooth_order=2, flow_mult=1.0,
                             data_term="brightness", census=None):
    """unsupervised_loss's forward without autograd, as an evaluate.UnsupLoss: the rows per direction and sample (counted, occluded,
    outside and non-finite pixels, the data and smoothness sums) and the loss; summary() gives the means and shares.  With
    data_term="census" the rows are those of the smoothness call (data_weight 0), .census holds census_loss_report's CensusLoss and .loss
    the sum of the two losses."""
    from .evaluate import UnsupLoss
    census = _data_term("unsupervised_loss_report", data_term, census)
    if data_term == "census":
        data = census_loss_report(img0, img1, fw, bw, occ_fw, occ_bw, data_weight=data_weight, charbonnier=charbonnier, flow_mult=flow_mult,
                                  **census)
        u = unsupervised_loss_report(img0, img1, fw, bw, occ_fw, occ_bw, data_weight=0.0, smooth_weight=smooth_weight, charbonnier=charbonnier,
                                     smooth_charbonnier=smooth_charbonnier, edge_weight=edge_weight, smooth_order=smooth_order,
                                     flow_mult=flow_mult)
        return UnsupLoss(u.rows_fw, u.rows_bw, loss=data.loss + u.loss, data_weight=0.0, smooth_weight=smooth_weight, census=data)
    with torch.no_grad():
        blobs, params = _unsup_loss_args("unsupervised_loss_report", img0, img1, fw, bw, occ_fw, occ_bw, dict(
            data_weight=data_weight, smooth_weight=smooth_weight, charbonnier=charbonnier, smooth_charbonnier=smooth_charbonnier,
            edge_weight=edge_weight, smooth_order=smooth_order, flow_mult=flow_mult))
        results, loss = ops.unsup_loss_forward(*blobs, params)
    rows = results[:, :-1].cpu().numpy()
    return UnsupLoss(rows[0], rows[1], loss=float(loss), data_weight=data_weight, smooth_weight=smooth_weight)


def _no_grad_inputs(what, tensors):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise RuntimeError(f"{what} is not differentiable: detach the inputs or call it under torch.no_grad()")


def flow_track_grid(N, H, W, cell=1, device=None):
    """The initial points of a tracker on a [H,W] plane cut into cells of `cell` pixels: float32 [N,2,P], P = ceil(H / cell) ceil(W / cell),
    x plane then y plane, one point at every cell's centre (cell = 1: the pixel grid) -- flow_track_reseed on an all-stopped state."""
    P = -(-int(H) // int(cell)) * -(-int(W) // int(cell))
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    points = torch.zeros((int(N), 2, P), dtype=torch.float32, device=device)
    state = torch.ones((int(N), P), dtype=torch.uint8, device=device)
    ops.flow_track_reseed(points, state, (H, W), cell, born=False)
    return points


def flow_track_reseed(points, state, size, cell):
    """Fill the gaps in a tracker's coverage, IN PLACE (fn2_flow_track_reseed, include/flownet2_hip_flow_track.h): points [N,2,P] and
    state uint8 [N,P] on a plane size = (H, W) cut into cells of `cell` pixels, slot c owning cell c.  Every stopped slot whose home cell
    holds no alive point starts anew at the cell's centre.  Returns born uint8 [N,P], 1 at exactly those slots."""
    _no_grad_inputs("flow_track_reseed", (points,))
    return ops.flow_track_reseed(points, state, size, cell, born=True)


def flow_track(fw, bw, points=None, state=None, stop=None, stop_mask=None, alpha=(0.01, 0.5), tracks=True):
    """Carry points through a sequence of flows (csrc/flow_track.hip; the arithmetic is stated in include/flownet2_hip_flow_track.h): fw, bw
    [N,T,2,H,W], fw[:,t] from frame t to t+1 and bw[:,t] back, or [N,2,H,W] for one step.  points [N,2,P] (x plane, y plane; [N,2,H,W] is
    taken as P = H W) or None for the dense pixel grid; state uint8 [N,P], non-zero = already stopped; stop uint8 [N,T,1,H,W] (or
    [N,1,H,W]): a point stops where stop & stop_mask is non-zero at its nearest pixel -- by default the BOUNDARY bit, so
    flow_consistency(..., flags=True).flags_fw goes in as it is.  A point also stops where its target leaves the image, where the backward
    flow at its target does not cancel the forward one (alpha, as in flow_consistency) and where a value is not finite.  One launch for all
    T frames.  Returns an evaluate.FlowTracks.  Not differentiable."""
    from .evaluate import CONSISTENCY_FLAGS, FlowTracks
    _no_grad_inputs("flow_track", (fw, bw, points))
    if isinstance(fw, torch.Tensor) and fw.dim() == 4:
        fw = fw.unsqueeze(1)
    if isinstance(bw, torch.Tensor) and bw.dim() == 4:
        bw = bw.unsqueeze(1)
    if isinstance(stop, torch.Tensor) and stop.dim() == 4:
        stop = stop.unsqueeze(1)
    if not isinstance(fw, torch.Tensor) or fw.dim() != 5:
        raise ValueError("flow_track: fw must be [N,T,2,H,W] or [N,2,H,W]")
    N, T, _, H, W = fw.shape
    if points is None:
        ops._chk(fw, "fw", 5)
        points = flow_track_grid(N, H, W, 1, device=fw.device)
    elif isinstance(points, torch.Tensor) and points.dim() == 4:
        points = points.reshape(points.shape[0], points.shape[1], -1)
    mask = CONSISTENCY_FLAGS["BOUNDARY"] if stop_mask is None else int(stop_mask)
    results, tr, p_out, s_out, st = ops.flow_track(fw, bw, points, state=state, stop=stop, stop_mask=mask, alpha=alpha, tracks=tracks)
    return FlowTracks(results[:-1].cpu().numpy(), tracks=tr, points=p_out, state=s_out, steps=st, start=points.contiguous(), size=(H, W), alpha=alpha)


def flow_to_color(flow, max_flow=None, norm="sample"):
    """The Middlebury colour coding of a flow [N,2,H,W] as uint8 [N,H,W,3] on the device (csrc/flow_visualize.hip; the arithmetic is stated
    in include/flownet2_hip_flow_visualize.h): hue from the direction, saturation from the radius over a normalising radius, unknown flow
    (a value above 1e9, NaN, Inf) black.  With max_flow the radius is divided by it, so pictures of different runs compare (a pixel beyond
    it is drawn at three quarters of its hue's brightness); without, by the largest radius of the sample (norm="sample": a sample's picture
    is the same alone and in any batch) or of the whole batch (norm="batch").  No host readback.  Not differentiable: a picture."""
    _no_grad_inputs("flow_to_color", (flow,))
    if norm not in ("sample", "batch"):
        raise ValueError(f"flow_to_color: norm must be 'sample' or 'batch', got {norm!r}")
    return ops.flow_color(flow, norm="fixed" if max_flow is not None else norm, max_flow=max_flow)[0]


def flow_error_map(pred, gt, valid=None, occ=None, abs_thresh=3.0, rel_thresh=0.05):
    """The KITTI-style error image of a predicted flow against ground truth, both [N,2,H,W], as uint8 [N,H,W,3] on the device
    (csrc/flow_visualize.hip): the colour of the bin of n = min(EPE / abs_thresh, EPE / |gt| / rel_thresh), blue below 1 and red above -- 1
    is the Fl outlier criterion of flow_metrics --, black where there is no ground truth (gt unknown, or valid [N,1,H,W] zero), dimmed to
    half where occ [N,1,H,W] is non-zero (flow_consistency(...).occ_fw goes in as it is).  Not differentiable: a picture."""
    _no_grad_inputs("flow_error_map", (pred, gt, valid, occ))
    return ops.flow_error_map(pred, gt, valid, occ, abs_thresh=abs_thresh, rel_thresh=rel_thresh)


def add_loss_flags(ap):
    """--loss l1 | lpq and the Lpq schedule of a training script (scripts/train_pipeline.py, scripts/train_prototxt_step.py)."""
    ap.add_argument("--loss", choices=("l1", "lpq"), default="l1", help="l1: L1Loss{l2_per_location} (the default); lpq: LpqLoss with --lpq-p / --lpq-q")
    ap.add_argument("--lpq-p", type=float, nargs="+", default=[2.0], metavar="P", help="p of every episode (one value: constant)")
    ap.add_argument("--lpq-q", type=float, nargs="+", default=[0.2], metavar="Q", help="q of every episode")
    ap.add_argument("--lpq-starts", type=int, nargs="+", default=[], metavar="ITER", help="iteration at which each episode starts (the first is 0)")
    ap.add_argument("--lpq-p-epsilon", type=float, default=0.0)
    ap.add_argument("--lpq-q-epsilon", type=float, default=1e-2)


def loss_schedule(args):
    """None for --loss l1, else the LpqSchedule of the flags (its checks are LpqLossLayer::LayerSetUp's)."""
    from .lpq_schedule import LpqSchedule
    return LpqSchedule(args.lpq_starts, args.lpq_p, args.lpq_q) if args.loss == "lpq" else None


class _PredictFlow(torch.autograd.Function):
    """predict_flow (Convolution{3,1,1} C -> 2): own forward (csrc/flow_head.hip) and own backward (csrc/flow_head_bwd.hip: weight,
    bias and bottom gradients as streaming kernels over NCHW -- a 2-channel side cannot feed a matrix tile)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return ops.predict_flow_conv_forward(x.contiguous(), weight.contiguous(), bias)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        blob, c0 = _channel_slice(x)
        g = g.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        side = _wgrad_side_stream(g, x, w) if (need_w or need_b) and need_x else None
        if side is None:
            return ops.predict_flow_conv_backward((blob, c0, x.shape[1]), w, g, need_x, need_w, need_b)
        # round 6: only the data gradient is on the critical path of the backward pass; the head's weight / bias gradient (a pass over the
        # whole Concat blob in front of it) runs beside the data-gradient chain like the convolutions' weight gradients
        dx, _, _ = ops.predict_flow_conv_backward((blob, c0, x.shape[1]), w, g, True, False, False)
        main = torch.cuda.current_stream(g.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            _, dw, db = ops.predict_flow_conv_backward((blob, c0, x.shape[1]), w, g, False, need_w, need_b)
        for t in (g, blob):
            t.record_stream(side)
        for t in (dw, db):
            if t is not None:
                t.record_stream(main)
        if dw is not None:
            _SIDE_PENDING.append((w, dw.data_ptr()))
        return dx, dw, db


class _UpsampleFlow(torch.autograd.Function):
    """upsample_flow (Deconvolution{4,2,1} 2 -> 2): own forward and own backward (csrc/flow_head_bwd.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, into=None):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        if into is None:
            return ops.upsample_flow_deconv_forward(x.contiguous(), weight.contiguous(), bias)
        ops.upsample_flow_deconv_forward(x.contiguous(), weight.contiguous(), bias, out=into[0], out_c0=into[1])
        return into[0][:, into[1]:into[1] + 2]          # (see _OwnForwardConv.forward)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dx, dw, db = ops.upsample_flow_deconv_backward(x.contiguous(), w, g.contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                                       ctx.has_bias and ctx.needs_input_grad[2])
        return dx, dw, db, None


def predict_flow_conv(x, weight, bias=None):
    """predict_flow (Convolution{3,1,1} -> 2 channels): own forward kernel; with autograd active own backward kernels too."""
    run = lambda xx, ww, bb: ops.predict_flow_conv_forward(xx.contiguous(), ww.contiguous(), bb)
    if _needs_grad(x, weight, bias):
        if ops.predict_flow_conv_backward_supported(x.shape[0], x.shape[1], x.shape[2], x.shape[3]):
            return _PredictFlow.apply(x, weight, bias)
        return _OwnForwardConv.apply(x, weight, bias, run, 1, 1, 0.0, False, False)
    return run(x, weight, bias)


def upsample_flow_deconv(x, weight, bias=None, out=None, out_c0=0):
    """upsample_flow (Deconvolution{4,2,1} 2 -> 2 channels); `out`: write into that channel slice of a Concat blob (no autograd)."""
    if out is not None and not _needs_grad(x, weight, bias):
        return ops.upsample_flow_deconv_forward(x.contiguous(), weight.contiguous(), bias, out=out, out_c0=out_c0)
    run = lambda xx, ww, bb: ops.upsample_flow_deconv_forward(xx.contiguous(), ww.contiguous(), bb)
    if _needs_grad(x, weight, bias):
        return _UpsampleFlow.apply(x, weight, bias, None if out is None else (out, out_c0))
    return run(x, weight, bias)


def predict_upsample_flow(x, weight, bias, up_weight, up_bias, out, out_c0):
    """predict_flow and the upsample_flow of it into out[:, out_c0:out_c0+2] with one launch less (no autograd): the flow, or None where
    a gradient is needed or the kernel declines -- the caller then runs predict_flow_conv and upsample_flow_deconv."""
    if _needs_grad(x, weight, bias) or _needs_grad(x, up_weight, up_bias):
        return None
    return ops.predict_upsample_flow_forward(x.contiguous(), weight.contiguous(), bias, up_weight.contiguous(), up_bias, out, out_c0)


class _BiasLeakyReLU(torch.autograd.Function):
    """y -> leaky_relu(y + bias) in place on the convolution output (conv2d's backward does not need its output), with the
    fused backward: one pass for the activation gradient and the bias gradient."""

    @staticmethod
    def forward(ctx, y, bias, negative_slope):
        ctx.mark_dirty(y)
        ops.bias_leaky_relu_(y, bias, negative_slope)
        ctx.slope = negative_slope
        ctx.has_bias = bias is not None
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        d, db = ops.bias_leaky_relu_backward(y, g.contiguous(), ctx.slope, ctx.has_bias and ctx.needs_input_grad[1])
        return d, db, None


def conv_bias_leaky_relu(y, bias, negative_slope=0.1):
    """Bias term + in-place leaky ReLU on a bias-free convolution output: one HIP pass forward, one backward."""
    if not y.is_contiguous():
        if bias is not None:
            y = y + bias.view(1, -1, 1, 1)
        return torch.nn.functional.leaky_relu(y, negative_slope)
    if torch.is_grad_enabled() and (y.requires_grad or (bias is not None and bias.requires_grad)):
        return _BiasLeakyReLU.apply(y, bias, negative_slope)
    return ops.bias_leaky_relu_(y, bias, negative_slope)


def invalidate_weight_caches():
    """Drop every packed weight copy.  The caches notice in-place writes through the tensor itself (`_version`), but not
    writes through `.data` or a checkpoint load into `.data`: call this after such a write (parallel.broadcast_params does)."""
    _bump_weight_generation()
    _PACKED_T.clear()


_WEIGHT_GENERATION = [0]     # bumped by every torch optimizer step (global post-step hook below) and by invalidate_weight_caches()


def weight_generation() -> int:
    return _WEIGHT_GENERATION[0]


def _bump_weight_generation(*_a, **_k):
    _WEIGHT_GENERATION[0] += 1


try:        # every torch.optim.Optimizer.step() of this process, fused ones included (they write the parameters WITHOUT bumping `_version`)
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_step_hook
    _reg_step_hook(_bump_weight_generation)
    _HAVE_STEP_HOOK = True
except Exception:       # pragma: no cover - torch without the global hook: trainable tensors are never cached (round-4 behaviour)
    _HAVE_STEP_HOOK = False


def _cached(cache, key, w, make):
    """make() for weight tensor w, remembered under `key` while w is alive and unwritten.  Writes are noticed through `_version` -- which
    fused optimizers do NOT touch (torch.optim.Adam(fused=True) leaves it at 0: scripts/probes/stale_pack_probe.py, round 4: the cached
    operands of step 1 served every later step).  For a tensor that requires grad the entry therefore also carries the weight GENERATION,
    a counter every torch optimizer step bumps through the global post-step hook above: a trainable parameter is repacked once per
    optimizer step (not once per use), and inference under no_grad with default nn.Parameter weights keeps its packs.  Writes through
    `.data` / a custom optimizer that is not a torch.optim.Optimizer need invalidate_weight_caches()."""
    import weakref
    if w.requires_grad and (not _HAVE_STEP_HOOK or (w.is_cuda and torch.cuda.is_current_stream_capturing())):
        # (under hipGraph capture a trainable weight is packed INSIDE the graph: a replayed optimizer step fires no hook, and a pack left
        # out of the capture would serve every replay the operands of capture time)
        cache.pop(key, None)
        return make()
    gen = _WEIGHT_GENERATION[0] if w.requires_grad else -1
    hit = cache.get(key)
    if hit is None or hit[0]() is not w or hit[1] != w._version or hit[3] != gen:
        hit = (weakref.ref(w, lambda _r, k=key: cache.pop(k, None)), w._version, make(), gen)
        cache[key] = hit
    return hit[2]


_ROUTE_FORCE = [False]


def set_route_force(on: bool = True):
    """Test hook (FN2_ROUTE_FORCE of fn2_conv_route): the Winograd kernel wherever it applies, the small-map kernel whatever the map size."""
    _ROUTE_FORCE[0] = bool(on)


# The opt-in split-bf16 ("bf16x3") arithmetics: one switch per kernel family, each of its own.  "fp32" (exact fp32 products) is the default
# of every one; "bf16x3" (six bf16 piece products per multiply, fp32 accumulation: include/flownet2_hip.h, FN2_CONV_ARITH_BF16X3) moves
# only the layers the family's route function hands to that kernel, every other layer and every other pass stays exact fp32.
#   key          the script flag is --<key>-arith
#   env          the environment variable that sets the initial value (read once, below; a bad value raises there)
#   setter, getter   the public functions of this module
#   what         the switch's name in the setter's ValueError
#   of           "arithmetic of the <of>" in a script's help;  report: "<report> arithmetic: ..." in a script's output
#   covers       what bf16x3 moves
ArithSwitch = collections.namedtuple("ArithSwitch", "key env setter getter what of report covers")
ARITH_SWITCHES = (
    ArithSwitch("conv", "FN2_CONV_ARITH", "set_conv_arithmetic", "conv_arithmetic", "conv", "convolution forward", "convolution forward",
                "split-bf16 on the direct 5x5 / 2 layers"),
    ArithSwitch("deconv", "FN2_DECONV_ARITH", "set_deconv_arithmetic", "deconv_arithmetic", "deconv", "deconvolution forward", "deconvolution forward",
                "split-bf16 in the GEMM of the 4x4 / 2 layers"),
    ArithSwitch("wino", "FN2_WINO_ARITH", "set_winograd_arithmetic", "winograd_arithmetic", "winograd", "Winograd 3x3 forward", "winograd forward",
                "split-bf16 on the 3x3 / 1 layers with Cout % 64 == 0"),
    ArithSwitch("corr", "FN2_CORR_ARITH", "set_correlation_arithmetic", "correlation_arithmetic", "correlation", "correlation forward", "correlation forward",
                "split-bf16 in the FlowNetC correlation (same fp64 bound as the exact kernel; measured times: profiles/corr_bf16x3_bench.md)"),
    ArithSwitch("dgrad", "FN2_DGRAD_ARITH", "set_conv_backward_arithmetic", "conv_backward_arithmetic", "conv backward", "convolution data gradient",
                "data-gradient", "split-bf16 on the 5x5 / 2 layers"),
    ArithSwitch("wgrad", "FN2_WGRAD_ARITH", "set_conv_weight_gradient_arithmetic", "conv_weight_gradient_arithmetic", "conv weight gradient",
                "convolution weight gradient", "weight-gradient", "split-bf16 on the 5x5 / 2 layers"),
)
_CONV_ARITHMETICS = ("fp32", "bf16x3")
_ARITH_SWITCH = {s.key: s for s in ARITH_SWITCHES}
_ARITH = {s.key: "fp32" for s in ARITH_SWITCHES}


def _set_arithmetic(key: str, name: str):
    if name not in _CONV_ARITHMETICS:
        raise ValueError("%s arithmetic must be one of %s, got %r" % (_ARITH_SWITCH[key].what, ", ".join(_CONV_ARITHMETICS), name))
    _ARITH[key] = name


def arithmetic(key: str) -> str:
    """The value of the switch `key` of ARITH_SWITCHES: "fp32" or "bf16x3"."""
    return _ARITH[key]


def _bf16x3(key: str) -> bool:
    return _ARITH[key] == "bf16x3"


for _s in ARITH_SWITCHES:
    if os.environ.get(_s.env):
        _set_arithmetic(_s.key, os.environ[_s.env])


def set_conv_arithmetic(name: str = "fp32"):
    """Arithmetic of the convolution FORWARD on the layers fn2_conv_route hands to the split kernel: the direct 5x5 / 2 layers
    (csrc/conv_bf16x3.hip).  Initial value: $FN2_CONV_ARITH."""
    _set_arithmetic("conv", name)


def conv_arithmetic() -> str:
    return arithmetic("conv")


def set_deconv_arithmetic(name: str = "fp32"):
    """Arithmetic of the Deconvolution{4, 2, 1} FORWARD: the weight^T x bottom GEMM of the layers fn2_deconv_route hands to the GEMM route
    (csrc/deconv_bf16x3.hip; the col2im + bias + ReLU pass is unchanged).  Initial value: $FN2_DECONV_ARITH."""
    _set_arithmetic("deconv", name)


def deconv_arithmetic() -> str:
    return arithmetic("deconv")


def set_winograd_arithmetic(name: str = "fp32"):
    """Arithmetic of the Winograd F(2x2, 3x3) FORWARD on the Winograd layers fn2_conv_route hands to the split kernel under
    FN2_ROUTE_WINO_BF16X3 (csrc/conv_wino_bf16x3.hip: 3x3 / 1 / 1, Win % 4 == 0, Cout % 64 == 0).  Initial value: $FN2_WINO_ARITH."""
    _set_arithmetic("wino", name)


def winograd_arithmetic() -> str:
    return arithmetic("wino")


get_winograd_arithmetic = winograd_arithmetic          # the name it was introduced under


def set_conv_backward_arithmetic(name: str):
    """Arithmetic of the convolution DATA GRADIENT on the layers fn2_conv_backward_data_route_flags hands to the split kernel
    (csrc/tconv_bf16x3.hip: the stride-2 5x5 / 2 / 2 class of the transposed-convolution route, conv2 / conv3 of the encoders, plain and
    with the ReLU derivative of the layer in front folded in); every weight and bias gradient stays as it is.  Initial value:
    $FN2_DGRAD_ARITH."""
    _set_arithmetic("dgrad", name)


def conv_backward_arithmetic() -> str:
    return arithmetic("dgrad")


def set_conv_weight_gradient_arithmetic(name: str):
    """Arithmetic of the convolution WEIGHT GRADIENT on the layers fn2_conv_backward_weights_arith hands to the split kernel
    (csrc/conv_wgrad_bf16x3.hip: the 5x5 / 2 / 2 class, conv2 / conv3 of the encoders); the stem's fused weight + bias gradient, every
    Deconvolution and every bias and data gradient stay as they are.  Initial value: $FN2_WGRAD_ARITH."""
    _set_arithmetic("wgrad", name)


def conv_weight_gradient_arithmetic() -> str:
    return arithmetic("wgrad")


def set_correlation_arithmetic(name: str = "fp32"):
    """Arithmetic of the Correlation FORWARD on the layers fn2_correlation_route hands to the split kernel (csrc/correlation_bf16x3.hip:
    the FlowNetC instance, C % 32 == 0, W % 4 == 0); the backward stays exact fp32.  Honoured by correlation / correlation_relu_into here
    and by layers.CorrelationLayer.  Initial value: $FN2_CORR_ARITH."""
    _set_arithmetic("corr", name)


def correlation_arithmetic() -> str:
    return arithmetic("corr")


def arithmetic_flags(keys=None):
    """The script flags of the switches `keys` (default: all): ["--conv-arith", ...]."""
    return ["--%s-arith" % s.key for s in ARITH_SWITCHES if keys is None or s.key in keys]


def add_arithmetic_flags(ap, keys, notes=None):
    """Adds --<key>-arith for every key of `keys` to the argparse parser `ap`, in that order; notes[key] is appended to that flag's help."""
    for key in keys:
        s = _ARITH_SWITCH[key]
        text = "arithmetic of the %s (default: $%s, else fp32); bf16x3: %s%s" % (s.of, s.env, s.covers, (notes or {}).get(key, ""))
        ap.add_argument("--%s-arith" % key, choices=list(_CONV_ARITHMETICS), default=None, help=text.replace("%", "%%"))


def apply_arithmetic_flags(args, keys):
    """Sets every switch of `keys` whose flag was given (add_arithmetic_flags) from the parsed arguments."""
    for key in keys:
        name = getattr(args, "%s_arith" % key)
        if name:
            _set_arithmetic(key, name)


def print_arithmetics(keys):
    for key in keys:
        print("%s arithmetic: %s" % (_ARITH_SWITCH[key].report, _ARITH[key]))


def _channel_slice(x):
    """(blob, first channel): x itself, or -- when x is a channel-slice view `blob[:, c0:c0+C]` of a contiguous NCHW blob (a skip
    tensor that was written straight into its Concat blob) -- that blob and the offset, so that the kernels read it in place."""
    if x.is_contiguous():
        return x, 0
    b = x._base
    if (b is not None and b.dim() == 4 and b.is_contiguous() and x.dim() == 4 and x.stride() == b.stride() and x.shape[0] == b.shape[0]
            and x.shape[2:] == b.shape[2:]):
        plane = b.shape[2] * b.shape[3]
        off = x.storage_offset() - b.storage_offset()
        if off % plane == 0 and 0 <= off // plane and off // plane + x.shape[1] <= b.shape[1]:
            return b, off // plane
    return x.contiguous(), 0


class _OwnForwardConv(torch.autograd.Function):
    """Training form of the fused forward kernels: `runner(x, weight, bias)` is one of the own kernels (convolution or
    deconvolution + bias [+ leaky ReLU] in one launch or one GEMM route); the backward undoes the activation and reduces the bias
    gradient in one fused pass (csrc/bias_act.hip, from the saved OUTPUT) and computes the two convolution gradients on the own backward
    routes (conv_backward: fn2_conv_backward_data / _weights; what they decline is the counted library's convolution_backward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, runner, stride, pad, negative_slope, act, transposed, into=None, relu_chain=None):
        # autograd does not record inside forward(): the parameter OBJECT goes to the runner, so that the packed-weight caches
        # (keyed on the parameter and its _version) hit until the optimizer writes the weight.
        # into = (blob, first channel): the runner writes its channels into that slice of the consumer's Concat blob (a plain buffer
        # outside the graph; nets._ConcatInPlace ties the slices together) and the output is the slice view
        if into is None:
            y = runner(x, weight, bias)
        else:
            runner(x, weight, bias, into[0], into[1])
            co = weight.shape[1] if transposed else weight.shape[0]
            y = into[0][:, into[1]:into[1] + co]
        ctx.cfg = (stride, pad, negative_slope, act, bias is not None, transposed)
        ctx.into = into
        # relu_chain (round 6, set by the graph builder for a layer pair A -> B where B is A's ONLY consumer): bit 0 on A = "my top_diff arrives
        # already multiplied by my ReLU derivative" (B did it), bit 1 on B = "fold the ReLU derivative of the layer in front into my data gradient"
        ctx.relu_chain, ctx.chain_cell = (int(relu_chain[0]), relu_chain[1]) if relu_chain else (0, None)
        # ... and both ends must be in the graph: a consumer whose producer took another path (no relu_chain handed to it) would fold a ReLU
        # derivative the producer's own backward applies a second time
        if ctx.relu_chain & 1:
            ctx.chain_cell["armed"] = True
        elif ctx.relu_chain & 2 and not ctx.chain_cell.get("armed"):
            raise RuntimeError("relu_chain: the layer in front of this one is not a chain producer (it would undo its ReLU twice)")
        # the activated output is needed for the ReLU mask: a slice of a Concat blob is kept as the BLOB (a saved view comes back from autograd
        # as a plain strided tensor that has forgotten its base: reading it in place needs the blob and the offset)
        ctx.save_for_backward(x, weight, (into[0] if into is not None else y) if act else None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, y = ctx.saved_tensors
        stride, pad, slope, act, has_bias, transposed = ctx.cfg
        if act and ctx.into is not None:
            y = (y, ctx.into[1], w.shape[1] if transposed else w.shape[0])          # (blob, first channel, channels)
        premasked = False
        if ctx.relu_chain & 1:
            # the consumer must have folded this layer's ReLU derivative into the gradient it handed over -- checked, not assumed: a consumer
            # that took another route (a library fallback, a frozen graph) would otherwise leave the gradient unmasked without a sound
            if not ctx.chain_cell.get("masked"):
                raise RuntimeError("relu_chain: the consumer of this layer did not fold the ReLU derivative into its data gradient")
            ctx.chain_cell["masked"] = False
            premasked = True
        gx, gw, db = conv_backward(x, w, y if act else None, g, stride, pad, slope, transposed, bool(ctx.needs_input_grad[0]),
                                   bool(ctx.needs_input_grad[1]), has_bias and ctx.needs_input_grad[2], premasked=premasked,
                                   mask_bottom=(ctx.chain_cell["slope"] if (ctx.relu_chain & 2) else None))
        if ctx.relu_chain & 2:
            ctx.chain_cell["masked"] = True
        return (gx, gw, db) + (None,) * (len(ctx.needs_input_grad) - 3)


_GRAD_SLOT = [None]          # parallel.GradientExchange with a collective: weight tensor -> its slot of the flat all-reduce bucket (or None)


def set_grad_slots(fn=None):
    """fn(weight) -> a fresh fp32 view shaped like `weight` into the flat bucket its gradient travels in (or None).  The weight-gradient
    kernels then write their result THERE (fn2_conv_backward_weights' `weight_diff` pointer) and autograd moves that view into `.grad`:
    the gradient is produced in the bucket instead of being copied into it by the hook (156.7 MB read + written per FlowNetC step)."""
    _GRAD_SLOT[0] = fn


def _grad_slot(w):
    fn = _GRAD_SLOT[0]
    if fn is None or w.grad is not None:          # a pass that ACCUMULATES adds into what is there (AccumulateGrad), not into a fresh slot
        return None
    return fn(w)


_WGRAD_SIDE = {"pixels": 0, "streams": {}}
_SIDE_TASK = [-1]           # autograd graph task the pending entries belong to
_SIDE_PENDING = []          # (weight, address of its gradient computed under the side stream) of the running backward pass -- the address
                            # only: a reference to the tensor would make autograd COPY it into .grad instead of moving it there


def set_wgrad_side_stream(max_pixels: int = 0):
    """Weight gradients beside the data-gradient chain (opt-in; parallel.GradientExchange switches it on for a single-rank job).  Nothing in a
    backward pass reads a layer's weight gradient, and from 1/4 resolution down neither gradient kernel of a layer fills the chip: with
    max_pixels > 0 the weight gradient of every layer whose top and bottom maps have at most that many pixels runs on a second HIP stream
    (FlowNetC train step, batch 8 @448x320: 9.46-9.52 -> 9.33 ms with 36000 = every layer but the stem).  The main stream waits for it when the
    backward pass ends (an autograd-engine callback; outside the engine -- the prototxt executor -- the gradient stays on the main stream).
    Constraints, checked where they can be: the weight has no gradient yet (a pass that ACCUMULATES stays on the main stream) and feeds ONE
    layer of the graph (the engine would add two gradients of a shared weight before the join); nothing reads `.grad` inside the pass
    (GradientExchange's hooks with a collective only COUNT the gradients and launch a bucket's all-reduce on the side stream itself, behind
    the kernels that produce it: side_stream_for_collective).  0 = off (default)."""
    _WGRAD_SIDE["pixels"] = int(max_pixels)


def side_stream_for_collective(device):
    """The stream a gradient bucket's all-reduce has to be ordered behind when weight gradients run on the second stream: that stream, made
    to wait for everything the main stream has been given so far (bias / flow-head / stem gradients are produced there).  The collective
    library orders its own stream behind the CURRENT stream at launch, so the caller launches under `torch.cuda.stream(side)`.  None when
    the second stream is not in use (the collective is then ordered behind the main stream as usual)."""
    if not _WGRAD_SIDE["pixels"]:
        return None
    st = _WGRAD_SIDE["streams"].get(device)
    if st is None:
        return None
    st.wait_stream(torch.cuda.current_stream(device))
    return st


def _wgrad_side_stream(d, x, w):
    if not _WGRAD_SIDE["pixels"] or not d.is_cuda or w.grad is not None or max(d.shape[2] * d.shape[3], x.shape[2] * x.shape[3]) > _WGRAD_SIDE["pixels"]:
        return None
    task = torch._C._current_graph_task_id()
    if task < 0:                # not inside the autograd engine (Net.Backward of the prototxt executor): nobody would join
        return None
    if task != _SIDE_TASK[0]:   # first one of this backward pass: the join rides on its end
        if _SIDE_PENDING:       # a pass that died on the way (an exception in some backward) left entries behind: settle them first
            _SIDE_PENDING.clear()
            for dev, st in _WGRAD_SIDE["streams"].items():
                torch.cuda.current_stream(dev).wait_stream(st)
        torch.autograd.Variable._execution_engine.queue_callback(join_side_streams)
        _SIDE_TASK[0] = task
    st = _WGRAD_SIDE["streams"].get(d.device)
    if st is None:
        st = _WGRAD_SIDE["streams"][d.device] = torch.cuda.Stream(device=d.device)
    return st


def join_side_streams():
    """The current stream waits for the weight gradients computed beside it.  A gradient the engine COPIED or ADDED instead of moving it into
    `.grad` was read before it was complete (a weight shared by two layers, a retained graph ...): that is an error, not a silent race."""
    _SIDE_TASK[0] = -1
    if not _SIDE_PENDING:
        return
    for dev, st in _WGRAD_SIDE["streams"].items():
        torch.cuda.current_stream(dev).wait_stream(st)
    pending = list(_SIDE_PENDING)
    _SIDE_PENDING.clear()
    if _GRAD_SLOT[0] is not None:       # a gradient exchange owns `.grad` (it copies what was not produced in its bucket slot -- on the second stream)
        return
    for w, ptr in pending:
        if ptr and w.grad is not None and w.grad.data_ptr() != ptr:
            raise RuntimeError("functional.set_wgrad_side_stream: autograd did not move a weight gradient computed on the second stream into "
                               ".grad as it was (shared weight? retained graph?): the result may have been read early.  Switch it off "
                               "(set_wgrad_side_stream(0)) for this graph.")


def relu_chain_supported(x_shape, w, stride, pad) -> bool:
    """Can a Convolution with this weight on a bottom of this shape fold the ReLU derivative of the layer in front into its data gradient
    (fn2_conv_backward_data_masked: the transposed-convolution route)?"""
    desc = _layer_desc(w, stride, pad, False, x_shape=x_shape)
    if desc is None or not w.is_cuda:
        return False
    route = ops.conv_backward_data_route(desc, False, bf16x3=_bf16x3("dgrad"))
    return route != 0 and ops.conv_backward_data_masked_supported(desc, False, route)


def conv_backward(x, w, y, g, stride, pad, slope, transposed, need_x, need_w, need_b, premasked=False, mask_bottom=None):
    """(bottom_diff, weight_diff, bias_diff) of a Convolution / Deconvolution (+ the leaky ReLU folded into it when `y`, the ACTIVATED
    output, is given) from top_diff g -- ConvolutionLayer / DeconvolutionLayer::Backward_gpu (conv_layer.cu:26-60, deconv_layer.cu:27-58)
    behind ReLULayer::Backward_gpu (relu_layer.cu:33-60).  One fused pass undoes the activation and reduces the bias gradient
    (csrc/bias_act.hip, from the saved output), the two convolution gradients run on the library's own routes (fn2_conv_backward_*); a
    geometry without an own kernel goes to the counted last resort (aten::convolution_backward).  Shared by the autograd function above
    and by the prototxt executor's Convolution / Deconvolution mirrors (stock_layers.py)."""
    if y is not None and premasked:
        # the ONE consumer of this layer's output folded this layer's ReLU derivative into its data gradient (relu_chain): g is top_diff of
        # the convolution itself.  The bias gradient comes out of the weight-gradient kernel where that has the fused form (the stem), else
        # from a read-only reduction pass
        d = g.contiguous()
        db = None
        if need_w and need_b and not transposed and d.is_cuda:
            desc = _layer_desc(w, stride, pad, False, x_shape=x.shape)
            if desc is not None and ops.conv_backward_weights_bias_fused(desc, False) and x.is_contiguous():
                gw, db = ops.conv_backward_weights_bias(x, d, desc, False, out=_grad_slot(w))
                gx = _own_bwd_data(d, w, stride, pad, transposed, x.shape) if need_x else None
                if not need_x or gx is not None:
                    return gx, gw, db
        if need_b:
            db = ops.conv_backward_bias(d, d.shape[1])
    elif y is not None:
        # the gradient of a Concat arrives as a channel-slice view of the Concat's top_diff: read in place (no .contiguous() copy)
        gb, g0 = _channel_slice(g)
        if not isinstance(y, tuple):                    # (a tuple: an output that lives in its consumer's Concat blob, read in place too)
            yb, y0 = _channel_slice(y)
            y = (yb, y0, y.shape[1])
        d, db = ops.bias_leaky_relu_backward(y, (gb, g0, g.shape[1]), slope, need_b)
    else:
        g = g.contiguous()
        d, db = g, (g.sum((0, 2, 3)) if need_b else None)
    gx = None
    if need_x and mask_bottom is not None:
        gx = _own_bwd_data_masked(d, w, stride, pad, x, mask_bottom)
    if need_x and gx is None:
        if mask_bottom is not None:
            raise RuntimeError("relu_chain: the data gradient of this layer has no masked form (relu_chain_supported was not asked?)")
        gx = _own_bwd_data(d, w, stride, pad, transposed, x.shape)
    gw = None
    if need_w:
        side = _wgrad_side_stream(d, x, w)
        if side is None:
            gw = _own_bwd_weight(d, x, w, stride, pad, transposed)
        else:
            # the weight gradient of a small map is off the critical path (nothing in the backward pass reads it) and does not fill the chip:
            # beside the data-gradient chain on a second stream; join_side_streams() before the optimizer / the gradient exchange reads it
            main = torch.cuda.current_stream(d.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                gw = _own_bwd_weight(d, x, w, stride, pad, transposed)
            if gw is None:
                main.wait_stream(side)
            else:
                for t in (d, x):
                    t.record_stream(side)                 # read under the side stream, freed under the main one
                gw.record_stream(main)
                _SIDE_PENDING.append((w, gw.data_ptr()))
    lib_x, lib_w = need_x and gx is None, need_w and gw is None
    if (lib_x or lib_w) and os.environ.get("FN2_TRACE_BWD") == "1":
        print("bwd on the library: x %s w %s stride %d pad %d transposed %s -> %s%s" % (tuple(x.shape), tuple(w.shape), stride, pad, transposed,
                                                                                      "data " if lib_x else "", "weight" if lib_w else ""), flush=True)
    if lib_x or lib_w:
        if x.is_cuda:       # counted like the forward's last resort: `library_conv_fallbacks: 0` in the bench line covers backward too
            _note_fallback("%s backward{stride %d, pad %d}%s%s" % ("Deconvolution" if transposed else "Convolution", stride, pad,
                                                                   " data" if lib_x else "", " weight" if lib_w else ""), x, w)
        # deterministic library solvers (MIOpen's DETERMINISTIC attribute): with its default solvers the weight gradients of the small-channel
        # first layers (FlowNet-SD's / the fusion net's conv0, 6 / 11 inputs) differed from run to run
        cd, was = torch.backends.cudnn, torch.backends.cudnn.deterministic
        cd.deterministic = True
        try:
            gxl, gwl, _ = torch.ops.aten.convolution_backward(d, x, w, None, [stride, stride], [pad, pad], [1, 1], transposed, [0, 0], 1,
                                                              [lib_x, lib_w, False])
        finally:
            cd.deterministic = was
        gx, gw = (gxl if lib_x else gx), (gwl if lib_w else gw)
    return gx, gw, db


def _layer_desc(w, stride, pad, transposed, x_shape=None, d_shape=None):
    """fn2_conv_desc of the layer that owns weight blob w ([Cout, Cin, k, k]; Deconvolution: [Cin, Cout, k, k]) from its bottom shape, or --
    where that is unambiguous (stride 1; Deconvolution{4, 2, 1}) -- from the shape of its top_diff."""
    k = int(w.shape[2])
    if w.shape[3] != k:
        return None
    Cin, Cout = (int(w.shape[0]), int(w.shape[1])) if transposed else (int(w.shape[1]), int(w.shape[0]))
    if x_shape is not None:
        N, H, W = int(x_shape[0]), int(x_shape[2]), int(x_shape[3])
    elif transposed and d_shape[2] % 2 == 0 and d_shape[3] % 2 == 0:
        N, H, W = int(d_shape[0]), int(d_shape[2]) // 2, int(d_shape[3]) // 2
    elif not transposed and stride == 1:
        N, H, W = int(d_shape[0]), int(d_shape[2]) - 1 + k - 2 * pad, int(d_shape[3]) - 1 + k - 2 * pad
    else:
        return None
    if H < 1 or W < 1:
        return None
    return ops.conv_desc(N, Cin, H, W, Cout, k, stride, pad)


def _own_bwd_weight(d, x, w, stride, pad, transposed):
    """weight_diff of a Convolution (ConvolutionLayer::Backward_gpu -> weight_gpu_gemm, conv_layer.cu:40-52) or Deconvolution
    (deconv_layer.cu:36-50, the roles of the two blobs swapped) on the own fp32 MFMA kernels: NCHW in, weight layout out, no layout
    transposes, deterministic.  Which kernel (the stem's taps-on-N kernel, csrc/conv_stem_wgrad.hip, or csrc/conv_wgrad.hip) is the library's
    decision (fn2_conv_backward_weights, csrc/conv_route.cpp -- the Caffe adapter's Backward_gpu calls the same function).  Returns None when
    no own kernel applies (tap classes 1/1, 3/1, 3/2, 4/2, 5/2 and the stem; layers with fewer than 16 channels on either side -- the
    2-channel flow heads -- have kernels of their own)."""
    if not d.is_cuda:
        return None
    desc = _layer_desc(w, stride, pad, transposed, x_shape=x.shape)
    if desc is None or not ops.conv_backward_weights_supported(desc, transposed):
        return None
    if (not transposed and desc.kernel == 7) and not (d.is_contiguous() and x.is_contiguous()):
        d, x = d.contiguous(), x.contiguous()           # the stem kernel reads whole blobs
    xb, x0 = _channel_slice(x)
    db, d0 = _channel_slice(d)
    return ops.conv_backward_weights(xb, db, desc, transposed, out=_grad_slot(w), bottom_c0=x0, top_c0=d0,
                                     bf16x3=not transposed and _bf16x3("wgrad"))


# (id(weight tensor), tag) -> (weak reference, _version, packed operand, weight generation), see _cached: the operand of a layer's
# forward ("fwd") or data-gradient ("dgrad") route
_PACKED_T = {}


def _cached_pack(cache, w, tag, make):
    return _cached(cache, (id(w), tag), w, make)


def _own_bwd_data(d, w, stride, pad, transposed, x_shape=None):
    """bottom_diff on the own kernels (ConvolutionLayer::Backward_gpu, conv_layer.cu:53-57: backward_gpu_gemm = weight^T x top_diff +
    col2im; DeconvolutionLayer::Backward_gpu, deconv_layer.cu:52-56: forward_gpu_gemm of top_diff).  The kernel is the library's choice
    (fn2_conv_backward_data_route, csrc/conv_route.cpp: Winograd on the rotated weights for 3x3 / 1, the transposed-convolution kernel for the
    stride-2 layers, the 4x4 / 2 convolution for a Deconvolution, the small-map kernels on 10x14 / 5x7 maps, the 1x1 kernel on the transposed
    weight); its operand is packed once per weight version.  Returns None when no own kernel applies."""
    if not d.is_cuda:
        return None
    desc = _layer_desc(w, stride, pad, transposed, x_shape=x_shape, d_shape=d.shape)
    if desc is None:
        return None
    route = ops.conv_backward_data_route(desc, transposed, bf16x3=_bf16x3("dgrad"))
    if route == 0:
        return None
    key = (desc.N, desc.Hin, desc.Win)       # the route (and with it the operand's layout) is a function of the layer geometry
    packed = _cached_pack(_PACKED_T, w, ("dgrad", route, bool(transposed), stride, pad) + key,
                          lambda: ops.conv_backward_data_pack_weights(w.detach().contiguous(), desc, transposed, route))
    db, d0 = _channel_slice(d)
    return ops.conv_backward_data(db, packed, desc, transposed, route, top_c0=d0)


def _own_bwd_data_masked(d, w, stride, pad, x, slope):
    """_own_bwd_data with ReLUBackward of the layer in front folded in: x is this layer's bottom = that layer's activated output."""
    desc = _layer_desc(w, stride, pad, False, x_shape=x.shape)
    if desc is None or not d.is_cuda:
        return None
    route = ops.conv_backward_data_route(desc, False, bf16x3=_bf16x3("dgrad"))
    if route == 0 or not ops.conv_backward_data_masked_supported(desc, False, route):
        return None
    key = (desc.N, desc.Hin, desc.Win)
    packed = _cached_pack(_PACKED_T, w, ("dgrad", route, False, stride, pad) + key,
                          lambda: ops.conv_backward_data_pack_weights(w.detach().contiguous(), desc, False, route))
    db, d0 = _channel_slice(d)
    xb, x0 = _channel_slice(x)
    return ops.conv_backward_data_masked(db, packed, desc, False, route, xb, slope, top_c0=d0, data_c0=x0)


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def conv_forward_route(desc, act=True, whole_blobs=True) -> int:
    """The own kernel conv_mfma_relu runs this Convolution on (0 = none): the library's choice (fn2_conv_route, csrc/conv_route.cpp: thresholds,
    batch-invariant mode -- the one the Caffe adapter's Convolution gets) minus the layers this module does not serve."""
    route = ops.conv_forward_route(desc, force=_ROUTE_FORCE[0], bf16x3=_bf16x3("conv"), wino_bf16x3=_bf16x3("wino"))
    stem = route == ops.CONV_ROUTE_STEM
    if route == ops.CONV_ROUTE_HEAD:                      # the predict_flow heads: predict_flow_conv, with an autograd function of its own
        return ops.CONV_ROUTE_NONE
    if stem and not (act and whole_blobs):                # the stem kernel: only with its fused ReLU, from and into whole blobs
        return ops.CONV_ROUTE_NONE
    if desc.kernel not in (1, 3, 5, 7) or (desc.kernel == 7 and not stem and desc.Cin % 4 != 0):
        return ops.CONV_ROUTE_NONE                        # the direct kernel on 4x4 taps, or on 7x7 taps off whole channel quads
    return route


def deconv_forward_route(desc, act=True) -> int:
    """The own kernel deconv_relu runs this Deconvolution{4, 2, 1} on (0 = none): fn2_deconv_route minus the layers this module does not serve."""
    if not act or desc.Cin < 64:                          # no fused ReLU asked for; fewer than 64 input channels
        return ops.DECONV_ROUTE_NONE
    route = ops.deconv_forward_route(desc, bf16x3=_bf16x3("deconv"))
    return ops.DECONV_ROUTE_NONE if route == ops.DECONV_ROUTE_HEAD else route      # (2 -> 2: upsample_flow_deconv, with an autograd function of its own)


def conv_route_name(x_shape, w, stride, pad, act=True, whole_blobs=True):
    """Name (ops.CONV_FWD_ROUTES) of the kernel conv_mfma_relu runs this layer on for a CUDA bottom of this shape, None = declined: "stem"
    is the one relu_chain producer; the FN2_TRACE_CONV print of nets.py.  A layer run in split-bf16 arithmetic: "direct+bf16x3" / "wino+bf16x3"."""
    desc = _layer_desc(w, stride, pad, False, x_shape=x_shape)
    if desc is None:
        return None
    route = conv_forward_route(desc, act, whole_blobs)
    name = ops.CONV_FWD_ROUTES[route & ~ops.CONV_ARITH_BF16X3]
    return name + "+bf16x3" if name and route & ops.CONV_ARITH_BF16X3 else name


def conv_mfma_relu(x, weight, bias, stride, pad, negative_slope=0.1, act=True, out=None, out_c0=0, relu_chain=None):
    """Convolution + bias (+ leaky ReLU) on the own kernel the LIBRARY routes the layer to, NCHW in and out, optionally written into a channel
    slice of `out`: descriptor -> route -> the route's packed operand (once per weight version) -> fn2_conv_forward, the call sequence of the
    Caffe adapter's Convolution (Winograd F(2x2, 3x3), the small-map kernel, the direct kernel, the 7x7 / 2 stem).  With autograd active the
    same forward runs inside _OwnForwardConv (own backward routes).  Returns None when no own kernel takes the layer: the caller then runs
    the counted library convolution."""
    desc = _layer_desc(weight, stride, pad, False, x_shape=x.shape) if x.is_cuda else None
    route = conv_forward_route(desc, act, out is None) if desc is not None else ops.CONV_ROUTE_NONE
    if route == ops.CONV_ROUTE_NONE:
        return None
    if relu_chain is not None and int(relu_chain[0]) & 1 and route != ops.CONV_ROUTE_STEM:
        raise RuntimeError("relu_chain: only the stem layer is a chain producer")

    def run(xx, ww, bb, o=None, o0=0):
        # ww is the parameter itself (autograd does not record inside _OwnForwardConv.forward): the packed operand is cached on it
        if route == ops.CONV_ROUTE_STEM:                # the stem kernel reads a whole blob, and the weight blob as it is
            blob, c0, packed = xx.contiguous(), 0, ww.detach().contiguous()
        else:
            blob, c0 = _channel_slice(xx)
            # (the operand's layout is a function of the route and the weight's shape: one copy per weight, whatever the bottom's size)
            packed = _cached_pack(_PACKED_T, ww, ("fwd", route, False), lambda: ops.conv_pack_weights(ww.detach(), desc, route))
        return ops.conv_forward(blob, packed, bb, desc, route, False, act, negative_slope, out=o, out_c0=o0, in_c0=c0)

    if _needs_grad(x, weight, bias):
        return _OwnForwardConv.apply(x, weight, bias, run, stride, pad, negative_slope, act, False, None if out is None else (out, out_c0), relu_chain)
    return run(x, weight, bias, out, out_c0)


def deconv_relu(x, weight, bias, negative_slope=0.1, act=True, out=None, out_c0=0):
    """Deconvolution{4, 2, 1} + bias + leaky ReLU on the own kernel the LIBRARY routes the layer to (fn2_deconv_route: weight^T x bottom on the
    1x1 MFMA kernel + our col2im / bias / ReLU pass as the reference computes it, base_conv_layer.cpp:375-384; the parity-class small-map
    kernel for the planes the GEMM does not take, 5x7), optionally written into a channel slice of `out` (the consumer's Concat blob).
    weight: Caffe's [Cin, Cout, 4, 4] blob; the operand is packed from it as it is (the GEMM's through the strided view, no transposed
    copy).  The call sequence of the Caffe adapter's Deconvolution; with autograd active inside _OwnForwardConv.  Returns None when no own
    kernel takes the layer."""
    desc = _layer_desc(weight, 2, 1, True, x_shape=x.shape) if x.is_cuda else None
    route = deconv_forward_route(desc, act) if desc is not None else ops.DECONV_ROUTE_NONE
    if route == ops.DECONV_ROUTE_NONE:
        return None

    def run(xx, ww, bb, o=None, o0=0):
        blob, c0 = _channel_slice(xx)
        packed = _cached_pack(_PACKED_T, ww, ("fwd", route, True), lambda: ops.conv_pack_weights(ww.detach(), desc, route, True))
        return ops.conv_forward(blob, packed, bb, desc, route, True, True, negative_slope, out=o, out_c0=o0, in_c0=c0)

    if _needs_grad(x, weight, bias):
        return _OwnForwardConv.apply(x, weight, bias, run, 2, 1, negative_slope, True, True, None if out is None else (out, out_c0))
    return run(x, weight, bias, out, out_c0)
