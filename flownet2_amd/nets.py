"""FlowNetC / FlowNetS graphs as the reference's deploy prototxts wire them.

TOPOLOGY CAVEAT: the prototxt templates are NOT in the reference tree (models/download-models.sh:3-10
fetches them); the graphs below restate them from the FlowNet / FlowNet2 papers and the layer names
third-party converters use.  Every topology assumption lives in this file.

Every layer goes through `backend`: flownet2_amd.functional (HIP kernels) in the product, oracle.backend or a minimal namespace on the
host.  Each public entry turns it into a graph_backend.GraphBackend once (backend_of) and the graphs below are written against that adapter
(`be`): the custom layers (Correlation, Resample, FlowWarp, ChannelNorm, L1Loss, Downsample) by name; Convolution / Deconvolution / ReLU
(conv_layer.cpp:8-40, deconv_layer.cpp:8-45, relu_layer.cu:8-14) through be.conv / be.deconv / be.predict_flow / be.upsample_flow: the own
MFMA kernels (functional.conv_mfma_relu / deconv_relu, optionally writing into a channel slice of the consumer's Concat blob), and what
they decline -- or a backend without them -- on the counted library convolution or plain torch (conv2d / conv_transpose2d).  What a
backend can do is asked in the adapter alone; listening(fn) sees every layer that ran.  Caffe's weight layouts ([Cout,Cin,kh,kw], deconv
[Cin,Cout,kh,kw], base_conv_layer.cpp:125-139) are torch's, so .caffemodel blobs load without transposition.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional

import torch

from .graph_backend import NEG_SLOPE, GraphBackend, backend_of, listening  # noqa: F401

FLOW_SCALE = 20.0        # deploy multiplies predict_flow2 by 20 (training divides GT by 20)
SD_FLOW_SCALE = 0.05     # FlowNet-SD predicts in units of 0.05 px: its deploy branch multiplies by 0.05 (released FlowNet2 graph; flownetsd_flow2 / div_flow in the third-party ports)
LOSS_WEIGHTS = {6: 0.32, 5: 0.08, 4: 0.02, 3: 0.01, 2: 0.005}   # Appendix B (memory)

# name: (kind, Cin, Cout, k, stride, pad)
_ENC_TAIL = [("conv4", 256, 512, 3, 2, 1), ("conv4_1", 512, 512, 3, 1, 1), ("conv5", 512, 512, 3, 2, 1),
             ("conv5_1", 512, 512, 3, 1, 1), ("conv6", 512, 1024, 3, 2, 1), ("conv6_1", 1024, 1024, 3, 1, 1)]
_DEC = [("Convolution1", "conv", 1024, 2), ("deconv5", "deconv", 1024, 512), ("upsample_flow6to5", "deconv", 2, 2),
        ("Convolution2", "conv", 1026, 2), ("deconv4", "deconv", 1026, 256), ("upsample_flow5to4", "deconv", 2, 2),
        ("Convolution3", "conv", 770, 2), ("deconv3", "deconv", 770, 128), ("upsample_flow4to3", "deconv", 2, 2),
        ("Convolution4", "conv", 386, 2), ("deconv2", "deconv", 386, 64), ("upsample_flow3to2", "deconv", 2, 2),
        ("Convolution5", "conv", 194, 2)]


def layer_table(kind: str = "C", in_channels: int = 6):
    """[(name, 'conv'|'deconv', Cin, Cout, k, stride, pad)] in execution order."""
    t = []
    if kind == "C":
        t += [("conv1", "conv", 3, 64, 7, 2, 3), ("conv2", "conv", 64, 128, 5, 2, 2), ("conv3", "conv", 128, 256, 5, 2, 2),
              ("conv_redir", "conv", 256, 32, 1, 1, 0), ("conv3_1", "conv", 473, 256, 3, 1, 1)]
    else:
        t += [("conv1", "conv", in_channels, 64, 7, 2, 3), ("conv2", "conv", 64, 128, 5, 2, 2), ("conv3", "conv", 128, 256, 5, 2, 2),
              ("conv3_1", "conv", 256, 256, 3, 1, 1)]
    t += [(n, "conv", ci, co, k, s, p) for (n, ci, co, k, s, p) in _ENC_TAIL]
    for (n, k, ci, co) in _DEC:
        t.append((n, k, ci, co, 3, 1, 1) if k == "conv" else (n, k, ci, co, 4, 2, 1))
    return t


def init_params(kind: str = "C", seed: int = 0, device="cpu", in_channels: int = 6) -> Dict[str, torch.Tensor]:
    """Seeded synthetic weights (no .caffemodel can be downloaded here): He-normal for the leaky
    convs, small predict_flow / upsample heads so flows come out O(1-10 px); biases 0."""
    g = torch.Generator().manual_seed(seed)
    params = {}
    for (name, k, ci, co, ks, s, p) in layer_table(kind, in_channels):
        shape = (co, ci, ks, ks) if k == "conv" else (ci, co, ks, ks)
        fan_in = ci * ks * ks if k == "conv" else ci * ks * ks / (s * s)
        std = math.sqrt(2.0 / ((1 + NEG_SLOPE ** 2) * fan_in))
        if name.startswith("Convolution"):
            std *= 0.5
        if name.startswith("upsample_flow"):
            std = 0.25
        params[name + ".w"] = (torch.randn(shape, generator=g) * std).to(device)
        params[name + ".b"] = torch.zeros(co).to(device)
    return params


def num_params(params) -> int:
    return sum(int(v.numel()) for v in params.values())


def conv_forward(x, w, b, stride, pad, act, backend, slope=None, relu_chain=None):
    """Convolution{w, stride, pad} + bias (+ ReLU{NEG_SLOPE} when act) on explicit tensors: the call every graph of this file (be.conv) and the
    Convolution layer of the prototxt executor (flownet2_amd.layers.ConvolutionLayer) share -- same kernels, same bits.  The backend routes
    (functional.conv_mfma_relu: the library's fn2_conv_route); what it declines is the counted library convolution's."""
    return backend_of(backend).conv_wb(x, w, b, stride, pad, act, NEG_SLOPE if slope is None else slope, relu_chain=relu_chain)


_LAST_ROUTE = [""]


def _note_route(name, y, info):
    """Listener: which kernel a convolution ran on, into _LAST_ROUTE[0]."""
    if info["kind"] != "conv":
        return
    be, x, w = info["backend"], info["x"], info["w"]
    if not info["own"]:
        _LAST_ROUTE[0] = "library conv2d"
    elif be.conv_route_name is None:
        _LAST_ROUTE[0] = "own kernel"
    else:
        _LAST_ROUTE[0] = "fn2 %s" % be.conv_route_name(x.shape, w, info["stride"], info["pad"], info["act"], not info["into"])


def _trace_route(name, y, info):
    """Listener of FN2_TRACE_CONV=1: one line per convolution."""
    if info["kind"] == "conv":
        _note_route(name, y, info)
        print("conv route %-16s in %-22s k%d s%d act=%d -> %s%s" % (name, tuple(info["x"].shape), info["w"].shape[2], info["stride"], info["act"],
                                                                  _LAST_ROUTE[0], " (into its Concat blob)" if info["into"] else ""))


if os.environ.get("FN2_TRACE_CONV") == "1":
    listening(_trace_route).__enter__()


_CONSTS: Dict[tuple, torch.Tensor] = {}


def _const(device, values):
    """Small fp32 device constants (mean, output scale), uploaded once: no host-to-device copy inside a step, so a
    step can be captured into a hipGraph."""
    key = (str(device), tuple(float(v) for v in values))
    if key not in _CONSTS:
        _CONSTS[key] = torch.tensor(key[1], device=device, dtype=torch.float32)
    return _CONSTS[key]


def deconv_forward(x, w, b, act=True, backend=None, slope=None):
    """Deconvolution{4, 2, 1} + bias (+ ReLU): the call shared with flownet2_amd.layers.DeconvolutionLayer.  The backend routes
    (functional.deconv_relu: the library's fn2_deconv_route); what it declines is the counted library deconvolution's."""
    return backend_of(backend).deconv_wb(x, w, b, act, NEG_SLOPE if slope is None else slope)


def _conv_into_concat(x, P, name, stride, pad, extra_channels, be, relu_chain=None):
    """A convolution whose output is the FIRST input of a Concat (a decoder skip tensor): where an own kernel writes into a channel slice
    and -- in a training graph -- the backend trains in place, the Concat blob [N, Cout + extra_channels, H, W] is allocated here and the
    convolution writes its channels straight into it (ConcatLayer, concat_layer.cu:8-52, becomes a no-op for this input).  Returns (blob or
    None, the layer's output -- a channel-slice view of the blob, or an ordinary tensor)."""
    w = P[name + ".w"]
    # The blob route writes the later Concat inputs in place (deconvolution, upsampled flow).  Without autograd what those calls return is
    # discarded.  With autograd every producer is an autograd function whose output is its slice view of the blob -- a plain buffer outside
    # the graph -- and _ConcatInPlace ties the slices together for the consumer: no Concat copy in a training step either.
    training = torch.is_grad_enabled() and (x.requires_grad or _any_requires_grad(P))
    if be.writes_slices and w.shape[2] in (3, 5) and (be.trains_in_place or not training):
        k = w.shape[2]
        ho, wo = (x.shape[2] + 2 * pad - k) // stride + 1, (x.shape[3] + 2 * pad - k) // stride + 1
        blob = torch.empty((x.shape[0], w.shape[0] + extra_channels, ho, wo), device=x.device, dtype=x.dtype)
        y = be.own_conv(x, w, P[name + ".b"], stride, pad, NEG_SLOPE, True, out=blob, out_c0=0, relu_chain=relu_chain)
        if y is not None:
            be.wrote("conv", name, y, blob, 0, w.shape[0], x, w, stride, pad)
            return blob, (y if (training and y.requires_grad) else blob[:, :w.shape[0]])
    if relu_chain is not None:
        raise RuntimeError("relu_chain: conv '%s' left the own-kernel route after its producer was told it would fold the ReLU derivative" % name)
    return None, be.conv(x, P, name, stride, pad)


def _any_requires_grad(P) -> bool:
    vals = P.P.values() if isinstance(P, _Prefixed) else P.values()
    return any(v.requires_grad for v in vals)


def _refine_stage(P, skip, x, dname, flow, uname, be, upsampled=False):
    """One refinement Concat [skip | ReLU(deconv(x)) | upsampled flow].  `skip` is a tensor or a pair (concat blob, tensor) from
    _conv_into_concat: with a blob the Concat layer (concat_layer.cu:8-52) has nothing to copy -- the skip convolution already wrote its
    channels there, and the deconvolution and the upsampled flow are written behind them by their own kernels.  upsampled: _head_into_stage
    has written the upsampled flow into the blob already."""
    blob, s = skip if isinstance(skip, tuple) else (None, skip)
    if blob is None:
        return torch.cat([s, be.deconv(x, P, dname), be.upsample_flow(flow, P, uname)], 1)
    wd, bd = P[dname + ".w"], P[dname + ".b"]
    cs, cd = s.shape[1], wd.shape[1]
    assert blob.shape[1] == cs + cd + 2
    # ReLU(deconv(x)) written into channels [cs, cs + cd) of the blob (with autograd: d is the slice view that carries the graph)
    d = be.own_deconv(x, wd, bd, NEG_SLOPE, True, out=blob, out_c0=cs)
    if d is not None:
        be.wrote("deconv", dname, d, blob, cs, cd, x, wd, 2, 1)
    stage_params = [wd, bd, P[uname + ".w"], P[uname + ".b"]]
    if torch.is_grad_enabled() and (s.requires_grad or x.requires_grad or flow.requires_grad or any(p.requires_grad for p in stage_params)):
        # training (also a partial freeze whose first trainable tensors are this stage's own deconvolution / up-sampling weights): the
        # three producers are autograd functions that wrote / write their slices; _ConcatInPlace hands the consumer the blob
        u = be.upsample_flow(flow, P, uname, out=blob, out_c0=cs + cd) if d is not None else None
        if d is None or u is None:          # a producer without an own kernel for this shape: the stock Concat (a copy) for this stage
            return torch.cat([s, be.deconv(x, P, dname), be.upsample_flow(flow, P, uname)], 1)
        part = lambda t, c0, c: t if t.requires_grad else blob[:, c0:c0 + c]      # (a frozen producer returned the blob it wrote into)
        return _ConcatInPlace.apply(blob, s, part(d, cs, cd), part(u, cs + cd, 2))
    if d is None:
        blob[:, cs:cs + cd].copy_(be.deconv(x, P, dname))
    if not upsampled and be.upsample_flow(flow, P, uname, out=blob, out_c0=cs + cd) is None:
        blob[:, cs + cd:].copy_(be.upsample_flow(flow, P, uname))
    return blob


def _head_into_stage(P, x, pname, skip, dname, uname, be):
    """predict_flow `pname` of x for the stage _refine_stage(P, skip, x, dname, flow, uname) that follows: (flow, upsampled).  Without
    autograd and with a Concat blob, the flow is up-sampled into its slice of that blob on the way (be.predict_upsample_flow: one launch
    less per stage), and the stage is told so."""
    blob, s = skip if isinstance(skip, tuple) else (None, skip)
    params = [P[n + k] for n in (pname, dname, uname) for k in (".w", ".b")]
    if blob is None or (torch.is_grad_enabled() and (s.requires_grad or x.requires_grad or any(p.requires_grad for p in params))):
        return be.predict_flow(x, P, pname), False
    return be.predict_upsample_flow(x, P, pname, uname, blob, s.shape[1] + P[dname + ".w"].shape[1])


def _decoder(P, conv6_1, conv5_1, conv4_1, conv3_1, conv2, be):
    """The refinement stages.  Every skip argument is a tensor or a pair (concat blob, tensor) from _conv_into_concat: with a blob the
    Concat layer (concat_layer.cu:8-52) has nothing to copy -- the skip convolution already wrote its channels there, and the
    deconvolution and the upsampled flow are written behind them by their own kernels."""
    # (Round 4 measured the flow head of every level on a second HIP stream beside that level's deconvolution: 2.366 ms per FlowNetC step against
    # 2.343 without -- the fork / join event pairs cost more than ~90 us of head kernels can hide behind GEMMs that fill every CU.  The branch was
    # removed in round 5; what a second stream pays for is LONG independent chains: FlowNet-SD beside the CSS stack, weight gradients beside data
    # gradients.)
    flow6, up = _head_into_stage(P, conv6_1, "Convolution1", conv5_1, "deconv5", "upsample_flow6to5", be)
    c5 = _refine_stage(P, conv5_1, conv6_1, "deconv5", flow6, "upsample_flow6to5", be, up)
    flow5, up = _head_into_stage(P, c5, "Convolution2", conv4_1, "deconv4", "upsample_flow5to4", be)
    c4 = _refine_stage(P, conv4_1, c5, "deconv4", flow5, "upsample_flow5to4", be, up)
    flow4, up = _head_into_stage(P, c4, "Convolution3", conv3_1, "deconv3", "upsample_flow4to3", be)
    c3 = _refine_stage(P, conv3_1, c4, "deconv3", flow4, "upsample_flow4to3", be, up)
    flow3, up = _head_into_stage(P, c3, "Convolution4", conv2, "deconv2", "upsample_flow3to2", be)
    c2 = _refine_stage(P, conv2, c3, "deconv2", flow3, "upsample_flow3to2", be, up)
    flow2 = be.predict_flow(c2, P, "Convolution5")
    return {2: flow2, 3: flow3, 4: flow4, 5: flow5, 6: flow6}


def _skip_conv(x, P, name, stride, pad, dname, be, relu_chain=None):
    """An encoder convolution whose output is also the first input of a refinement Concat: (concat blob or None, output tensor)."""
    return _conv_into_concat(x, P, name, stride, pad, P[dname + ".w"].shape[1] + 2, be, relu_chain=relu_chain)


RELU_CHAIN = [True]      # A/B hook: False = every layer undoes its own ReLU in a pass of its own (rounds 1-5)


def _stem_chain(P, x, be):
    """conv1 -> conv2 in a TRAINING graph: conv2 is conv1's only consumer, so ReLUBackward of conv1 is folded into the epilogue of conv2's data
    gradient (the transposed 5x5 / 2 convolution) and conv1's bias gradient comes out of its weight-gradient kernel: no pass over the largest
    activation of the net (147 MB at batch 8 @448x320: read twice, written once) between the two.  Returns the (producer, consumer) handles
    for the two layers, or (None, None)."""
    if not (RELU_CHAIN[0] and be.has_stem_chain and torch.is_grad_enabled() and x.is_cuda):
        return None, None
    w1, w2 = P["conv1.w"], P["conv2.w"]
    if not (w1.requires_grad and w2.requires_grad and P["conv1.b"].requires_grad) or x.requires_grad:
        return None, None
    if be.conv_route_name(x.shape, w1, 2, 3) != "stem":                       # (conv1 must take the stem kernel: whole blobs)
        return None, None
    c1_shape = (x.shape[0], w1.shape[0], (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1)
    if not be.relu_chain_supported(c1_shape, w2, 2, 2):
        return None, None
    cell = {"masked": False, "slope": NEG_SLOPE}
    return (1, cell), (2, cell)


class _ConcatInPlace(torch.autograd.Function):
    """Concat (concat_layer.cu:8-52 / :62-90) of tensors that already ARE consecutive channel slices of `blob`: nothing to copy forward, the
    gradient of each is its slice of top_diff (a view: the producers' backward kernels read it in place)."""

    @staticmethod
    def forward(ctx, blob, *parts):
        ctx.cuts = [p.shape[1] for p in parts]
        assert sum(ctx.cuts) == blob.shape[1] and all(p.data_ptr() >= blob.data_ptr() for p in parts)
        return blob.view_as(blob)

    @staticmethod
    def backward(ctx, g):
        out, c0 = [None], 0
        for c in ctx.cuts:
            out.append(g[:, c0:c0 + c])
            c0 += c
        return tuple(out)


class _SplitTowers(torch.autograd.Function):
    """The stacked siamese batch [2N, ...] -> (first tower, second tower).  Two plain slices cost the backward pass two zero-fills of the
    stacked shape, two strided copies and an add (SliceBackward twice, then the sum); here it is ONE concatenation of the two gradients."""

    @staticmethod
    def forward(ctx, x):
        n = x.shape[0] // 2
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        return torch.cat([ga, gb], 0)


class _StackedAndFirstTower(torch.autograd.Function):
    """The stacked batch as it is (for the next tower layer) AND its first tower (the skip connection into the refinement).  The skip's
    gradient is added into the first half of the stacked gradient in place -- instead of a zero-fill of the stacked shape, a strided copy
    and a full-size add."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x[:x.shape[0] // 2]

    @staticmethod
    def backward(ctx, g_all, g_first):
        # g_all is the data gradient of the ONE layer that read output 0 (conv3's transposed convolution), produced for this node alone: both
        # outputs are locals of flownet_c_core -- nobody outside can hang a tensor hook or retain_grad on them, and a retained graph
        # recomputes g_all on its next pass -- so the skip gradient is added in place (a clone is 146 MB of traffic per step).  A gradient
        # that arrives as a view of something else is NOT ours to write: copy then.
        if g_all._base is not None or not g_all.is_contiguous():
            g_all = g_all.clone(memory_format=torch.contiguous_format)
        g_all[:g_first.shape[0]].add_(g_first)
        return g_all


_CORR = dict(pad=20, kernel_size=1, max_displacement=20, stride_1=1, stride_2=2)      # FlowNetC's Correlation layer: 21 x 21 = 441 planes


def flownet_c_core(P, img0, img1, backend, towers=None):
    """Pre-processed images [N,3,H,W] (H, W multiples of 64) -> {scale: flow prediction /20}.  `towers`: the two images already
    stacked along the batch axis [2N,3,H,W] (the deploy head writes them there directly)."""
    be = backend_of(backend)
    # siamese towers share weights (param { name: } sharing, net.cpp:451-540): one batch of 2N through conv1-3
    x = towers if towers is not None else torch.cat([img0, img1], 0)
    n = x.shape[0] // 2
    chain1, chain2 = _stem_chain(P, x, be)
    c1 = be.conv(x, P, "conv1", 2, 3, relu_chain=chain1)
    # conv2 of BOTH towers goes into a [2N, 128 + 64 + 2, h, w] blob: its first N samples are the concat2 blob of the refinement
    blob2, c2 = _skip_conv(c1, P, "conv2", 2, 2, "deconv2", be, relu_chain=chain2)
    training = torch.is_grad_enabled() and c2.requires_grad
    c2_first = None
    if training:
        c2, c2_first = _StackedAndFirstTower.apply(c2)
    c3 = be.conv(c2, P, "conv3", 2, 2)
    c3a, c3b = _SplitTowers.apply(c3) if (training and c3.requires_grad) else (c3[:n], c3[n:])
    # the correlation writes its 441 activated planes straight into the [conv_redir | corr] blob (no ReLU pass, no Concat pass), and
    # conv_redir (1x1: the own MFMA GEMM kernel) its 32 channels in front of them -- where the backend has these forms
    wr, br = P["conv_redir.w"], P["conv_redir.b"]
    cr = wr.shape[0]
    cat = None
    if be.fuses_correlation:
        cat = torch.empty((n, cr + 441, c3a.shape[2], c3a.shape[3]), device=c3a.device, dtype=c3a.dtype)
        if be.trains_in_place and torch.is_grad_enabled() and (c3a.requires_grad or c3b.requires_grad):
            # training: both producers are autograd functions that write their slice of the blob (conv_redir; the fused correlation + ReLU)
            redir = be.own_conv(c3a, wr, br, 1, 0, NEG_SLOPE, True, out=cat, out_c0=0)
            if redir is not None:
                be.wrote("conv", "conv_redir", redir, cat, 0, cr, c3a, wr, 1, 0)
            corr = be.own_correlation_relu_into(c3a, c3b, cat, cr, NEG_SLOPE, training=True, **_CORR)
            be.wrote("relu", "relu", corr, cat, cr, 441, c3a)
            if redir is not None and redir.requires_grad:
                cat = _ConcatInPlace.apply(cat, redir, corr)
            else:                                       # conv_redir without an own kernel for this shape (or frozen): the stock Concat
                cat = torch.cat([be.conv(c3a, P, "conv_redir", 1, 0), corr], 1)
        else:
            corr = be.own_correlation_relu_into(c3a, c3b, cat, cr, NEG_SLOPE, **_CORR)
            if corr is None:
                cat = None
            else:
                be.wrote("relu", "relu", corr, cat, cr, 441, c3a)
                redir = None
                if not (torch.is_grad_enabled() and _any_requires_grad(P)):
                    redir = be.own_conv(c3a, wr, br, 1, 0, NEG_SLOPE, True, out=cat, out_c0=0)
                if redir is None:
                    cat[:, :cr].copy_(be.conv(c3a, P, "conv_redir", 1, 0))
                else:
                    be.wrote("conv", "conv_redir", redir, cat, 0, cr, c3a, wr, 1, 0)
    if cat is None:
        redir = be.conv(c3a, P, "conv_redir", 1, 0)
        corr = be.correlation(c3a, c3b, **_CORR)
        cat = torch.cat([redir, be.leaky_relu(corr, "relu")], 1)
    blob3, c31 = _skip_conv(cat, P, "conv3_1", 1, 1, "deconv3", be)
    c4 = be.conv(c31, P, "conv4", 2, 1)
    blob4, c41 = _skip_conv(c4, P, "conv4_1", 1, 1, "deconv4", be)
    c5 = be.conv(c41, P, "conv5", 2, 1)
    blob5, c51 = _skip_conv(c5, P, "conv5_1", 1, 1, "deconv5", be)
    c6 = be.conv(c51, P, "conv6", 2, 1)
    c61 = be.conv(c6, P, "conv6_1", 1, 1)
    c2s = c2_first if c2_first is not None else c2[:n]
    skip2 = (blob2[:n], c2s) if blob2 is not None else c2s
    return _decoder(P, c61, (blob5, c51), (blob4, c41), (blob3, c31), skip2, be)


def flownet_s_core(P, x, backend=None):
    be = backend_of(backend)
    c1 = be.conv(x, P, "conv1", 2, 3)
    blob2, c2 = _skip_conv(c1, P, "conv2", 2, 2, "deconv2", be)
    c3 = be.conv(c2, P, "conv3", 2, 2)
    blob3, c31 = _skip_conv(c3, P, "conv3_1", 1, 1, "deconv3", be)
    c4 = be.conv(c31, P, "conv4", 2, 1)
    blob4, c41 = _skip_conv(c4, P, "conv4_1", 1, 1, "deconv4", be)
    c5 = be.conv(c41, P, "conv5", 2, 1)
    blob5, c51 = _skip_conv(c5, P, "conv5_1", 1, 1, "deconv5", be)
    c6 = be.conv(c51, P, "conv6", 2, 1)
    c61 = be.conv(c6, P, "conv6_1", 1, 1)
    return _decoder(P, c61, (blob5, c51), (blob4, c41), (blob3, c31), (blob2, c2), be)


def adapted_size(h: int, w: int, divisor: int = 64):
    """scripts/run-flownet.py:43-45."""
    return int(math.ceil(h / divisor) * divisor), int(math.ceil(w / divisor) * divisor)


def deploy_forward(kind: str, P, img0, img1, backend, mean: Optional[torch.Tensor] = None):
    """Deploy net: raw 0..255 BGR images [N,3,H,W] -> predict_flow_final [N,2,H,W] in pixels.

    Head/tail as in SURVEY.md Appendix B: Eltwise(1/255) -> Resample(ADAPTED, LINEAR) -> mean
    subtraction -> net -> x20 -> Resample(TARGET, LINEAR) -> diag(SCALE_WIDTH, SCALE_HEIGHT) 1x1 conv.
    """
    backend = backend_of(backend)
    N, _, H, W = img0.shape
    ah, aw = adapted_size(H, W)
    neg_default = mean is None
    if mean is None:
        mean = _const(img0.device, (0.411, 0.433, 0.45))   # BGR order of a typical RGB mean
    if (ah, aw) == (H, W) and img0.is_cuda and not torch.is_grad_enabled() and backend.has_scale_shift:
        # At the ADAPTED size the LINEAR Resample is the identity (one tap of weight 1), so the head is x * (1 / 255) - mean per image:
        # one pass per image (product and difference rounded separately: the bits of the Eltwise and mean-subtraction layers), written
        # straight into the blob the towers (C: batch axis) or conv1 (S: channel axis) read -- instead of scale, subtract and concat.
        neg_mean = _const(img0.device, (-0.411, -0.433, -0.45)) if neg_default else (-mean).contiguous()
        if kind == "C":
            x = torch.empty((2 * N, 3, H, W), device=img0.device, dtype=torch.float32)
            backend.scale_shift(img0, 1.0 / 255.0, neg_mean, out=x[:N])
            backend.scale_shift(img1, 1.0 / 255.0, neg_mean, out=x[N:])
            flows = flownet_c_core(P, None, None, backend, towers=x)
        else:
            x = torch.empty((N, 6, H, W), device=img0.device, dtype=torch.float32)
            backend.scale_shift(img0, 1.0 / 255.0, neg_mean, out=x, out_c0=0)
            backend.scale_shift(img1, 1.0 / 255.0, neg_mean, out=x, out_c0=3)
            flows = flownet_s_core(P, x, backend)
    else:
        pre = []
        for im in (img0, img1):
            x = im * (1.0 / 255.0)                                                 # Eltwise, coeff 1/255
            if (ah, aw) != (H, W):
                x = backend.resample(x, ah, aw)                                    # Resample to ADAPTED size
            pre.append(x - mean.view(1, 3, 1, 1))                                  # DataAugmentation mean subtraction (deploy slice)
        if kind == "C":
            flows = flownet_c_core(P, pre[0], pre[1], backend)
        else:
            flows = flownet_s_core(P, torch.cat(pre, 1), backend)
    if img0.is_cuda and not torch.is_grad_enabled() and backend.has_slices:
        flow = backend.resample_slices(flows[2], H, W, in_scale=FLOW_SCALE)         # Eltwise{20} folded into the Resample (same roundings)
        if (ah, aw) == (H, W):
            return flow                                                              # diag(1, 1): x * 1.0f is x
    else:
        flow = flows[2] * FLOW_SCALE                                                # Eltwise, coeff 20
        flow = backend.resample(flow, H, W)                                         # Resample to TARGET size (x4 up-sampling)
    scale = _const(flow.device, (W / float(aw), H / float(ah)))   # run-flownet.py:47-48
    return flow * scale.view(1, 2, 1, 1)                                            # 1x1 conv, diagonal filler


def loss_targets_ahead(gt_flow, backend, divisors=None):
    """The Downsample(GT * 0.05) pyramid of multiscale_loss issued ahead of the forward pass on a second stream (backend.downsample_ahead:
    it depends on the ground truth alone).  Returns an opaque handle for multiscale_loss(..., targets=handle), or None when the backend
    has no such form."""
    backend = backend_of(backend)
    if not (backend.targets_ahead and gt_flow.is_cuda):
        return None
    H, W = gt_flow.shape[2], gt_flow.shape[3]
    divisors = divisors or {s: 2 ** s for s in LOSS_WEIGHTS}
    gt = gt_flow * (1.0 / FLOW_SCALE)
    sizes = [(H // divisors[s], W // divisors[s]) for s in LOSS_WEIGHTS]
    tgts, ev = backend.downsample_ahead(gt, sizes)
    return {"targets": dict(zip(LOSS_WEIGHTS, tgts)), "event": ev, "sizes": dict(zip(LOSS_WEIGHTS, sizes))}


FINAL_FLOW_GT_SCALE = {"SD": 1.0 / SD_FLOW_SCALE, "fusion": 1.0}     # pixels -> the units of the final flow of flownet_sd_core / fusion_core


def _lpq_kwargs(loss):
    """loss = ("lpq", p, q[, p_epsilon[, q_epsilon]]) -> the keyword arguments of the backend's lpq_loss / lpq_loss_multi with the flags the
    L1Loss path uses (normalize_by_num_entries; p_epsilon 0 and q_epsilon 1e-2, the proto's defaults, when left out)."""
    if not (isinstance(loss, (tuple, list)) and 3 <= len(loss) <= 5 and loss[0] == "lpq"):
        raise ValueError('loss: None or ("lpq", p, q[, p_epsilon[, q_epsilon]]), got %r' % (loss,))
    p_eps, q_eps = (tuple(loss[3:]) + (0.0, 1e-2)[len(loss) - 3:])
    return dict(p=float(loss[1]), q=float(loss[2]), p_epsilon=float(p_eps), q_epsilon=float(q_eps), normalize_by_num_entries=True)


def final_flow_loss(flow, gt_flow, backend, scale, loss=None):
    """Training loss of a core that returns only its final flow (flownet_sd_core, fusion_core): Downsample(GT * scale) to that flow's size
    -> L1Loss{l2_per_location, normalize_by_num_entries}, the loss layer multiscale_loss uses per scale; loss=("lpq", p, q, p_epsilon,
    q_epsilon): LpqLoss{normalize_by_num_entries} in its place."""
    backend = backend_of(backend)
    tgt = backend.downsample(gt_flow * scale, flow.shape[2], flow.shape[3])
    if loss is not None:
        return backend.lpq_loss(flow, tgt, **_lpq_kwargs(loss))
    return backend.l1_loss(flow, tgt, l2_per_location=True, normalize_by_num_entries=True)


def multiscale_loss(flows, gt_flow, backend, targets=None, loss=None):
    """Training loss: per scale Downsample(GT * 0.05) -> L1Loss{l2_per_location, normalize_by_num_entries}.  `targets`: the handle of
    loss_targets_ahead (the same Downsample launches, issued at the start of the step on a second stream).  loss=("lpq", p, q, p_epsilon,
    q_epsilon): LpqLoss{normalize_by_num_entries} per scale instead (p = 2, q = 0.5 is the L1Loss form), in one launch where the backend
    has lpq_loss_multi."""
    backend = backend_of(backend)
    lpq = _lpq_kwargs(loss) if loss is not None else None
    if (backend.has_multi_loss if lpq is None else backend.has_multi_lpq_loss) and gt_flow.is_cuda:
        # the five loss layers in one launch per direction, the weighted sum (Net::ForwardFromTo's loss += ...) included
        scales = list(LOSS_WEIGHTS.items())
        preds = [flows[s] for s, _ in scales]
        if targets is not None and all(tuple(targets["sizes"][s]) == tuple(flows[s].shape[2:]) for s, _ in scales):
            backend.wait_ahead(targets["event"])
            tgts = [targets["targets"][s] for s, _ in scales]
        else:
            gt = gt_flow * (1.0 / FLOW_SCALE)
            tgts = [backend.downsample(gt, p.shape[2], p.shape[3]) for p in preds]
        if lpq is not None:
            return backend.lpq_loss_multi(preds, tgts, [w for _, w in scales], **lpq)[0]
        return backend.l1_loss_multi(preds, tgts, [w for _, w in scales], l2_per_location=True, normalize_by_num_entries=True)[0]
    gt = gt_flow * (1.0 / FLOW_SCALE)
    total = 0.0
    for s, w in LOSS_WEIGHTS.items():
        pred = flows[s]
        tgt = backend.downsample(gt, pred.shape[2], pred.shape[3])
        if lpq is not None:
            total = total + w * backend.lpq_loss(pred, tgt, **lpq)
        else:
            total = total + w * backend.l1_loss(pred, tgt, l2_per_location=True, normalize_by_num_entries=True)
    return total


def unsupervised_loss(flows_fw, flows_bw, img0, img1, backend, occ="consistency", **kw):
    """Training loss without ground truth: per scale s of LOSS_WEIGHTS that flows_fw holds, LOSS_WEIGHTS[s] times the backend's
    unsupervised_loss (photometric + smoothness, both directions) of flows_fw[s] and flows_bw[s] on the images brought to that scale with
    Downsample; the weighted sum in list order.  The predictions are in FlowNet's 1/20 units of full-resolution pixels, so flow_mult =
    FLOW_SCALE * w_s / W makes them pixels of the scale.  occ="consistency": the occlusion planes of the data term come from the
    backend's flow_consistency on the detached, rescaled flows of the scale; "range": from its flow_range_occlusion (the range maps of
    csrc/flow_splat.hip: a pixel nothing of the other frame maps to); None: no pixel is masked.  kw: the keyword arguments of
    functional.unsupervised_loss (weights, Charbonnier constants, edge_weight, smooth_order, data_term and census: data_term="census"
    takes the census data term of csrc/census_loss.hip at every scale)."""
    backend = backend_of(backend)
    if not backend.has_unsupervised_loss:
        raise RuntimeError("unsupervised_loss: the backend has no unsupervised_loss op (there is no composed fallback)")
    if kw.get("data_term", "brightness") == "census" and not backend.has_census_loss:
        raise RuntimeError("unsupervised_loss: the backend has no census_loss op (there is no composed fallback)")
    if occ not in ("consistency", "range", None):
        raise ValueError('unsupervised_loss: occ must be "consistency", "range" or None, got %r' % (occ,))
    if occ == "range" and not backend.has_flow_splat:
        raise RuntimeError("unsupervised_loss: the backend has no flow_range_occlusion op (there is no composed fallback)")
    if "flow_mult" in kw:
        raise ValueError("unsupervised_loss: flow_mult is set per scale (FLOW_SCALE * w_s / W)")
    W = img0.shape[3]
    total = None
    for s, weight in LOSS_WEIGHTS.items():
        if s not in flows_fw:
            continue
        fw, bw = flows_fw[s], flows_bw[s]
        h, w = fw.shape[2], fw.shape[3]
        mult = FLOW_SCALE * w / W
        i0, i1 = backend.downsample(img0, h, w), backend.downsample(img1, h, w)
        occ_fw = occ_bw = None
        if occ == "range":
            occ_fw, occ_bw = backend.flow_range_occlusion(fw.detach() * mult, bw.detach() * mult)[:2]
        elif occ is not None:
            c = backend.flow_consistency(fw.detach() * mult, bw.detach() * mult)
            occ_fw, occ_bw = c.occ_fw, c.occ_bw
        term = backend.unsupervised_loss(i0, i1, fw, bw, occ_fw, occ_bw, flow_mult=mult, **kw) * weight
        total = term if total is None else total + term
    if total is None:
        raise ValueError("unsupervised_loss: flows_fw holds no scale of LOSS_WEIGHTS")
    return total


# FLOP model (multiply-add = 2 flops) used by bench.py
def conv_flops(kind: str, h: int, w: int, in_channels: int = 6) -> float:
    fl = 0.0
    size = {}
    hh, ww = h, w
    res = {"conv1": 2, "conv2": 4, "conv3": 8, "conv_redir": 8, "conv3_1": 8, "conv4": 16, "conv4_1": 16, "conv5": 32, "conv5_1": 32,
           "conv6": 64, "conv6_1": 64, "Convolution1": 64, "deconv5": 32, "upsample_flow6to5": 32, "Convolution2": 32,
           "deconv4": 16, "upsample_flow5to4": 16, "Convolution3": 16, "deconv3": 8, "upsample_flow4to3": 8, "Convolution4": 8,
           "deconv2": 4, "upsample_flow3to2": 4, "Convolution5": 4}
    for (name, k, ci, co, ks, s, p) in layer_table(kind, in_channels):
        oh, ow = hh // res[name], ww // res[name]
        macs = oh * ow * co * ci * ks * ks if k == "conv" else (oh // 2) * (ow // 2) * ci * co * ks * ks
        mult = 2 if (kind == "C" and name in ("conv1", "conv2", "conv3")) else 1
        fl += 2.0 * macs * mult
    return fl


# ------------------------------------------------------------------------------------------------------------------
# Full FlowNet2 (BASELINE.json configs[2]): FlowNetC -> FlowNetS -> FlowNetS ("CSS") || FlowNet-SD -> fusion net.
# Topology from SURVEY.md Appendix B (memory of the paper / third-party converters -- the prototxts are not in the
# reference tree).  Weight names carry the prefixes of the released caffemodels: net2_, net3_, netsd_, fuse_.
# ------------------------------------------------------------------------------------------------------------------
_SD_TABLE = [("conv0", "conv", 6, 64, 3, 1, 1), ("conv1", "conv", 64, 64, 3, 2, 1), ("conv1_1", "conv", 64, 128, 3, 1, 1),
             ("conv2", "conv", 128, 128, 3, 2, 1), ("conv2_1", "conv", 128, 128, 3, 1, 1), ("conv3", "conv", 128, 256, 3, 2, 1),
             ("conv3_1", "conv", 256, 256, 3, 1, 1), ("conv4", "conv", 256, 512, 3, 2, 1), ("conv4_1", "conv", 512, 512, 3, 1, 1),
             ("conv5", "conv", 512, 512, 3, 2, 1), ("conv5_1", "conv", 512, 512, 3, 1, 1), ("conv6", "conv", 512, 1024, 3, 2, 1),
             ("conv6_1", "conv", 1024, 1024, 3, 1, 1),
             ("Convolution1", "conv", 1024, 2, 3, 1, 1), ("deconv5", "deconv", 1024, 512, 4, 2, 1), ("upsample_flow6to5", "deconv", 2, 2, 4, 2, 1),
             ("interconv5", "conv", 1026, 512, 3, 1, 1), ("Convolution2", "conv", 512, 2, 3, 1, 1),
             ("deconv4", "deconv", 1026, 256, 4, 2, 1), ("upsample_flow5to4", "deconv", 2, 2, 4, 2, 1),
             ("interconv4", "conv", 770, 256, 3, 1, 1), ("Convolution3", "conv", 256, 2, 3, 1, 1),
             ("deconv3", "deconv", 770, 128, 4, 2, 1), ("upsample_flow4to3", "deconv", 2, 2, 4, 2, 1),
             ("interconv3", "conv", 386, 128, 3, 1, 1), ("Convolution4", "conv", 128, 2, 3, 1, 1),
             ("deconv2", "deconv", 386, 64, 4, 2, 1), ("upsample_flow3to2", "deconv", 2, 2, 4, 2, 1),
             ("interconv2", "conv", 194, 64, 3, 1, 1), ("Convolution5", "conv", 64, 2, 3, 1, 1)]
_FUSE_TABLE = [("conv0", "conv", 11, 64, 3, 1, 1), ("conv1", "conv", 64, 64, 3, 2, 1), ("conv1_1", "conv", 64, 128, 3, 1, 1),
               ("conv2", "conv", 128, 128, 3, 2, 1), ("conv2_1", "conv", 128, 128, 3, 1, 1),
               ("Convolution5", "conv", 128, 2, 3, 1, 1), ("deconv1", "deconv", 128, 32, 4, 2, 1), ("upsample_flow2to1", "deconv", 2, 2, 4, 2, 1),
               ("interconv1", "conv", 162, 32, 3, 1, 1), ("Convolution6", "conv", 32, 2, 3, 1, 1),
               ("deconv0", "deconv", 162, 16, 4, 2, 1), ("upsample_flow1to0", "deconv", 2, 2, 4, 2, 1),
               ("interconv0", "conv", 82, 16, 3, 1, 1), ("Convolution7", "conv", 16, 2, 3, 1, 1)]


_SD_RES = {"conv0": 1, "conv1": 2, "conv1_1": 2, "conv2": 4, "conv2_1": 4, "conv3": 8, "conv3_1": 8, "conv4": 16, "conv4_1": 16, "conv5": 32,
           "conv5_1": 32, "conv6": 64, "conv6_1": 64, "Convolution1": 64, "deconv5": 32, "upsample_flow6to5": 32, "interconv5": 32,
           "Convolution2": 32, "deconv4": 16, "upsample_flow5to4": 16, "interconv4": 16, "Convolution3": 16, "deconv3": 8,
           "upsample_flow4to3": 8, "interconv3": 8, "Convolution4": 8, "deconv2": 4, "upsample_flow3to2": 4, "interconv2": 4, "Convolution5": 4}
_FUSE_RES = {"conv0": 1, "conv1": 2, "conv1_1": 2, "conv2": 4, "conv2_1": 4, "Convolution5": 4, "deconv1": 2, "upsample_flow2to1": 2,
             "interconv1": 2, "Convolution6": 2, "deconv0": 1, "upsample_flow1to0": 1, "interconv0": 1, "Convolution7": 1}


def _table_flops(table, res, h, w):
    fl = 0.0
    for (name, k, ci, co, ks, s, p) in table:
        oh, ow = h // res[name], w // res[name]          # output size of the layer (a deconv's input is half of it)
        fl += 2.0 * (oh * ow * co * ci * ks * ks if k == "conv" else (oh // 2) * (ow // 2) * ci * co * ks * ks)
    return fl


def flownet2_conv_flops(h: int, w: int) -> float:
    """Multiply-add flops of the conv / deconv layers of one full FlowNet2 forward (C + S + S + SD + fusion) per image pair."""
    return conv_flops("C", h, w) + 2 * conv_flops("S", h, w, 12) + _table_flops(_SD_TABLE, _SD_RES, h, w) + _table_flops(_FUSE_TABLE, _FUSE_RES, h, w)


def _init_table(table, prefix, g, params, device):
    for (name, k, ci, co, ks, s, p) in table:
        shape = (co, ci, ks, ks) if k == "conv" else (ci, co, ks, ks)
        fan_in = ci * ks * ks if k == "conv" else ci * ks * ks / (s * s)
        std = math.sqrt(2.0 / ((1 + NEG_SLOPE ** 2) * fan_in))
        if name.startswith("Convolution"):
            std *= 0.5
        if name.startswith("upsample_flow"):
            std = 0.25
        params[prefix + name + ".w"] = (torch.randn(shape, generator=g) * std).to(device)
        params[prefix + name + ".b"] = torch.zeros(co).to(device)


def init_params_flownet2(seed: int = 0, device="cpu") -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    P: Dict[str, torch.Tensor] = {}
    _init_table(layer_table("C"), "", g, P, device)
    _init_table(layer_table("S", 12), "net2_", g, P, device)
    _init_table(layer_table("S", 12), "net3_", g, P, device)
    _init_table(_SD_TABLE, "netsd_", g, P, device)
    _init_table(_FUSE_TABLE, "fuse_", g, P, device)
    return P


class _Prefixed(dict):
    """View of a parameter dict under a layer-name prefix."""

    def __init__(self, P, prefix):
        super().__init__()
        self.P, self.prefix = P, prefix

    def __getitem__(self, k):
        return self.P[self.prefix + k]


def flownet_sd_core(P, x, backend):
    be = backend_of(backend)
    c0 = be.conv(x, P, "conv0", 1, 1)
    c1 = be.conv(be.conv(c0, P, "conv1", 2, 1), P, "conv1_1", 1, 1)
    # the skip tensors of the two finest decoder levels are written straight into their Concat blobs (66 / 66 % of those copies)
    blob2, c2 = _conv_into_concat(be.conv(c1, P, "conv2", 2, 1), P, "conv2_1", 1, 1, 64 + 2, be)
    blob3, c3 = _conv_into_concat(be.conv(c2, P, "conv3", 2, 1), P, "conv3_1", 1, 1, 128 + 2, be)
    blob4, c4 = _skip_conv(be.conv(c3, P, "conv4", 2, 1), P, "conv4_1", 1, 1, "deconv4", be)
    blob5, c5 = _skip_conv(be.conv(c4, P, "conv5", 2, 1), P, "conv5_1", 1, 1, "deconv5", be)
    c6 = be.conv(be.conv(c5, P, "conv6", 2, 1), P, "conv6_1", 1, 1)
    flow6 = be.predict_flow(c6, P, "Convolution1")
    cat5 = _refine_stage(P, (blob5, c5), c6, "deconv5", flow6, "upsample_flow6to5", be)
    flow5 = be.predict_flow(be.conv(cat5, P, "interconv5", 1, 1, act=False), P, "Convolution2")
    cat4 = _refine_stage(P, (blob4, c4), cat5, "deconv4", flow5, "upsample_flow5to4", be)
    flow4 = be.predict_flow(be.conv(cat4, P, "interconv4", 1, 1, act=False), P, "Convolution3")
    cat3 = _refine_stage(P, (blob3, c3), cat4, "deconv3", flow4, "upsample_flow4to3", be)
    flow3 = be.predict_flow(be.conv(cat3, P, "interconv3", 1, 1, act=False), P, "Convolution4")
    cat2 = _refine_stage(P, (blob2, c2), cat3, "deconv2", flow3, "upsample_flow3to2", be)
    return be.predict_flow(be.conv(cat2, P, "interconv2", 1, 1, act=False), P, "Convolution5")      # 1/4 resolution, units of 1/SD_FLOW_SCALE px


def fusion_core(P, x, backend):
    be = backend_of(backend)
    # conv0 / conv1_1 write their 64 / 128 channels straight into the 82- / 162-channel Concat blobs of the decoder (387 MB and 191 MB
    # at 768x384 batch 4: the two largest copies of a FlowNet2 forward)
    blob0, c0 = _conv_into_concat(x, P, "conv0", 1, 1, 16 + 2, be)
    blob1, c1 = _conv_into_concat(be.conv(c0, P, "conv1", 2, 1), P, "conv1_1", 1, 1, 32 + 2, be)
    c2 = be.conv(be.conv(c1, P, "conv2", 2, 1), P, "conv2_1", 1, 1)
    flow2 = be.predict_flow(c2, P, "Convolution5")
    cat1 = _refine_stage(P, (blob1, c1), c2, "deconv1", flow2, "upsample_flow2to1", be)
    flow1 = be.predict_flow(be.conv(cat1, P, "interconv1", 1, 1, act=False), P, "Convolution6")
    cat0 = _refine_stage(P, (blob0, c0), cat1, "deconv0", flow1, "upsample_flow1to0", be)
    return be.predict_flow(be.conv(cat0, P, "interconv0", 1, 1, act=False), P, "Convolution7")        # full resolution, pixels


def flownet2_deploy_forward(P, img0, img1, backend, mean: Optional[torch.Tensor] = None):
    """Full FlowNet2: raw 0..255 BGR pairs [N,3,H,W] -> flow [N,2,H,W] in pixels.  Four FlowWarp + four ChannelNorm
    + six Resample calls per forward."""
    backend = backend_of(backend)
    N, _, H, W = img0.shape
    ah, aw = adapted_size(H, W)
    neg_mean = _const(img0.device, (-0.411, -0.433, -0.45)) if mean is None else (-mean).contiguous()
    if mean is None:
        mean = _const(img0.device, (0.411, 0.433, 0.45))
    if img0.is_cuda and not torch.is_grad_enabled() and backend.has_slices:
        return _flownet2_pick_streams(P, img0, img1, backend, neg_mean)
    if (ah, aw) == (H, W) and img0.is_cuda and not torch.is_grad_enabled() and backend.has_scale_shift:
        # LINEAR Resample at equal size is the identity: scale and mean in one pass per image (two roundings, like the two layers)
        a = backend.scale_shift(img0, 1.0 / 255.0, neg_mean)
        b = backend.scale_shift(img1, 1.0 / 255.0, neg_mean)
    else:
        a = backend.resample(img0 * (1.0 / 255.0), ah, aw) - mean.view(1, 3, 1, 1)
        b = backend.resample(img1 * (1.0 / 255.0), ah, aw) - mean.view(1, 3, 1, 1)

    def refine_input(flow_q):                       # flow_q: 1/4 resolution, units px/20
        flow = backend.resample(flow_q * FLOW_SCALE, ah, aw)                       # x20, Resample x4 (LINEAR)
        warped = backend.flow_warp(b, flow)                                          # FlowWarp(img1, flow)
        err = backend.channel_norm(a - warped)                                       # ChannelNorm(img0 - warped)
        return flow, warped, err

    flow1_q = flownet_c_core(P, a, b, backend)[2]
    f1, w1, e1 = refine_input(flow1_q)
    flow2_q = flownet_s_core(_Prefixed(P, "net2_"), torch.cat([a, b, w1, f1 * (1.0 / FLOW_SCALE), e1], 1), backend)[2]
    f2, w2, e2 = refine_input(flow2_q)
    flow3_q = flownet_s_core(_Prefixed(P, "net3_"), torch.cat([a, b, w2, f2 * (1.0 / FLOW_SCALE), e2], 1), backend)[2]
    flow_css = backend.resample(flow3_q * FLOW_SCALE, ah, aw, type=1)               # NEAREST into the fusion net (Appendix B)
    flow_sd = backend.resample(flownet_sd_core(_Prefixed(P, "netsd_"), torch.cat([a, b], 1), backend) * SD_FLOW_SCALE, ah, aw, type=1)
    err_css = backend.channel_norm(a - backend.flow_warp(b, flow_css))
    err_sd = backend.channel_norm(a - backend.flow_warp(b, flow_sd))
    fuse_in = torch.cat([a, flow_sd, flow_css, backend.channel_norm(flow_sd), backend.channel_norm(flow_css), err_sd, err_css], 1)
    flow = fusion_core(_Prefixed(P, "fuse_"), fuse_in, backend)
    flow = backend.resample(flow, H, W)
    scale = _const(flow.device, (W / float(aw), H / float(ah)))
    return flow * scale.view(1, 2, 1, 1)


_SD_STREAM = {"mode": "auto", "streams": {}, "picked": {}}


def set_sd_side_stream(mode="auto"):
    """FlowNet-SD only reads the two images: it is independent of the FlowNetC -> S -> S stack until the fusion net.  "on" / True
    runs it on a second HIP stream beside that stack, "off" / False behind it; "auto" (default) times both layouts on the first calls of a
    geometry -- like the kernels time their tile variants -- and keeps the faster (on most boxes the second stream; two boxes of the pool ran
    batch 1 SLOWER with it: 5.65-5.72 against 5.35 ms, while batch 4 gained there too).  Two LONG independent chains share the chip well -- the coarse
    layers of either net leave CUs idle, most of all at batch 1: 5.38 -> 5.00 ms at batch 1 @1024x448, 10.31 -> 10.01 ms at batch 4 @768x384,
    15.20 -> 14.75 ms at batch 4 @1024x448 (round 5) -- where a handful of small kernels beside a chip-filling GEMM did not (the flow heads on a
    second stream, round 4).  Same kernels, same bits."""
    _SD_STREAM["mode"] = {True: "on", False: "off"}.get(mode, mode)
    _SD_STREAM["picked"] = {}


def _flownet2_pick_streams(P, img0, img1, backend, neg_mean):
    """set_sd_side_stream: "on" / "off" as told; "auto": call 0 of a geometry runs with the second stream (lazy initialisation, the kernels'
    own variant timing), calls 1 .. 4 alternate the two layouts between device synchronisations and are timed, then the faster one stays
    (the second stream unless it loses by more than 1 %).  Under graph capture nothing is timed (the second stream, or what was picked)."""
    import time
    mode = _SD_STREAM["mode"]
    run = lambda side: _flownet2_deploy_forward_slices(P, img0, img1, backend, neg_mean, side)
    if mode != "auto":
        return run(mode == "on")
    key = (img0.device, tuple(img0.shape))
    st = _SD_STREAM["picked"].get(key)
    if isinstance(st, bool):
        return run(st)
    if torch.cuda.is_current_stream_capturing():
        return run(True)
    if st is None:
        st = _SD_STREAM["picked"][key] = {"n": 0, True: [], False: []}
    n = st["n"]
    st["n"] += 1
    if n == 0:
        return run(True)
    side = n % 2 == 1
    torch.cuda.synchronize(img0.device)
    t0 = time.perf_counter()
    out = run(side)
    torch.cuda.synchronize(img0.device)
    st[side].append(time.perf_counter() - t0)
    if n >= 4:
        _SD_STREAM["picked"][key] = min(st[True]) <= 1.01 * min(st[False])
        _SD_STREAM.setdefault("timings_ms", {})[key] = {"second_stream": round(min(st[True]) * 1e3, 4), "one_stream": round(min(st[False]) * 1e3, 4)}
    return out


def sd_side_stream_timings():
    """{(device, image shape): {"second_stream": ms, "one_stream": ms}}: what "auto" measured (host clock around one synchronised forward,
    best of two per layout) when it decided -- bench.py prints it so that a box where the second stream loses leaves a record."""
    return dict(_SD_STREAM.get("timings_ms", {}))


def sd_side_stream_picks():
    """{(device, image shape): True / False} of the geometries "auto" has decided (bench.py reports it)."""
    return {k: v for k, v in _SD_STREAM["picked"].items() if isinstance(v, bool)}


def _sd_side_stream(dev, on):
    if not on:
        return None
    st = _SD_STREAM["streams"].get(dev)
    if st is None:
        st = _SD_STREAM["streams"][dev] = torch.cuda.Stream(device=dev)
    return st


def _flownet2_deploy_forward_slices(P, img0, img1, backend, neg_mean, sd_beside=True):
    """The same graph on the GPU backend without its glue passes: the Concat blobs are allocated once and every producer writes its
    channel slice (fn2_*_slices), the Eltwise scalings (x20 in front of a Resample, x0.05 behind it, img0 - warped in front of a
    ChannelNorm) ride in the kernels of their neighbours with the same roundings.  Per forward this removes 7 Concat copies and 19
    element-wise passes over full-resolution blobs; results equal the layer-by-layer graph bit for bit
    (tests/test_gpu_parity.py::test_flownet2_slice_path_is_bitwise_the_layer_graph)."""
    N, _, H, W = img0.shape
    ah, aw = adapted_size(H, W)
    dev = img0.device
    new = lambda c: torch.empty((N, c, ah, aw), device=dev, dtype=torch.float32)
    towers = torch.empty((2 * N, 3, ah, aw), device=dev, dtype=torch.float32)     # FlowNetC's siamese batch [img0 ; img1]
    blob = new(12)            # Concat of net2 / net3: [img0 | img1 | warped img1 | flow / 20 | brightness error]
    pair = new(6)             # Concat of FlowNet-SD: [img0 | img1]
    fuse = new(11)            # Concat of the fusion net: [img0 | flow_sd | flow_css | |flow_sd| | |flow_css| | err_sd | err_css]
    for k, img in enumerate((img0, img1)):
        if (ah, aw) == (H, W):   # LINEAR Resample at equal size is the identity: Eltwise{1/255} and the mean subtraction in one pass
            src, s = img, 1.0 / 255.0
        else:                    # Eltwise{1/255} folded into the Resample, then the mean subtraction
            src, s = backend.resample_slices(img, ah, aw, in_scale=1.0 / 255.0), 1.0
        backend.scale_shift(src, s, neg_mean, out=towers[k * N:(k + 1) * N])
        backend.scale_shift(src, s, neg_mean, out=blob, out_c0=3 * k)
        backend.scale_shift(src, s, neg_mean, out=pair, out_c0=3 * k)
        if k == 0:
            backend.scale_shift(src, s, neg_mean, out=fuse, out_c0=0)
    A, B, WARPED = (blob, 0, 3), (blob, 3, 3), (blob, 6, 3)

    def refine_input(flow_q):                       # flow_q: 1/4 resolution, units px/20 -> channels 6..11 of `blob`
        flow = backend.resample_slices(flow_q, ah, aw, in_scale=FLOW_SCALE, out2=(blob, 9, 2), out2_scale=1.0 / FLOW_SCALE)
        backend.flow_warp_slices(B, flow, out=WARPED)
        backend.channel_norm_slices(A, minus=WARPED, out=(blob, 11, 1))

    side = _sd_side_stream(dev, sd_beside)
    sd_q = None
    if side is not None:                            # FlowNet-SD beside the CSS stack (set_sd_side_stream)
        main = torch.cuda.current_stream(dev)
        side.wait_stream(main)                      # `pair` is written
        with torch.cuda.stream(side):
            sd_q = flownet_sd_core(_Prefixed(P, "netsd_"), pair, backend)
    flow1_q = flownet_c_core(P, None, None, backend, towers=towers)[2]
    refine_input(flow1_q)
    flow2_q = flownet_s_core(_Prefixed(P, "net2_"), blob, backend)[2]
    refine_input(flow2_q)                           # net2's conv1 has read the blob (stream order): channels 6..11 are rewritten in place
    flow3_q = flownet_s_core(_Prefixed(P, "net3_"), blob, backend)[2]
    if side is not None:
        main.wait_stream(side)
        sd_q.record_stream(main)                    # allocated under the side stream, read (and freed) under this one
    else:
        sd_q = flownet_sd_core(_Prefixed(P, "netsd_"), pair, backend)
    backend.resample_slices(sd_q, ah, aw, type=1, in_scale=SD_FLOW_SCALE, out=(fuse, 3, 2))        # NEAREST into the fusion net (Appendix B)
    backend.resample_slices(flow3_q, ah, aw, type=1, in_scale=FLOW_SCALE, out=(fuse, 5, 2))
    backend.channel_norm_slices((fuse, 3, 2), out=(fuse, 7, 1))
    backend.channel_norm_slices((fuse, 5, 2), out=(fuse, 8, 1))
    backend.flow_warp_slices(B, (fuse, 3, 2), out=WARPED)
    backend.channel_norm_slices(A, minus=WARPED, out=(fuse, 9, 1))
    backend.flow_warp_slices(B, (fuse, 5, 2), out=WARPED)
    backend.channel_norm_slices(A, minus=WARPED, out=(fuse, 10, 1))
    flow = fusion_core(_Prefixed(P, "fuse_"), fuse, backend)
    if (ah, aw) == (H, W):
        return flow               # Resample to an equal size and the Eltwise{1, 1} behind it are identities
    flow = backend.resample(flow, H, W)
    scale = _const(flow.device, (W / float(aw), H / float(ah)))
    return flow * scale.view(1, 2, 1, 1)
