"""The one interface the graphs of nets.py are written against, and the one seam for "every layer that ran".

GraphBackend wraps whatever a caller hands over as `backend` -- the module flownet2_amd.functional (HIP kernels), oracle.backend (the C
oracle on the host), a namespace with three ops (the fp64 comparator), a test stub, or None -- and probes it ONCE, in its constructor.  The
graphs then call total layer ops and read a few named booleans; they never ask what the object can do:
  * conv / deconv (conv_wb / deconv_wb on explicit tensors), predict_flow, upsample_flow, leaky_relu: the stock forms.  A convolution
    runs on the own kernel, else on the counted library convolution + conv_bias_leaky_relu, else on plain torch;
  * own_conv / own_deconv / own_correlation_relu_into: the backend's own kernels as they are (functional.conv_mfma_relu, deconv_relu,
    correlation_relu_into), which also write into a channel slice of a Concat blob (out=..., out_c0=...) -- called by the graph without
    a frame in between, followed by wrote(...) for the listeners.
"The backend has no such form, or declined this layer" is one answer, None, as functional.conv_mfma_relu gives it; the graph then
copies or concatenates from the stock form.

listening(fn) registers fn(name, y, info) for the duration of a with block: the adapter calls it after every convolution, deconvolution and
stand-alone ReLU that ran, in execution order, with the bare layer name, the layer's output (for an in-place form the slice that carries
the autograd graph, else the layer's channel slice of the blob) and info = {"kind": "conv" | "deconv" | "relu", "act", "x", "w", "stride",
"pad", "own", "into", "backend"}.  oracle/fp64_graph.record_relu_branches, the FN2_TRACE_CONV print and scripts/step_breakdown.py are
such listeners."""
from __future__ import annotations

import contextlib
import types

import torch.nn.functional as F

NEG_SLOPE = 0.1          # ReLU negative_slope of every FlowNet conv/deconv

_LISTENERS = []          # fn(name, y, info); one truthiness test per layer when nobody listens


@contextlib.contextmanager
def listening(fn):
    _LISTENERS.append(fn)
    try:
        yield fn
    finally:
        _LISTENERS.remove(fn)


def _declines(*args, **kwargs):
    return None


class GraphBackend:
    # the custom-layer ops (and their *_slices / one-launch forms) the graphs call by name: bound when the object has them; one it lacks
    # fails when it is called, with the object's own AttributeError that names it.  Nothing else of the object is reachable through the adapter.
    FORWARDED = ("correlation", "resample", "flow_warp", "channel_norm", "downsample", "l1_loss", "scale_shift", "resample_slices",
                 "flow_warp_slices", "channel_norm_slices", "l1_loss_multi", "downsample_ahead", "wait_ahead", "lpq_loss", "lpq_loss_multi",
                 "unsupervised_loss", "flow_consistency", "census_loss", "flow_splat", "flow_range_occlusion")

    def __init__(self, obj):
        get = lambda name: getattr(obj, name, None)
        self.obj = obj
        for name in self.FORWARDED:
            if get(name) is not None:
                setattr(self, name, get(name))
        self.own_conv, self.own_deconv = get("conv_mfma_relu") or _declines, get("deconv_relu") or _declines
        self.own_correlation_relu_into = get("correlation_relu_into") or _declines
        self._predict, self._upsample = get("predict_flow_conv"), get("upsample_flow_deconv")
        self._predict_upsample = get("predict_upsample_flow")
        self._bias_act = get("conv_bias_leaky_relu")
        self._conv2d = get("lib_conv2d") or (lambda x, w, b, s, p: F.conv2d(x, w, b, stride=s, padding=p))
        self._deconv2d = get("lib_conv_transpose2d") or (lambda x, w, b, s, p: F.conv_transpose2d(x, w, b, stride=s, padding=p))
        self._act = get("leaky_relu") or (lambda y, slope, name: F.leaky_relu(y, slope))     # (y, slope, layer name)
        self.conv_route_name, self.relu_chain_supported = get("conv_route_name"), get("relu_chain_supported")
        # graph-level choices
        self.writes_slices = self.own_conv is not _declines             # Concat blobs written in place by their producers
        self.fuses_correlation = self.own_correlation_relu_into is not _declines
        self.has_slices = get("resample_slices") is not None            # the *_slices forms: nets._flownet2_deploy_forward_slices
        self.has_scale_shift = get("scale_shift") is not None           # the deploy head in one pass per image
        self.trains_in_place = get("conv_backward") is not None         # the in-place Concat producers carry an autograd graph
        # conv1 -> conv2 share one ReLU derivative pass (nets._stem_chain); conv2 then has to be an in-place producer of a training graph
        self.has_stem_chain = self.trains_in_place and self.conv_route_name is not None and self.relu_chain_supported is not None
        self.has_multi_loss = get("l1_loss_multi") is not None          # the five loss layers in one launch
        self.has_multi_lpq_loss = get("lpq_loss_multi") is not None     # the same for loss=("lpq", ...)
        self.has_unsupervised_loss = get("unsupervised_loss") is not None      # the fused photometric + smoothness loss (nets.unsupervised_loss)
        self.has_census_loss = get("census_loss") is not None           # its census data term (data_term="census")
        self.has_flow_splat = get("flow_splat") is not None and get("flow_range_occlusion") is not None      # forward warping; occ="range"
        self.targets_ahead = get("downsample_ahead") is not None        # the loss's target pyramid on a second stream

    def __getattr__(self, name):
        if name in self.FORWARDED:
            return getattr(self.obj, name)              # (the object lacks it: its AttributeError names the op)
        raise AttributeError(name)

    def _ran(self, name, y, **info):
        for fn in list(_LISTENERS):
            fn(name, y, dict(info, backend=self))

    def wrote(self, kind, name, y, out, out_c0, channels, x, w=None, stride=1, pad=0):
        """An own kernel wrote layer `name` into channels [out_c0, out_c0 + channels) of `out` and returned y: tell the listeners."""
        if _LISTENERS:
            self._ran(name, y if y.requires_grad else out[:, out_c0:out_c0 + channels], kind=kind, act=True, x=x, w=w, stride=stride, pad=pad,
                      own=True, into=True)

    def conv_wb(self, x, w, b, stride, pad, act=True, slope=NEG_SLOPE, name=None, relu_chain=None):
        """Convolution{w, stride, pad} + bias (+ ReLU{slope} when act)."""
        y = self.own_conv(x, w, b, stride, pad, slope, act, relu_chain=relu_chain)
        own = y is not None
        if not own:
            if relu_chain is not None:
                raise RuntimeError("relu_chain: no own kernel takes this layer (its consumer was told the stem kernel would)")
            if act and self._bias_act is not None:
                y = self._bias_act(self._conv2d(x, w, None, stride, pad), b, slope)
            else:
                y = self._conv2d(x, w, b, stride, pad)
                if act:
                    y = self._act(y, slope, name)
        if _LISTENERS:
            self._ran(name, y, kind="conv", act=act, x=x, w=w, stride=stride, pad=pad, own=own, into=False)
        return y

    def conv(self, x, P, name, stride, pad, act=True, relu_chain=None):
        return self.conv_wb(x, P[name + ".w"], P[name + ".b"], stride, pad, act, NEG_SLOPE, name, relu_chain)

    def deconv_wb(self, x, w, b, act=True, slope=NEG_SLOPE, name=None):
        """Deconvolution{4, 2, 1} + bias (+ ReLU{slope} when act)."""
        y = self.own_deconv(x, w, b, slope, act)
        own = y is not None
        if not own:
            if act and self._bias_act is not None:
                y = self._bias_act(self._deconv2d(x, w, None, 2, 1), b, slope)
            else:
                y = self._deconv2d(x, w, b, 2, 1)
                if act:
                    y = self._act(y, slope, name)
        if _LISTENERS:
            self._ran(name, y, kind="deconv", act=act, x=x, w=w, stride=2, pad=1, own=own, into=False)
        return y

    def deconv(self, x, P, name, act=True):
        return self.deconv_wb(x, P[name + ".w"], P[name + ".b"], act, NEG_SLOPE, name)

    def predict_flow(self, x, P, name):
        """predict_flow (3x3 conv -> 2 channels): the backend's flow-head kernel (HIP: flow_head.hip), else the stock convolution."""
        if self._predict is not None:
            return self._predict(x, P[name + ".w"], P[name + ".b"])
        return self.conv(x, P, name, 1, 1, act=False)

    def upsample_flow(self, x, P, name, out=None, out_c0=0):
        """upsample_flow (4x4/2 deconv 2 -> 2): the backend's flow-head kernel, optionally into a channel slice of `out` (None without such
        a kernel), else the stock deconvolution."""
        if self._upsample is None:
            return None if out is not None else self.deconv(x, P, name, act=False)
        if out is not None:
            return self._upsample(x, P[name + ".w"], P[name + ".b"], out=out, out_c0=out_c0)
        return self._upsample(x, P[name + ".w"], P[name + ".b"])

    def predict_upsample_flow(self, x, P, pname, uname, out, out_c0):
        """predict_flow `pname` of x, and upsample_flow `uname` of it into channels [out_c0, out_c0 + 2) of `out`: (flow, written).  The
        backend's one-launch form where it has one and takes the layer, else the two ops above; written is False when nothing wrote the
        slice (no flow-head kernel that writes into a blob)."""
        if self._predict_upsample is not None:
            flow = self._predict_upsample(x, P[pname + ".w"], P[pname + ".b"], P[uname + ".w"], P[uname + ".b"], out, out_c0)
            if flow is not None:
                return flow, True
        flow = self.predict_flow(x, P, pname)
        return flow, self.upsample_flow(flow, P, uname, out=out, out_c0=out_c0) is not None

    def leaky_relu(self, x, name, slope=NEG_SLOPE):
        """A ReLU layer of the graph itself (the correlation's)."""
        y = self._act(x, slope, name)
        if _LISTENERS:
            self._ran(name, y, kind="relu", act=True, x=x, own=False, into=False)
        return y


_MODULE_ADAPTERS = {}


def backend_of(obj) -> GraphBackend:
    """The adapter of a backend object; an adapter passes through.  Modules (functional, oracle.backend) and None get theirs once, for the
    life of the process: an attribute of the module that is rebound later is not seen (hand over a namespace of the wrapped ops, or wrap an
    adapter, instead).  Any other object gets a new adapter -- some 25 attribute probes -- on every call: a caller that passes one through
    nets.conv_forward / deconv_forward layer by layer should call backend_of once itself and hand the adapter down."""
    if isinstance(obj, GraphBackend):
        return obj
    if obj is None or isinstance(obj, types.ModuleType):
        be = _MODULE_ADAPTERS.get(obj)
        if be is None:
            be = _MODULE_ADAPTERS[obj] = GraphBackend(obj)
        return be
    return GraphBackend(obj)
