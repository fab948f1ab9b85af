"""Mirrors of the STOCK Caffe layers a FlowNet2 prototxt contains, on the fast paths of this repository: the prototxt executor
(flownet2_amd.net.Net) creates them by `type:` string through the same LayerRegistry as the custom layers (layer_factory.hpp:75-84).

    Convolution    conv_layer.cpp:8-40, base_conv_layer.cpp:15-254 (LayerSetUp / Reshape), conv_layer.cu:8-23
    Deconvolution  deconv_layer.cpp:8-45 (weight blob [Cin, Cout/g, kh, kw], base_conv_layer.cpp:125-139), deconv_layer.cu:8-26
    ReLU           relu_layer.cu:8-27 (negative_slope), in place
    Eltwise        eltwise_layer.cpp:12-65, eltwise_layer.cu:34-66 (SUM with coeff, PROD, MAX; ONE bottom allowed: eltwise_layer.hpp:29)
    Concat / Slice concat_layer.cpp:24-65 / slice_layer.cpp:24-88
    Silence, Input silence_layer.cu, input_layer.cpp

Backward_gpu of every class follows the reference's (conv_layer.cu:26-60, deconv_layer.cu:27-58, relu_layer.cu:33-60, eltwise_layer.cu:68-118,
concat_layer.cu:47-74, slice_layer.cu:49-75, split_layer.cu:18-33, silence_layer.cu:16-27): top diffs in, bottom diffs OVERWRITTEN, parameter
diffs ACCUMULATED -- Net.Backward (net.py) steps a TRAIN prototxt through them; the gradient kernels are the ones nets.py's autograd graph
uses (functional.conv_backward and the flow-head kernels).  Convolution / Deconvolution call the SAME routing functions as nets.py
(nets.conv_forward / deconv_forward and the flow-head kernels), so a prototxt-built net computes the same bits as nets.deploy_forward.
A ReLU that directly follows a Convolution / Deconvolution in place is folded into that layer by the executor (`fused_relu_`): one
kernel, as in nets.py.
"""
from __future__ import annotations

from typing import Sequence

import torch

from . import layers as L
from .layers import Blob, CHECK, CheckError, Layer


def _first(v, default):
    if v is None:
        return default
    if isinstance(v, list):
        return v[0] if v else default
    return v


def fill_blob(blob: Blob, filler: dict, seed_name: str = ""):
    """include/caffe/filler.hpp: constant (:25-43), diagonal (:264-290: blob[n][n][:, :] = diag_val[n] / kernel_area, else 0).  The random
    fillers (msra, xavier, gaussian, uniform) exist to be overwritten by CopyTrainedLayersFrom in a deploy net: they draw from a
    torch generator seeded by the layer name (boost's stream is not reproducible)."""
    t = str(filler.get("type", "constant"))
    shape = blob.shape()
    if t == "constant":
        blob.data = torch.full(shape, float(filler.get("value", 0.0)), dtype=torch.float32, device=blob.device)
    elif t == "diagonal":
        num, ch = shape[0], shape[1] if len(shape) > 1 else 1
        area = 1
        for s in shape[2:]:
            area *= s
        w = torch.zeros(shape, dtype=torch.float32)
        dv = list(filler.get("diag_val", []))
        for n in range(min(num, ch)):
            w[n, n] = (float(dv[n]) if n < len(dv) else 1.0) / float(area)
        blob.data = w.to(blob.device)
    elif t in ("msra", "xavier", "gaussian", "uniform", "positive_unitball", "bilinear"):
        import zlib
        g = torch.Generator().manual_seed(zlib.crc32(seed_name.encode()) & 0x7fffffff)
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        std = float(filler.get("std", 0.0)) if t == "gaussian" else (2.0 / max(1, fan_in)) ** 0.5
        blob.data = (torch.randn(shape, generator=g) * std).to(blob.device)
    else:
        raise CheckError("Unknown filler name: " + t)                                   # filler.hpp:319


def _dims(cp, name, default, spatial=2):
    """The repeated field `name` of a ConvolutionParameter, one value per spatial axis: specified once, or once per spatial dimension
    (base_conv_layer.cpp:35-44, 59-70, 83-93, 98-108); `default` None: at least one entry is required."""
    v = cp.get(name)
    v = [] if v is None else (list(v) if isinstance(v, (list, tuple)) else [v])
    CHECK(len(v) in ((1, spatial) if default is None else (0, 1, spatial)),
          "%s must be specified once, or once per spatial dimension (%s specified %d times; %d spatial dims)." % (name, name, len(v), spatial))
    if not v:
        return (default,) * spatial
    return tuple(int(v[0 if len(v) == 1 else i]) for i in range(spatial))


MAX_SPATIAL_AXES = 3            # what the general kernels state (include/flownet2_hip_conv_volume.h)


class _ConvBase(Layer):
    """BaseConvolutionLayer::LayerSetUp / Reshape (base_conv_layer.cpp:15-254): `axis` and 0 to 3 spatial axes behind it, kernels, pads
    and strides once or once per axis (h / w fields with two axes), dilation and group; every axis in front of `axis` folds into the batch
    (by a view).  force_nd_im2col chooses an im2col routine in the reference and nothing here.  A PLAIN layer (two spatial axes, square
    taps, one stride, one pad, dilation 1, group 1: all a FlowNet uses) runs on the routed kernels of nets.py; every other layer runs
    forward and backward through functional.lib_conv2d / lib_conv_transpose2d (0 and 1 spatial axes as a 2-D layer on a map of height 1)
    or lib_conv3d / lib_conv_transpose3d (3 spatial axes)."""
    transposed = False

    def MinBottomBlobs(self): return 1
    def MinTopBlobs(self): return 1
    def EqualNumBottomTopBlobs(self): return True                                        # base_conv_layer.hpp:29

    def _geom(self, spatial=2):
        """(num_output, kernel, pad, stride, dilation, group, bias_term) as base_conv_layer.cpp:24-124 reads them, the four geometry
        values one per spatial axis."""
        cp = self.layer_param_.convolution_param
        CHECK("num_output" in cp, "num_output is required")

        def hw(name):
            if name + "_h" not in cp and name + "_w" not in cp:
                return False
            CHECK(spatial == 2, "%s_h & %s_w can only be used for 2D convolution." % (name, name))       # base_conv_layer.cpp:28-29, 52-53, 76-77
            return True
        if hw("kernel"):
            CHECK(not cp.get("kernel_size"), "Either kernel_size or kernel_h/w should be specified; not both.")
            kernel = int(cp.get("kernel_h", 0)), int(cp.get("kernel_w", 0))
        else:
            kernel = _dims(cp, "kernel_size", None, spatial)
        CHECK(all(k > 0 for k in kernel), "Filter dimensions must be nonzero.")          # base_conv_layer.cpp:45-47
        if hw("stride"):
            CHECK(not cp.get("stride"), "Either stride or stride_h/w should be specified; not both.")
            stride = int(cp.get("stride_h", 1)), int(cp.get("stride_w", 1))
        else:
            stride = _dims(cp, "stride", 1, spatial)
        CHECK(all(v > 0 for v in stride), "Stride dimensions must be nonzero.")          # base_conv_layer.cpp:69
        if hw("pad"):
            CHECK(not cp.get("pad"), "Either pad or pad_h/w should be specified; not both.")
            pad = int(cp.get("pad_h", 0)), int(cp.get("pad_w", 0))
        else:
            pad = _dims(cp, "pad", 0, spatial)
        dilation = _dims(cp, "dilation", 1, spatial)
        CHECK(all(d >= 1 for d in dilation), "Dilation dimensions must be nonzero.")
        group = int(cp.get("group", 1))
        CHECK(group >= 1, "group must be positive")
        return int(cp["num_output"]), kernel, pad, stride, dilation, group, bool(cp.get("bias_term", True))

    def LayerSetUp(self, bottom, top):
        cp = self.layer_param_.convolution_param
        num_axes, axis = bottom[0].num_axes(), int(cp.get("axis", 1))
        CHECK(-num_axes <= axis < num_axes, "axis %d out of range for %d-D Blob with shape %s" % (axis, num_axes, bottom[0].shape_string()))
        self.channel_axis_ = axis + num_axes if axis < 0 else axis                       # base_conv_layer.cpp:17 (blob.hpp:121-132)
        self.num_spatial_axes_ = spatial = num_axes - self.channel_axis_ - 1
        CHECK(spatial >= 0, "Check failed: num_spatial_axes_ >= 0 (%d vs. 0)" % spatial)   # base_conv_layer.cpp:21
        CHECK(spatial <= MAX_SPATIAL_AXES, "convolution over %d spatial axes is not supported (0 to %d are)" % (spatial, MAX_SPATIAL_AXES))
        self.folded_ = not (self.channel_axis_ == 1 and spatial == 2)                     # the blobs are viewed as [num, C, ...] around the kernels
        (self.num_output_, self.kernel_shape_, self.pad_shape_, self.stride_shape_, self.dilation_shape_, self.group_,
         self.bias_term_) = self._geom(spatial)
        # 0 and 1 spatial axes: the 2-D layer on a map of height 1 (kernel 1, stride 1, pad 0, dilation 1 on the axes that are not there)
        lead = max(0, 2 - spatial)
        self.kernel_hw_, self.stride_hw_, self.dilation_hw_ = ((1,) * lead + v for v in (self.kernel_shape_, self.stride_shape_, self.dilation_shape_))
        self.pad_hw_ = (0,) * lead + self.pad_shape_
        self.plain_ = (spatial == 2 and self.kernel_hw_[0] == self.kernel_hw_[1] and self.pad_hw_[0] == self.pad_hw_[1]
                       and self.stride_hw_[0] == self.stride_hw_[1] and self.dilation_hw_ == (1, 1) and self.group_ == 1)
        # what the plain code paths read; a layer that is not plain never reaches them
        self.kernel_, self.pad_, self.stride_ = (self.kernel_hw_[0], self.pad_hw_[0], self.stride_hw_[0]) if self.plain_ else (None, None, None)
        self.fused_relu_tops_ = {}              # top index -> negative slope of an in-place ReLU folded in by the executor
        cin = bottom[0].shape(self.channel_axis_)
        CHECK(self.num_output_ > 0, "num_output must be positive")                       # base_conv_layer.cpp:120
        CHECK(cin % self.group_ == 0, "Check failed: channels_ % group_ == 0")           # base_conv_layer.cpp:122
        CHECK(self.num_output_ % self.group_ == 0, "Number of output should be multiples of group.")     # base_conv_layer.cpp:123-124
        if not self.blobs_:                                                               # base_conv_layer.cpp:125-152
            wshape = ([cin, self.num_output_ // self.group_] if self.transposed else [self.num_output_, cin // self.group_]) + list(self.kernel_shape_)
            w = Blob(*wshape, device=bottom[0].device)
            fill_blob(w, cp.get("weight_filler", {}), self.layer_param_.name + ".w")
            self.blobs_ = [w]
            if self.bias_term_:
                b = Blob(self.num_output_, device=bottom[0].device)
                fill_blob(b, cp.get("bias_filler", {}), self.layer_param_.name + ".b")
                self.blobs_.append(b)

    def _out_shape(self, size):
        out = []
        for n, k, p, s, d in zip(size, self.kernel_shape_, self.pad_shape_, self.stride_shape_, self.dilation_shape_):
            ext = d * (k - 1) + 1
            out.append(s * (n - 1) + ext - 2 * p if self.transposed else (n + 2 * p - ext) // s + 1)      # deconv_layer.cpp:8-22 / conv_layer.cpp:8-23
        return out

    def _fold(self, t):
        """A bottom or top tensor as the kernels take it: [num, C, spatial...] with num = count(0, channel_axis) (base_conv_layer.cpp:191) and
        at least two spatial axes -- a view of a contiguous blob; the tensor itself for a four-axis blob with axis 1."""
        if not self.folded_:
            return t
        ca = self.channel_axis_
        lead = 1
        for d in t.shape[:ca]:
            lead *= d
        return t.reshape((lead, t.shape[ca]) + (1,) * max(0, 2 - self.num_spatial_axes_) + tuple(t.shape[ca + 1:]))

    def _unfold(self, t, blob):
        return t.reshape(blob.shape()) if self.folded_ else t

    def Reshape(self, bottom, top):
        cin = self.blobs_[0].shape(0) if self.transposed else self.blobs_[0].shape(1) * self.group_
        ca = self.channel_axis_
        CHECK(bottom[0].num_axes() == ca + 1 + self.num_spatial_axes_, "bottom num_axes may not change.")      # base_conv_layer.cpp:189-190
        CHECK(bottom[0].shape(ca) == cin, "Input size incompatible with convolution kernel.")    # base_conv_layer.cpp:191-192
        for b in bottom[1:]:                                                                     # base_conv_layer.cpp:194-197
            CHECK(b.shape() == bottom[0].shape(), "All inputs must have the same shape.")
        shape = bottom[0].shape()
        for t in top:                                                                            # one weight blob, applied to every bottom
            t.Reshape(*(shape[:ca] + [self.num_output_] + self._out_shape(shape[ca + 1:])))       # base_conv_layer.cpp:198-207

    @property
    def fused_relu_(self):
        """Negative slope of the folded ReLU when EVERY top has one with the same slope (the only case the single-top code paths and the
        batched siamese launch ask about), else None."""
        v = set(self.fused_relu_tops_.get(i) for i in range(len(self.layer_param_.top)))
        return next(iter(v)) if len(v) == 1 and None not in v else None

    def _slope(self, i):
        return self.fused_relu_tops_.get(i)

    def _forward_all(self, bottom, top, one):
        """`one(x, slope) -> y` on every (bottom, top) pair (base_conv_layer.cpp: the loop over bottom.size() in Forward_gpu,
        conv_layer.cu:12-22).  Several bottoms with one activation (the siamese towers of FlowNetC: one Convolution, two bottoms, two
        tops) run as ONE launch on the bottoms stacked along the batch axis -- the kernels are per-sample -- and the tops are the
        halves of its output."""
        self._stacked = None
        self._graphs = []                       # of a layer that is not plain (_general_one), one per call of `one`
        if len(bottom) > 1 and len({self._slope(i) for i in range(len(top))}) == 1 and bottom[0].data.is_cuda:
            xs = [self._fold(b.data) for b in bottom]
            n = xs[0].shape[0]
            x = torch.cat(xs, 0)
            y = one(x, self._slope(0))
            for i, t in enumerate(top):
                t.data = self._unfold(y[i * n:(i + 1) * n], t)
            self._stacked = (x, y)              # Backward_gpu runs the stacked batch as ONE launch per gradient, like the forward
            return
        for i, (b, t) in enumerate(zip(bottom, top)):
            t.data = self._unfold(one(self._fold(b.data), self._slope(i)), t)

    def _accumulate(self, k, g):
        """Parameter diffs accumulate (weight_gpu_gemm / backward_gpu_bias with beta = 1); Net.ClearParamDiffs zeroes them per iteration."""
        if g is not None:
            self.blobs_[k].mutable_gpu_diff().add_(g.reshape(self.blobs_[k].shape()))

    def _general_one(self, x, slope, be):
        """A layer that is not plain: lib_conv2d / lib_conv_transpose2d of the backend (the general kernels under
        set_general_convolution("own"), else the counted library), the folded ReLU as a pass of its own.  The autograd graph of the call is
        kept for Backward_gpu, in call order."""
        w, b = self.blobs_[0].data, (self.blobs_[1].data if self.bias_term_ else None)
        nd = "3d" if self.num_spatial_axes_ == 3 else "2d"
        name = ("lib_conv_transpose" if self.transposed else "lib_conv") + nd
        f = getattr(torch.nn.functional, ("conv_transpose" if self.transposed else "conv") + nd)
        stride, pad, dilation = (self.stride_shape_, self.pad_shape_, self.dilation_shape_) if nd == "3d" else (self.stride_hw_, self.pad_hw_, self.dilation_hw_)
        if w.dim() != x.dim():                  # 0 and 1 spatial axes: the weight blob [., ., k...] as the 2-D layer's [., ., 1, k]
            w = w.reshape(tuple(w.shape[:2]) + self.kernel_hw_)
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(True) if t is not None else None for t in (x, w, b)]
            if hasattr(be, name):
                y = getattr(be, name)(leaves[0], leaves[1], leaves[2], stride, pad, dilation=dilation, groups=self.group_)
            else:
                y = f(leaves[0], leaves[1], leaves[2], stride=stride, padding=pad, dilation=dilation, groups=self.group_)
            if slope is not None:
                y = torch.nn.functional.leaky_relu(y, slope)
        self._graphs.append((leaves, y))
        return y.detach()

    def _general_backward(self, index, g, need_x):
        leaves, y = self._graphs[index]
        wanted = [need_x, self.param_propagate_down(0), self.bias_term_ and self.param_propagate_down(1)]
        inputs = [t for t, need in zip(leaves, wanted) if need]
        grads = iter(torch.autograd.grad(y, inputs, g.contiguous(), retain_graph=True) if inputs else ())
        return tuple(next(grads) if need else None for need in wanted)

    def _backward_one(self, x, y, g, slope, need_x, head, index=0):
        from . import functional as Fn, ops
        if not self.plain_:
            return self._general_backward(index, g, need_x)
        w = self.blobs_[0].data
        need_w = self.param_propagate_down(0)
        need_b = self.bias_term_ and self.param_propagate_down(1)
        if head == "predict" and slope is None and ops.predict_flow_conv_backward_supported(x.shape[0], x.shape[1], x.shape[2], x.shape[3]):
            blob, c0 = Fn._channel_slice(x)
            return ops.predict_flow_conv_backward((blob, c0, x.shape[1]), w, g.contiguous(), need_x, need_w, need_b)
        if head == "upsample" and slope is None:
            return ops.upsample_flow_deconv_backward(x.contiguous(), w, g.contiguous(), need_x, need_w, need_b)
        return Fn.conv_backward(x, w, y if slope is not None else None, g, self.stride_, self.pad_, slope if slope is not None else 0.0,
                                self.transposed, need_x, need_w, need_b)

    def _head_kind(self):
        return None

    def Backward_gpu(self, top, propagate_down, bottom):
        CHECK(self.backend_ is None, "Backward runs on the default backend (flownet2_amd.functional) only")
        head = self._head_kind()
        if getattr(self, "_stacked", None) is not None:
            x, y = self._stacked
            n = x.shape[0] // len(bottom)
            g = torch.cat([self._fold(t.mutable_gpu_diff()) for t in top], 0)
            gx, gw, db = self._backward_one(x, y, g, self._slope(0), any(propagate_down), head)
            self._accumulate(0, gw)
            if self.bias_term_:
                self._accumulate(1, db)
            for i, b in enumerate(bottom):
                if propagate_down[i]:
                    b.diff = self._unfold(gx[i * n:(i + 1) * n], b)
            return
        for i, (b, t) in enumerate(zip(bottom, top)):
            gx, gw, db = self._backward_one(self._fold(b.data), self._fold(t.data), self._fold(t.mutable_gpu_diff()), self._slope(i),
                                            bool(propagate_down[i]), head, i)
            self._accumulate(0, gw)
            if self.bias_term_:
                self._accumulate(1, db)
            if propagate_down[i]:
                b.diff = self._unfold(gx, b)

    def _backend(self):
        if self.backend_ is not None:
            return self.backend_
        from . import functional
        return functional


class ConvolutionLayer(_ConvBase):
    def type(self): return "Convolution"

    def Forward_gpu(self, bottom, top):
        from . import nets
        be = self._backend()
        w, b = self.blobs_[0].data, (self.blobs_[1].data if self.bias_term_ else None)
        k, s, p = self.kernel_, self.stride_, self.pad_

        def one(x, slope):
            if not self.plain_:
                return self._general_one(x, slope, be)
            if k == 1 and s == 1 and p == 0 and slope is None and getattr(self, "diagonal_", None) is not None:
                # the deploy tail's SCALE convolution (weight_filler diagonal, run-flownet.py:47-48): y[c] = diag[c] x[c] + 0 x[other]
                y = x * self.diagonal_.view(1, -1, 1, 1)
                return y + b.view(1, -1, 1, 1) if (b is not None and bool((b != 0).any())) else y
            if k == 3 and s == 1 and p == 1 and self.num_output_ == 2 and slope is None and hasattr(be, "predict_flow_conv"):
                return be.predict_flow_conv(x, w, b)                                      # the predict_flow heads (csrc/flow_head.hip)
            return nets.conv_forward(x, w, b if b is not None else torch.zeros(self.num_output_, device=x.device), s, p,
                                     slope is not None, be, slope=slope)
        self._forward_all(bottom, top, one)

    def _head_kind(self):
        return "predict" if (self.kernel_, self.stride_, self.pad_, self.num_output_) == (3, 1, 1, 2) else None

    def note_weights_changed(self):
        """After the weights were (re)loaded: a 1x1 weight that is diagonal is applied as a per-channel scale (exactly what the zero
        off-diagonal products add up to for finite inputs)."""
        self.diagonal_ = None
        w = self.blobs_[0].data
        if self.kernel_ == 1 and w.shape[0] == w.shape[1]:
            m = w.view(w.shape[0], w.shape[1])
            d = torch.diagonal(m)
            if bool((m - torch.diag(d) == 0).all()):
                self.diagonal_ = d.contiguous()


class DeconvolutionLayer(_ConvBase):
    transposed = True

    def type(self): return "Deconvolution"

    def Forward_gpu(self, bottom, top):
        from . import nets
        be = self._backend()
        w, b = self.blobs_[0].data, (self.blobs_[1].data if self.bias_term_ else None)
        k, s, p = self.kernel_, self.stride_, self.pad_

        def one(x, slope):
            if not self.plain_:
                return self._general_one(x, slope, be)
            if (k, s, p) == (4, 2, 1) and w.shape[0] == 2 and w.shape[1] == 2 and slope is None and hasattr(be, "upsample_flow_deconv"):
                return be.upsample_flow_deconv(x, w, b)                                   # the upsample_flow heads (csrc/flow_head.hip)
            if (k, s, p) == (4, 2, 1):
                bb = b if b is not None else torch.zeros(self.num_output_, device=x.device)
                return nets.deconv_forward(x, w, bb, slope is not None, be, slope=slope)
            y = be.lib_conv_transpose2d(x, w, b, s, p) if hasattr(be, "lib_conv_transpose2d") else torch.nn.functional.conv_transpose2d(x, w, b, stride=s, padding=p)
            return torch.nn.functional.leaky_relu(y, slope) if slope is not None else y       # (a geometry outside FlowNet's: COUNTED in LIBRARY_FALLBACKS)
        self._forward_all(bottom, top, one)

    def _head_kind(self):
        w = self.blobs_[0].data
        return "upsample" if (self.kernel_, self.stride_, self.pad_) == (4, 2, 1) and w.shape[0] == 2 and w.shape[1] == 2 else None

    def note_weights_changed(self):
        pass


class ReLULayer(Layer):
    def type(self): return "ReLU"
    def ExactNumBottomBlobs(self): return 1
    def ExactNumTopBlobs(self): return 1

    def LayerSetUp(self, bottom, top):
        self.negative_slope_ = float(self.layer_param_.relu_param.get("negative_slope", 0.0))
        self.folded_ = False                    # True: the producing Convolution / Deconvolution applies it (executor peephole)

    def Reshape(self, bottom, top):
        top[0].ReshapeLike(bottom[0])

    def Forward_gpu(self, bottom, top):
        if self.folded_:
            if top[0] is not bottom[0]:
                top[0].data = bottom[0].data
            return
        x = bottom[0].data
        be = self.backend_
        if x.is_cuda and x.is_contiguous() and (be is None or hasattr(be, "conv_bias_leaky_relu")):
            from . import ops
            y = x if top[0] is bottom[0] else x.clone()
            top[0].data = ops.bias_leaky_relu_(y, None, self.negative_slope_)             # csrc/bias_act.hip, in place
        else:
            top[0].data = torch.nn.functional.leaky_relu(x, self.negative_slope_)

    def Backward_gpu(self, top, propagate_down, bottom):                                  # relu_layer.cu:33-60
        if not propagate_down[0]:
            return
        g = top[0].mutable_gpu_diff()
        if self.folded_:                        # the producing Convolution undoes the activation in its own backward pass
            bottom[0].diff = g
            return
        # in place the bottom data IS the top data; for a positive slope its sign is the input's (the reference reads bottom_data)
        y = top[0].data
        if y.is_cuda and y.is_contiguous():
            from . import ops
            bottom[0].diff = ops.bias_leaky_relu_backward(y, g.contiguous(), self.negative_slope_, False)[0]
        else:
            bottom[0].diff = g * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, self.negative_slope_))


class EltwiseLayer(Layer):
    def type(self): return "Eltwise"
    def MinBottomBlobs(self): return 1                                                   # eltwise_layer.hpp:29 (this fork)
    def ExactNumTopBlobs(self): return 1

    def LayerSetUp(self, bottom, top):
        ep = self.layer_param_.eltwise_param
        coeff = list(ep.get("coeff", []))
        CHECK(len(coeff) == 0 or len(coeff) == len(bottom), "Eltwise Layer takes one coefficient per bottom blob.")   # cpp:12-14
        self.op_ = str(ep.get("operation", "SUM"))
        CHECK(not (self.op_ == "PROD" and coeff), "Eltwise layer only takes coefficients for summation.")             # cpp:15-17
        self.coeffs_ = [float(c) for c in coeff] if coeff else [1.0] * len(bottom)
        self.stable_prod_grad_ = bool(ep.get("stable_prod_grad", True))                                               # caffe.proto: default true

    def Reshape(self, bottom, top):
        for b in bottom[1:]:
            CHECK(b.shape() == bottom[0].shape(), "bottom shapes differ")                 # cpp:29-31
        top[0].ReshapeLike(bottom[0])

    def Forward_gpu(self, bottom, top):
        xs = [b.data for b in bottom]
        if self.op_ == "PROD":
            y = xs[0] * xs[1] if len(xs) > 1 else xs[0].clone()
            for x in xs[2:]:
                y = y * x
        elif self.op_ == "MAX":
            y = xs[0].clone()
            for x in xs[1:]:
                y = torch.maximum(y, x)
        else:
            # eltwise_layer.cu:46-52: top = 0; top = coeff_i * bottom_i + top for every i.  0 + c x == c x, 1 a + (-1) b == a - b exactly
            c = self.coeffs_
            if len(xs) == 1:
                y = xs[0] * c[0]
            elif len(xs) == 2 and c == [1.0, -1.0]:
                y = xs[0] - xs[1]
            elif len(xs) == 2 and c == [1.0, 1.0]:
                y = xs[0] + xs[1]
            else:
                y = xs[0] * c[0]
                for x, ci in zip(xs[1:], c[1:]):
                    y = torch.add(y, x, alpha=ci)
        top[0].data = y

    def Backward_gpu(self, top, propagate_down, bottom):                                  # eltwise_layer.cu:68-118
        g = top[0].mutable_gpu_diff()
        for i, b in enumerate(bottom):
            if not propagate_down[i]:
                continue
            if self.op_ == "PROD" and not self.stable_prod_grad_:
                b.diff = (top[0].data / b.data) * g                    # eltwise_layer.cu:109-111: top / bottom (0 / 0 = NaN there too), then x top_diff
            elif self.op_ == "PROD":
                d = None                                               # :97-108: the product of the OTHER bottoms, in order, then x top_diff
                for j, o in enumerate(bottom):
                    if j != i:
                        d = o.data.clone() if d is None else o.data * d
                b.diff = g.clone() if d is None else d * g
            elif self.op_ == "MAX":
                # MaxForward (eltwise_layer.cu:10-31) keeps the running top only where it is STRICTLY greater (`a > b`, else b): on a tie the
                # LAST bottom that holds the maximum is recorded in the mask, and MaxBackward routes the gradient by that mask
                last = torch.ones_like(g, dtype=torch.bool)
                for j in range(i + 1, len(bottom)):
                    last &= bottom[j].data < top[0].data
                b.diff = g * ((b.data == top[0].data) & last).to(g.dtype)
            else:
                b.diff = g.clone() if self.coeffs_[i] == 1.0 else g * self.coeffs_[i]


class ConcatLayer(Layer):
    def type(self): return "Concat"
    def MinBottomBlobs(self): return 1
    def ExactNumTopBlobs(self): return 1

    def LayerSetUp(self, bottom, top):
        cp = self.layer_param_.concat_param
        CHECK(not ("axis" in cp and "concat_dim" in cp), "Either axis or concat_dim should be specified; not both.")   # cpp:13-14
        self.axis_ = int(cp.get("concat_dim", cp.get("axis", 1)))

    def Reshape(self, bottom, top):
        shape = bottom[0].shape()
        for b in bottom[1:]:
            s = b.shape()
            CHECK(len(s) == len(shape) and all(s[i] == shape[i] for i in range(len(s)) if i != self.axis_),
                  "All inputs must have the same shape, except at concat_axis.")          # cpp:42-49
            shape[self.axis_] += s[self.axis_]
        top[0].Reshape(*shape)

    def Forward_gpu(self, bottom, top):
        # one bottom: the top SHARES the bottom's storage, like the reference (concat_layer.cpp:50-53 ShareData / ShareDiff)
        top[0].data = bottom[0].data if len(bottom) == 1 else torch.cat([b.data for b in bottom], self.axis_)

    def Backward_gpu(self, top, propagate_down, bottom):                                  # concat_layer.cu:47-74
        g = top[0].mutable_gpu_diff()
        if len(bottom) == 1:
            bottom[0].diff = g
            return
        off = 0
        for i, b in enumerate(bottom):
            n = b.shape(self.axis_)
            if propagate_down[i]:
                b.diff = g.narrow(self.axis_, off, n)       # a channel-slice VIEW of the Concat's top_diff: the consumers read it in place
            off += n


class SliceLayer(Layer):
    def type(self): return "Slice"
    def ExactNumBottomBlobs(self): return 1
    def MinTopBlobs(self): return 1

    def LayerSetUp(self, bottom, top):
        sp = self.layer_param_.slice_param
        CHECK(not ("axis" in sp and "slice_dim" in sp), "Either axis or slice_dim should be specified; not both.")     # cpp:13-14
        self.axis_ = int(sp.get("slice_dim", sp.get("axis", 1)))
        self.slice_point_ = [int(v) for v in sp.get("slice_point", [])]

    def Reshape(self, bottom, top):
        n = bottom[0].shape(self.axis_)
        if self.slice_point_:
            CHECK(len(self.slice_point_) == len(top) - 1, "slice_point count must be top count - 1")                  # cpp:50
            cuts = [0] + self.slice_point_ + [n]
            CHECK(all(cuts[i] < cuts[i + 1] for i in range(len(cuts) - 1)), "slice points must be increasing")         # cpp:56
        else:
            CHECK(n % len(top) == 0, "Number of top blobs must evenly divide the slice axis")                          # cpp:67-70
            step = n // len(top)
            cuts = [i * step for i in range(len(top) + 1)]
        self.cuts_ = cuts
        for i, t in enumerate(top):
            s = bottom[0].shape()
            s[self.axis_] = cuts[i + 1] - cuts[i]
            t.Reshape(*s)

    def Forward_gpu(self, bottom, top):
        x = bottom[0].data
        if len(top) == 1:                                   # slice_layer.cpp:69-72: one top shares the bottom's storage
            top[0].data = x
            return
        for i, t in enumerate(top):
            # every top owns its storage (slice_layer.cpp:76-95 copies): a narrow() that is already contiguous (batch 1, or a slice along
            # axis 0) is a VIEW of the bottom, and an in-place layer behind it would write through into the bottom and the other tops
            y = x.narrow(self.axis_, self.cuts_[i], self.cuts_[i + 1] - self.cuts_[i])
            t.data = y.clone() if y.is_contiguous() else y.contiguous()

    def Backward_gpu(self, top, propagate_down, bottom):                                  # slice_layer.cu:49-75
        if not propagate_down[0]:
            return
        bottom[0].diff = top[0].mutable_gpu_diff() if len(top) == 1 else torch.cat([t.mutable_gpu_diff() for t in top], self.axis_)


class SilenceLayer(Layer):
    def type(self): return "Silence"
    def MinBottomBlobs(self): return 1
    def ExactNumTopBlobs(self): return 0
    def Reshape(self, bottom, top): pass
    def Forward_gpu(self, bottom, top): pass

    def Backward_gpu(self, top, propagate_down, bottom):                                  # silence_layer.cu:16-27
        for i, b in enumerate(bottom):
            if propagate_down[i]:
                b.diff = torch.zeros_like(b.data)


class SplitLayer(Layer):
    """split_layer.cpp:8-27, split_layer.cu:8-33: every top SHARES the bottom's data; the bottom's diff is the sum of the tops' diffs (the first
    two added, the rest accumulated in order).  Inserted by Net::Init (InsertSplits) wherever a blob has more than one consumer."""

    def type(self): return "Split"
    def ExactNumBottomBlobs(self): return 1
    def MinTopBlobs(self): return 1

    def Reshape(self, bottom, top):
        for t in top:
            CHECK(t is not bottom[0], "Split Layer does not allow in-place computation.")   # split_layer.cpp:13-18
            t.ReshapeLike(bottom[0])

    def Forward_gpu(self, bottom, top):
        for t in top:
            t.data = bottom[0].data

    def Backward_gpu(self, top, propagate_down, bottom):
        if not propagate_down[0]:
            return
        if len(top) == 1:
            bottom[0].diff = top[0].mutable_gpu_diff().clone()
            return
        d = top[0].mutable_gpu_diff() + top[1].mutable_gpu_diff()
        for t in top[2:]:
            d = d + t.mutable_gpu_diff()
        bottom[0].diff = d


class InputLayer(Layer):
    """input_layer.cpp:8-27: tops shaped by input_param.shape (one shape for all tops, or one per top)."""

    def type(self): return "Input"
    def ExactNumBottomBlobs(self): return 0
    def MinTopBlobs(self): return 1

    def LayerSetUp(self, bottom, top):
        shapes = self.layer_param_.input_param.get("shape", [])
        if isinstance(shapes, dict):
            shapes = [shapes]
        CHECK(len(shapes) in (0, 1, len(top)), "Must specify 'shape' once, once per top blob, or not at all")           # cpp:14-17
        for i, t in enumerate(top):
            if shapes:
                t.Reshape(*[int(d) for d in shapes[i if len(shapes) > 1 else 0].get("dim", [])])

    def Reshape(self, bottom, top): pass
    def Forward_gpu(self, bottom, top): pass


for _name, _cls in (("Convolution", ConvolutionLayer), ("Deconvolution", DeconvolutionLayer), ("ReLU", ReLULayer), ("Eltwise", EltwiseLayer),
                    ("Concat", ConcatLayer), ("Slice", SliceLayer), ("Silence", SilenceLayer), ("Split", SplitLayer), ("Input", InputLayer)):
    L.REGISTER_LAYER_CLASS(_name, _cls)
