"""Convolution over 0, 1 and 3 spatial axes, `axis` and force_nd_im2col from Python: functional.lib_conv3d / lib_conv_transpose3d and the
stock-layer mirror (stock_layers._ConvBase) building prototxts with 5-, 3- and 2-axis inputs.

CPU tier: the prototxts build as Nets, weight and top shapes are Caffe's (base_conv_layer.cpp:135-140, 198-207), the forward equals the fp64
layers within fp32 rounding, Caffe's CHECKs raise CheckError with the reference's messages, `axis` folds the leading axes into the batch,
force_nd_im2col changes nothing.  GPU tier: under set_general_convolution("own") a TRAIN-phase Net with a 3-D Convolution and a 3-D
Deconvolution, forward and Net.Backward against fp64 layer by layer at the bounds of tests/test_conv_general.py (every layer's reference is
computed from the fp32 blobs the net itself fed that layer) with nothing counted in LIBRARY_FALLBACKS; under the default the library
fallback is counted and FN2_STRICT=1 raises (a child process); the bit identities of force_nd_im2col, of `axis` and of a 1-axis layer."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_general_cases import scale_of
from conv_volume_cases import ROWS, case, fields, out_size, row_id
from flownet2_amd import functional as Fn
from flownet2_amd import net as fnet
from flownet2_amd.layers import CheckError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_ROWS = [ROWS[0], ROWS[2], ROWS[3], ROWS[4], ROWS[8], ROWS[10], ROWS[11]]

PROTOTXT = """
name: "volume"
force_backward: true
input: "data"
input_shape { dim: 2 dim: 4 dim: 5 dim: 6 dim: 7 }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv"
  convolution_param { num_output: 6 kernel_size: 3 kernel_size: 2 kernel_size: 3 stride: 2 stride: 1 stride: 1 pad: 1 pad: 0 pad: 2
                      dilation: 1 dilation: 2 dilation: 1 group: 2
                      weight_filler { type: "gaussian" std: 0.1 } bias_filler { type: "gaussian" std: 0.5 } } }
layer { name: "relu" type: "ReLU" bottom: "conv" top: "conv" relu_param { negative_slope: 0.1 } }
layer { name: "up" type: "Deconvolution" bottom: "conv" top: "up"
  convolution_param { num_output: 4 kernel_size: 4 stride: 2 pad: 1 bias_term: false weight_filler { type: "gaussian" std: 0.1 } } }
"""
CONV_ARGS = dict(stride=(2, 1, 1), padding=(1, 0, 2), dilation=(1, 2, 1), groups=2)
UP_ARGS = dict(stride=2, padding=1)
SLOPE = 0.1
CONV_SHAPE, UP_SHAPE = [2, 6, 3, 4, 9], [2, 4, 6, 8, 18]      # (5 + 2 - 3) / 2 + 1, 6 - 3 + 1, 7 + 4 - 3 + 1; 2 (n - 1) + 4 - 2 each


@pytest.fixture()
def switch():
    was = Fn.general_convolution()
    yield
    Fn.set_general_convolution(was)


def close(what, got, ref, bound):
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref.detach().numpy()).max())
    print("%s: error %.3g, bound %.3g, ratio %.3f" % (what, err, bound, err / bound))
    return tuple(got.shape) == tuple(ref.shape) and err <= bound


def scale(t):
    return max(1.0, float(t.detach().abs().max()))


def net_forward_checks(net, x):
    """Shapes as Caffe's, and each layer against fp64 on the blob the net fed it."""
    conv, up = net.layer_by_name("conv"), net.layer_by_name("up")
    assert [b.shape() for b in conv.blobs_] == [[6, 2, 3, 2, 3], [6]]              # [num_output, C / group, kd, kh, kw]
    assert [b.shape() for b in up.blobs_] == [[6, 4, 4, 4, 4]]                     # [C, num_output / group, kd, kh, kw], no bias
    assert net.blobs["conv"].shape() == CONV_SHAPE and net.blobs["up"].shape() == UP_SHAPE
    out = net.forward(data=x)
    assert list(out) == ["up"]
    w1, b1, w2 = (b.data.detach().cpu().double() for b in (conv.blobs_[0], conv.blobs_[1], up.blobs_[0]))
    y1 = F.leaky_relu(F.conv3d(x.double(), w1, b1, **CONV_ARGS), SLOPE)
    got1 = net.blobs["conv"].data
    assert close("Net conv3d + ReLU", got1, y1, 4e-6 * scale(y1))
    y2 = F.conv_transpose3d(got1.detach().cpu().double(), w2, None, **UP_ARGS)
    assert close("Net deconv3d", out["up"], y2, 4e-6 * scale(y2))
    return w1, b1, w2


def data(seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(2, 4, 5, 6, 7, generator=gen), torch.randn(*UP_SHAPE, generator=gen)


# ------------------------------------------------------------------------------------------------------------------------------ CPU tier
def test_a_five_axis_prototxt_builds_on_the_cpu_with_caffes_shapes_and_the_fp64_forward():
    """On the parent this raised "N-dimensional convolution (axis, force_nd_im2col) is not supported"."""
    net = fnet.Net(PROTOTXT, phase="TRAIN", device="cpu")
    conv = net.layer_by_name("conv")
    assert (conv.channel_axis_, conv.num_spatial_axes_, conv.plain_) == (1, 3, False)
    assert (conv.kernel_shape_, conv.stride_shape_, conv.pad_shape_, conv.dilation_shape_, conv.group_) == ((3, 2, 3), (2, 1, 1), (1, 0, 2), (1, 2, 1), 2)
    up = net.layer_by_name("up")
    assert (up.kernel_shape_, up.stride_shape_, up.pad_shape_, up.dilation_shape_, up.group_) == ((4, 4, 4), (2, 2, 2), (1, 1, 1), (1, 1, 1), 1)
    net_forward_checks(net, data()[0])


ONE_AXIS = """
input: "data"
input_shape { dim: 2 dim: 6 dim: 37 }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv"
  convolution_param { num_output: 10 kernel_size: 7 stride: 2 pad: 3 dilation: 2 group: 2 weight_filler { type: "gaussian" std: 0.1 }
                      bias_filler { type: "gaussian" std: 0.5 } } }
layer { name: "up" type: "Deconvolution" bottom: "conv" top: "up"
  convolution_param { num_output: 4 kernel_size: 4 stride: 2 pad: 1 weight_filler { type: "gaussian" std: 0.1 } } }
"""
NO_AXIS = """
input: "data"
input_shape { dim: 3 dim: 5 }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv"
  convolution_param { num_output: 7 kernel_size: 1 weight_filler { type: "gaussian" std: 0.1 } bias_filler { type: "gaussian" std: 0.5 } } }
"""


def test_one_and_no_spatial_axis_fold_onto_the_two_axis_layer():
    net = fnet.Net(ONE_AXIS, phase="TEST", device="cpu")
    conv, up = net.layer_by_name("conv"), net.layer_by_name("up")
    assert (conv.num_spatial_axes_, conv.kernel_hw_, conv.stride_hw_, conv.pad_hw_, conv.dilation_hw_, conv.plain_) == (1, (1, 7), (1, 2), (0, 3), (1, 2), False)
    assert [b.shape() for b in conv.blobs_] == [[10, 3, 7], [10]] and [b.shape() for b in up.blobs_] == [[10, 4, 4], [4]]
    assert net.blobs["conv"].shape() == [2, 10, 16] and net.blobs["up"].shape() == [2, 4, 32]      # (37 + 6 - 13) / 2 + 1; 2 (16 - 1) + 4 - 2
    x = torch.randn(2, 6, 37, generator=torch.Generator().manual_seed(5))
    out = net.forward(data=x)
    w1, b1, w2, b2 = (b.data.double() for b in conv.blobs_ + up.blobs_)
    y1 = F.conv1d(x.double(), w1, b1, stride=2, padding=3, dilation=2, groups=2)
    assert close("1-axis conv", net.blobs["conv"].data, y1, 4e-6 * scale(y1))
    y2 = F.conv_transpose1d(net.blobs["conv"].data.double(), w2, b2, stride=2, padding=1)
    assert close("1-axis deconv", out["up"], y2, 4e-6 * scale(y2))
    net = fnet.Net(NO_AXIS, phase="TEST", device="cpu")
    conv = net.layer_by_name("conv")
    assert (conv.num_spatial_axes_, conv.kernel_shape_, conv.kernel_hw_, conv.plain_) == (0, (), (1, 1), False)
    assert [b.shape() for b in conv.blobs_] == [[7, 5], [7]] and net.blobs["conv"].shape() == [3, 7]
    x = torch.randn(3, 5, generator=torch.Generator().manual_seed(6))
    y = x.double() @ conv.blobs_[0].data.double().t() + conv.blobs_[1].data.double()
    assert close("0-axis conv", net.forward(data=x)["conv"], y, 4e-6 * scale(y))


TWO_AXIS = """
input: "data"
input_shape { dim: 2 dim: 3 dim: 4 dim: 9 dim: 8 }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv"
  convolution_param { num_output: 6 kernel_size: 3 stride: 2 pad: 1 axis: 2
                      weight_filler { type: "gaussian" std: 0.1 } bias_filler { type: "gaussian" std: 0.5 } } }
"""


def axis_pair(device):
    """The layer with axis: 2 on a [2, 3, 4, 9, 8] blob and the same layer (the same weights) with axis: 1 on its [6, 4, 9, 8] view."""
    deep = fnet.Net(TWO_AXIS, phase="TEST", device=device)
    flat = fnet.Net(TWO_AXIS.replace("dim: 2 dim: 3 dim: 4", "dim: 6 dim: 4").replace(" axis: 2", " axis: 1"), phase="TEST", device=device)
    for a, b in zip(deep.layer_by_name("conv").blobs_, flat.layer_by_name("conv").blobs_):
        assert a.shape() == b.shape()
        b.data = a.data.clone()
    return deep, flat


def test_axis_folds_the_leading_axes_into_the_batch():
    deep, flat = axis_pair("cpu")
    conv = deep.layer_by_name("conv")
    assert (conv.channel_axis_, conv.num_spatial_axes_, conv.plain_) == (2, 2, True) and flat.layer_by_name("conv").plain_
    assert conv.blobs_[0].shape() == [6, 4, 3, 3] and deep.blobs["conv"].shape() == [2, 3, 6, 5, 4] and flat.blobs["conv"].shape() == [6, 6, 5, 4]
    x = torch.randn(2, 3, 4, 9, 8, generator=torch.Generator().manual_seed(7))
    assert torch.equal(deep.forward(data=x)["conv"].reshape(6, 6, 5, 4), flat.forward(data=x.view(6, 4, 9, 8))["conv"])
    # a negative axis counts from the end (blob.hpp:121-132): -3 on five axes is 2
    again = fnet.Net(TWO_AXIS.replace("axis: 2", "axis: -3"), phase="TEST", device="cpu").layer_by_name("conv")
    assert (again.channel_axis_, again.num_spatial_axes_) == (2, 2)


FLAT = """
input: "data"
input_shape { dim: 2 dim: 6 dim: 11 dim: 14 }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv"
  convolution_param { num_output: 8 kernel_h: 2 kernel_w: 3 stride_h: 2 stride_w: 1 pad_h: 1 pad_w: 2 dilation: 2 dilation: 3 group: 2
                      weight_filler { type: "gaussian" std: 0.1 } bias_filler { type: "gaussian" std: 0.5 } } }
layer { name: "plain" type: "Convolution" bottom: "conv" top: "plain"
  convolution_param { num_output: 5 kernel_size: 3 stride: 1 pad: 1 weight_filler { type: "gaussian" std: 0.1 } } }
"""


def forced_pair(device):
    nets = [fnet.Net(FLAT.replace("group: 2", "group: 2" + flag).replace("pad: 1 weight", "pad: 1" + flag + " weight"), phase="TEST", device=device)
            for flag in ("", " force_nd_im2col: true")]
    return nets


def test_force_nd_im2col_is_accepted_and_changes_nothing():
    plain, forced = forced_pair("cpu")
    for name in ("conv", "plain"):
        a, b = plain.layer_by_name(name), forced.layer_by_name(name)
        assert b.layer_param_.convolution_param.get("force_nd_im2col") and not a.layer_param_.convolution_param.get("force_nd_im2col", False)
        assert (a.plain_, a.folded_, a.kernel_hw_, a.blobs_[0].shape()) == (b.plain_, b.folded_, b.kernel_hw_, b.blobs_[0].shape())
    x = torch.randn(2, 6, 11, 14, generator=torch.Generator().manual_seed(8))
    assert torch.equal(plain.forward(data=x)["plain"], forced.forward(data=x)["plain"])


@pytest.mark.parametrize("old, new, message", [
    ("kernel_size: 3 kernel_size: 2 kernel_size: 3", "kernel_h: 3 kernel_w: 2", "kernel_h & kernel_w can only be used for 2D convolution."),
    ("stride: 2 stride: 1 stride: 1", "stride_h: 2 stride_w: 1", "stride_h & stride_w can only be used for 2D convolution."),
    ("pad: 1 pad: 0 pad: 2", "pad_h: 1 pad_w: 0", "pad_h & pad_w can only be used for 2D convolution."),
    ("kernel_size: 3 kernel_size: 2 kernel_size: 3", "kernel_size: 3 kernel_size: 2",
     "kernel_size must be specified once, or once per spatial dimension (kernel_size specified 2 times; 3 spatial dims)."),
    ("kernel_size: 3 kernel_size: 2 kernel_size: 3", "", "kernel_size must be specified once, or once per spatial dimension (kernel_size specified 0 times; 3 spatial dims)."),
    ("stride: 2 stride: 1 stride: 1", "stride: 2 stride: 1", "stride must be specified once, or once per spatial dimension (stride specified 2 times; 3 spatial dims)."),
    ("pad: 1 pad: 0 pad: 2", "pad: 1 pad: 0 pad: 2 pad: 0", "pad must be specified once, or once per spatial dimension (pad specified 4 times; 3 spatial dims)."),
    ("dilation: 1 dilation: 2 dilation: 1", "dilation: 1 dilation: 2",
     "dilation must be specified once, or once per spatial dimension (dilation specified 2 times; 3 spatial dims)."),
    ("kernel_size: 3 kernel_size: 2 kernel_size: 3", "kernel_size: 3 kernel_size: 0 kernel_size: 3", "Filter dimensions must be nonzero."),
    ("stride: 2 stride: 1 stride: 1", "stride: 0", "Stride dimensions must be nonzero."),
    ("dilation: 1 dilation: 2 dilation: 1", "dilation: 0", "Dilation dimensions must be nonzero."),
    ("group: 2", "group: 3", "channels_ % group_ == 0"),
    ("num_output: 6", "num_output: 7", "Number of output should be multiples of group."),
    ("dim: 2 dim: 4 dim: 5 dim: 6 dim: 7", "dim: 2 dim: 4 dim: 5 dim: 6 dim: 7 dim: 3", "4 spatial axes"),       # refused by name, with the count
    ("group: 2", "group: 2 axis: 5", "axis 5 out of range"),
])
def test_caffes_checks_raise_with_the_references_messages(old, new, message):
    assert old in PROTOTXT
    with pytest.raises(CheckError) as e:
        fnet.Net(PROTOTXT.replace(old, new, 1), phase="TEST", device="cpu")
    assert message in str(e.value)


def test_cpu_tensors_go_to_torch_with_the_same_arguments(switch):
    x, w = torch.randn(1, 6, 4, 6, 7), torch.randn(4, 3, 2, 3, 2)
    want = F.conv3d(x, w, None, stride=(1, 2, 1), padding=(0, 1, 0), dilation=(2, 1, 2), groups=2)
    xt, wt = torch.randn(1, 6, 2, 3, 4), torch.randn(6, 2, 2, 3, 2)
    want_t = F.conv_transpose3d(xt, wt, None, stride=(2, 3, 2), padding=(1, 0, 1), dilation=(1, 1, 2), groups=3)
    for name in ("library", "own"):
        Fn.set_general_convolution(name)
        before = Fn.LIBRARY_FALLBACKS[0]
        assert torch.equal(Fn.lib_conv3d(x, w, None, (1, 2, 1), (0, 1, 0), dilation=(2, 1, 2), groups=2), want)
        assert torch.equal(Fn.lib_conv_transpose3d(xt, wt, None, (2, 3, 2), (1, 0, 1), dilation=(1, 1, 2), groups=3), want_t)
        assert Fn.LIBRARY_FALLBACKS[0] == before


# ------------------------------------------------------------------------------------------------------------------------------ GPU tier
def call(row, c, requires_grad=True):
    tr, N, Cin, size, Cout, kernel, stride, pad, dilation, group = fields(row)
    x, w, b = (torch.tensor(c[n], device="cuda").requires_grad_(requires_grad) for n in ("x", "w", "b"))
    return x, w, b, (Fn.lib_conv_transpose3d if tr else Fn.lib_conv3d)(x, w, b, stride, pad, dilation=dilation, groups=group)


@pytest.mark.gpu
@pytest.mark.parametrize("row", PY_ROWS, ids=row_id)
def test_own_runs_forward_and_backward_on_the_depth_kernels(switch, row, monkeypatch):
    c = case(row)
    N, voxels = row[1], int(np.prod(out_size(row)))
    Fn.set_general_convolution("own")
    monkeypatch.setenv("FN2_STRICT", "1")                             # would raise at the first call that leaves the own kernels
    before = Fn.LIBRARY_FALLBACKS[0]
    x, w, b, top = call(row, c)
    top.backward(torch.tensor(c["g"], device="cuda"))
    assert Fn.LIBRARY_FALLBACKS[0] == before
    for what, got, ref, bound in (("forward", top.detach(), c["top"], 4e-6 * scale_of(c["top"])),
                                  ("data gradient", x.grad, c["gx"], 4e-6 * scale_of(c["gx"])),
                                  ("weight gradient", w.grad, c["gw"], 2e-6 * scale_of(c["gw"]) * math.sqrt(N * voxels)),
                                  ("bias gradient", b.grad, c["gb"], 2e-6 * scale_of(c["gb"]))):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print("%s %s: error %.3g, bound %.3g, ratio %.3f" % (what, row_id(row), err, bound, err / bound))
        assert got.shape == ref.shape and err <= bound, what
    assert torch.equal(call(row, c)[3], top)                          # a second call (the cached operand) gives the same bits


@pytest.mark.gpu
def test_the_train_net_runs_forward_and_backward_on_the_depth_kernels(switch, monkeypatch):
    Fn.set_general_convolution("own")
    monkeypatch.setenv("FN2_STRICT", "1")
    before = Fn.LIBRARY_FALLBACKS[0]
    x, g = data()
    net = fnet.Net(PROTOTXT, phase="TRAIN", device="cuda", with_backward=True)
    w1, b1, w2 = net_forward_checks(net, x)
    net.ClearParamDiffs()
    net.blobs["up"].diff = g.cuda()
    net.Backward()
    assert Fn.LIBRARY_FALLBACKS[0] == before
    conv, up = net.layer_by_name("conv"), net.layer_by_name("up")
    voxels_up, voxels_conv = 6 * 8 * 18, 3 * 4 * 9
    # the Deconvolution, at the fp32 blob the net fed it
    y1 = net.blobs["conv"].data.detach().cpu()
    a, w2g = y1.double().requires_grad_(True), w2.clone().requires_grad_(True)
    ga, gw2 = torch.autograd.grad(F.conv_transpose3d(a, w2g, None, **UP_ARGS), (a, w2g), g.double())
    g1 = net.blobs["conv"].diff.detach().cpu()
    assert close("Net deconv3d data gradient", g1, ga, 4e-6 * scale(ga))
    assert close("Net deconv3d weight gradient", up.blobs_[0].mutable_gpu_diff(), gw2, 2e-6 * scale(gw2) * math.sqrt(2 * voxels_up))
    # the Convolution with its folded ReLU, at the fp32 diff the net fed it (the mask from the net's own activations)
    masked = g1.double() * torch.where(y1 > 0, 1.0, SLOPE).double()
    xd, w1g, b1g = x.double().requires_grad_(True), w1.clone().requires_grad_(True), b1.clone().requires_grad_(True)
    gx, gw1, gb1 = torch.autograd.grad(F.conv3d(xd, w1g, b1g, **CONV_ARGS), (xd, w1g, b1g), masked)
    assert close("Net conv3d data gradient", net.blobs["data"].diff, gx, 4e-6 * scale(gx))
    assert close("Net conv3d weight gradient", conv.blobs_[0].mutable_gpu_diff(), gw1, 2e-6 * scale(gw1) * math.sqrt(2 * voxels_conv))
    assert close("Net conv3d bias gradient", conv.blobs_[1].mutable_gpu_diff(), gb1, 2e-6 * scale(gb1))


CHILD = """
import os, sys, torch
sys.path.insert(0, os.path.join({root!r}, "tests"))
import test_conv_volume_python as t
from flownet2_amd import functional as Fn, net as fnet
assert Fn.general_convolution() == "library"
net = fnet.Net(t.PROTOTXT, phase="TRAIN", device="cuda", with_backward=True)
before = Fn.LIBRARY_FALLBACKS[0]
t.net_forward_checks(net, t.data()[0])
print("fallbacks", Fn.LIBRARY_FALLBACKS[0] - before)
os.environ["FN2_STRICT"] = "1"
try:
    net.forward(data=t.data()[0])
    print("strict: no error")
except RuntimeError as e:
    print("strict:", e)
"""


@pytest.mark.gpu
def test_the_default_counts_the_library_fallback_and_strict_raises_in_a_child_process():
    env = {k: v for k, v in os.environ.items() if k not in ("FN2_CONV_GENERAL", "FN2_STRICT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fallbacks 2" in r.stdout                                   # one per volumetric layer
    assert "strict: flownet2_amd: no own kernel for Convolution" in r.stdout and "FN2_STRICT=1" in r.stdout


@pytest.mark.gpu
def test_force_nd_im2col_gives_the_bits_of_the_layer_without_it(switch):
    """Identity (c): through Net, a 2-D net (a grouped dilated rectangular layer on the general kernels and a plain 3x3 on the routed ones)
    with force_nd_im2col: true gives the bits of the same prototxt without it."""
    Fn.set_general_convolution("own")
    plain, forced = forced_pair("cuda")
    x = torch.randn(2, 6, 11, 14, generator=torch.Generator().manual_seed(8))
    a, b = plain.forward(data=x), forced.forward(data=x)
    assert torch.equal(a["plain"], b["plain"]) and torch.equal(plain.blobs["conv"].data, forced.blobs["conv"].data)


@pytest.mark.gpu
def test_axis_two_gives_the_bits_of_axis_one_on_the_view(switch):
    """Identity (d): axis: 2 on a [A, B, C, H, W] blob equals axis: 1 on its [A B, C, H, W] view."""
    Fn.set_general_convolution("own")
    deep, flat = axis_pair("cuda")
    x = torch.randn(2, 3, 4, 9, 8, generator=torch.Generator().manual_seed(7))
    got, want = deep.forward(data=x)["conv"], flat.forward(data=x.view(6, 4, 9, 8))["conv"]
    assert got.shape == (2, 3, 6, 5, 4) and torch.equal(got.reshape(6, 6, 5, 4), want)
    ref = F.conv2d(x.view(6, 4, 9, 8).double(), *(b.data.detach().cpu().double() for b in flat.layer_by_name("conv").blobs_), stride=2, padding=1)
    assert close("axis: 2", want, ref, 4e-6 * scale(ref))


@pytest.mark.gpu
def test_a_one_axis_net_gives_the_bits_of_the_folded_two_axis_functions(switch):
    """Identity (b) through Net: the [N, C, L] layers are lib_conv2d / lib_conv_transpose2d on [N, C, 1, L]."""
    Fn.set_general_convolution("own")
    net = fnet.Net(ONE_AXIS, phase="TEST", device="cuda")
    x = torch.randn(2, 6, 37, generator=torch.Generator().manual_seed(5))
    out = net.forward(data=x)
    conv, up = net.layer_by_name("conv"), net.layer_by_name("up")
    y1 = Fn.lib_conv2d(x.cuda()[:, :, None], conv.blobs_[0].data[:, :, None], conv.blobs_[1].data, (1, 2), (0, 3), dilation=(1, 2), groups=2)
    assert torch.equal(net.blobs["conv"].data, y1[:, :, 0])
    y2 = Fn.lib_conv_transpose2d(y1, up.blobs_[0].data[:, :, None], up.blobs_[1].data, (1, 2), (0, 1), dilation=(1, 1), groups=1)
    assert torch.equal(out["up"], y2[:, :, 0])
