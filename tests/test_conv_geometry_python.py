"""The widened general convolution from Python: functional.lib_conv2d / lib_conv_transpose2d with pair arguments, dilation and groups, and
the stock-layer mirror (stock_layers._ConvBase) building a prototxt with a grouped dilated rectangular Convolution and a depthwise 4x4 / 2
Deconvolution.

CPU tier: the prototxt builds as a Net, blob and top shapes are Caffe's, the forward equals the fp64 layers within fp32 rounding, Caffe's
CHECKs raise CheckError.  GPU tier: under set_general_convolution("own") forward and autograd gradients against fp64 at the bounds of
tests/test_conv_general.py with nothing counted in LIBRARY_FALLBACKS and FN2_STRICT=1 not raising; under "library" the same call is
counted; the Net on the GPU under "own", forward and Net.Backward against fp64 layer by layer (every layer's reference is computed from the
fp32 blobs the net itself fed that layer, so the single-layer bounds apply as they stand)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_general_cases import scale_of
from conv_geometry_cases import ROWS, case, out_hw, row_id
from flownet2_amd import functional as Fn
from flownet2_amd import net as fnet
from flownet2_amd.layers import CheckError

PY_ROWS = [ROWS[1], ROWS[3], ROWS[6], ROWS[9], ROWS[11], ROWS[14], ROWS[15]]      # rectangular, dilated, grouped, all at once; four deconvolutions' worth

PROTOTXT = """
name: "geometry"
force_backward: true
input: "data"
input_shape { dim: 2 dim: 6 dim: 11 dim: 14 }
layer { name: "conv" type: "Convolution" bottom: "data" top: "conv"
  convolution_param { num_output: 8 kernel_h: 2 kernel_w: 3 stride_h: 2 stride_w: 1 pad_h: 1 pad_w: 2 dilation: 2 dilation: 3 group: 2
                      weight_filler { type: "gaussian" std: 0.1 } bias_filler { type: "gaussian" std: 0.5 } } }
layer { name: "relu" type: "ReLU" bottom: "conv" top: "conv" relu_param { negative_slope: 0.1 } }
layer { name: "up" type: "Deconvolution" bottom: "conv" top: "up"
  convolution_param { num_output: 8 kernel_size: 4 stride: 2 pad: 1 group: 8 bias_term: false weight_filler { type: "gaussian" std: 0.1 } } }
"""
CONV_ARGS = dict(stride=(2, 1), padding=(1, 2), dilation=(2, 3), groups=2)
UP_ARGS = dict(stride=2, padding=1, groups=8)
SLOPE = 0.1


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
    assert [b.shape() for b in conv.blobs_] == [[8, 3, 2, 3], [8]]                 # [num_output, C / group, kh, kw]
    assert [b.shape() for b in up.blobs_] == [[8, 1, 4, 4]]                        # [C, num_output / group, kh, kw], no bias
    # (11 + 2 - (2 (2 - 1) + 1)) / 2 + 1 = 6, (14 + 4 - (3 (3 - 1) + 1)) / 1 + 1 = 12; 2 (6 - 1) + 4 - 2 = 12, 2 (12 - 1) + 4 - 2 = 24
    assert net.blobs["conv"].shape() == [2, 8, 6, 12] and net.blobs["up"].shape() == [2, 8, 12, 24]
    out = net.forward(data=x)
    assert list(out) == ["up"]
    w1, b1, w2 = (b.data.detach().cpu().double() for b in (conv.blobs_[0], conv.blobs_[1], up.blobs_[0]))
    y1 = F.leaky_relu(F.conv2d(x.double(), w1, b1, **CONV_ARGS), SLOPE)
    got1 = net.blobs["conv"].data
    assert close("Net conv + ReLU", got1, y1, 4e-6 * scale(y1))
    y2 = F.conv_transpose2d(got1.detach().cpu().double(), w2, None, **UP_ARGS)
    assert close("Net depthwise deconv", out["up"], y2, 4e-6 * scale(y2))
    return w1, b1, w2


# ------------------------------------------------------------------------------------------------------------------------------ CPU tier
def test_the_prototxt_builds_on_the_cpu_with_caffes_shapes_and_the_fp64_forward():
    net = fnet.Net(PROTOTXT, phase="TEST", device="cpu")
    conv = net.layer_by_name("conv")
    assert (conv.kernel_hw_, conv.stride_hw_, conv.pad_hw_, conv.dilation_hw_, conv.group_, conv.plain_) == ((2, 3), (2, 1), (1, 2), (2, 3), 2, False)
    up = net.layer_by_name("up")
    assert (up.kernel_hw_, up.stride_hw_, up.pad_hw_, up.dilation_hw_, up.group_, up.plain_) == ((4, 4), (2, 2), (1, 1), (1, 1), 8, False)
    net_forward_checks(net, torch.randn(2, 6, 11, 14, generator=torch.Generator().manual_seed(3)))


def test_a_plain_layer_stays_plain():
    text = PROTOTXT.replace("kernel_h: 2 kernel_w: 3 stride_h: 2 stride_w: 1 pad_h: 1 pad_w: 2 dilation: 2 dilation: 3 group: 2",
                            "kernel_h: 3 kernel_w: 3 stride: 2 stride: 2 pad_h: 1 pad_w: 1 dilation: 1")
    conv = fnet.Net(text, phase="TEST", device="cpu").layer_by_name("conv")
    assert conv.plain_ and (conv.kernel_, conv.stride_, conv.pad_) == (3, 2, 1) and conv.blobs_[0].shape() == [8, 6, 3, 3]


@pytest.mark.parametrize("old, new", [
    ("group: 2", "group: 4"),                                         # 6 % 4: channels_ % group_
    ("num_output: 8 kernel_h", "num_output: 9 kernel_h"),             # 9 % 2: "Number of output should be multiples of group."
    ("group: 8", "group: 3"),                                         # the Deconvolution: 8 % 3
    ("dilation: 2 dilation: 3", "dilation: 2 dilation: 0"),
    ("dilation: 2 dilation: 3", "dilation: 1 dilation: 2 dilation: 3"),
    ("kernel_size: 4", "kernel_size: 4 kernel_size: 4 kernel_size: 4"),
    ("stride: 2", "stride: 2 stride: 2 stride: 2"),
    ("kernel_h: 2", "kernel_size: 2 kernel_h: 2"),                    # "Either kernel_size or kernel_h/w should be specified; not both."
    ("kernel_w: 3", "kernel_w: 0"),                                   # "Filter dimensions must be nonzero."
    ("stride_h: 2", "stride_h: 0"),
])
def test_caffes_checks_raise(old, new):
    assert old in PROTOTXT
    with pytest.raises(CheckError):
        fnet.Net(PROTOTXT.replace(old, new, 1), phase="TEST", device="cpu")


def test_cpu_tensors_go_to_torch_with_the_same_arguments(switch):
    x, w = torch.randn(1, 6, 6, 7), torch.randn(4, 3, 3, 2)
    want = F.conv2d(x, w, None, stride=(2, 1), padding=(1, 0), dilation=(1, 2), groups=2)
    xt, wt = torch.randn(1, 6, 3, 4), torch.randn(6, 2, 3, 2)
    want_t = F.conv_transpose2d(xt, wt, None, stride=(3, 2), padding=(0, 1), dilation=(1, 2), groups=3)
    for name in ("library", "own"):
        Fn.set_general_convolution(name)
        before = Fn.LIBRARY_FALLBACKS[0]
        assert torch.equal(Fn.lib_conv2d(x, w, None, (2, 1), (1, 0), dilation=(1, 2), groups=2), want)
        assert torch.equal(Fn.lib_conv_transpose2d(xt, wt, None, (3, 2), (0, 1), dilation=(1, 2), groups=3), want_t)
        assert Fn.LIBRARY_FALLBACKS[0] == before


# ------------------------------------------------------------------------------------------------------------------------------ GPU tier
def call(row, c, requires_grad=True):
    tr, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group = row
    x, w, b = (torch.tensor(c[n], device="cuda").requires_grad_(requires_grad) for n in ("x", "w", "b"))
    return x, w, b, (Fn.lib_conv_transpose2d if tr else Fn.lib_conv2d)(x, w, b, (sh, sw), (ph, pw), dilation=(dh, dw), groups=group)


@pytest.mark.gpu
@pytest.mark.parametrize("row", PY_ROWS, ids=row_id)
def test_own_runs_forward_and_backward_on_the_general_kernels(switch, row, monkeypatch):
    c = case(row)
    N = row[1]
    Ho, Wo = out_hw(row)
    Fn.set_general_convolution("own")
    monkeypatch.setenv("FN2_STRICT", "1")                             # would raise at the first call that leaves the own kernels
    before = Fn.LIBRARY_FALLBACKS[0]
    x, w, b, top = call(row, c)
    top.backward(torch.tensor(c["g"], device="cuda"))
    assert Fn.LIBRARY_FALLBACKS[0] == before
    for what, got, ref, bound in (("forward", top.detach(), c["top"], 4e-6 * scale_of(c["top"])),
                                  ("data gradient", x.grad, c["gx"], 4e-6 * scale_of(c["gx"])),
                                  ("weight gradient", w.grad, c["gw"], 2e-6 * scale_of(c["gw"]) * math.sqrt(N * Ho * Wo)),
                                  ("bias gradient", b.grad, c["gb"], 2e-6 * scale_of(c["gb"]))):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print("%s %s: error %.3g, bound %.3g, ratio %.3f" % (what, row_id(row), err, bound, err / bound))
        assert got.shape == ref.shape and err <= bound, what
    assert torch.equal(call(row, c)[3], top)                          # a second call (the cached operand) gives the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("row", [ROWS[9], ROWS[14]], ids=row_id)
def test_default_counts_one_fallback_per_call_and_equals_torch_bit_for_bit(switch, row, monkeypatch):
    c = case(row)
    tr, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group = row
    Fn.set_general_convolution("library")
    monkeypatch.delenv("FN2_STRICT", raising=False)
    before = Fn.LIBRARY_FALLBACKS[0]
    x, w, b, top = call(row, c, requires_grad=False)
    assert Fn.LIBRARY_FALLBACKS[0] == before + 1
    f = F.conv_transpose2d if tr else F.conv2d
    assert torch.equal(top, f(x, w, b, stride=(sh, sw), padding=(ph, pw), dilation=(dh, dw), groups=group))
    monkeypatch.setenv("FN2_STRICT", "1")
    with pytest.raises(RuntimeError, match="FN2_STRICT=1"):
        call(row, c, requires_grad=False)


@pytest.mark.gpu
def test_the_prototxt_net_runs_forward_and_backward_on_the_general_kernels(switch, monkeypatch):
    Fn.set_general_convolution("own")
    monkeypatch.setenv("FN2_STRICT", "1")
    before = Fn.LIBRARY_FALLBACKS[0]
    gen = torch.Generator().manual_seed(3)
    x, g = torch.randn(2, 6, 11, 14, generator=gen), torch.randn(2, 8, 12, 24, generator=gen)
    net = fnet.Net(PROTOTXT, phase="TEST", device="cuda", with_backward=True)
    w1, b1, w2 = net_forward_checks(net, x)
    net.ClearParamDiffs()
    net.blobs["up"].diff = g.cuda()
    net.Backward()
    assert Fn.LIBRARY_FALLBACKS[0] == before
    conv, up = net.layer_by_name("conv"), net.layer_by_name("up")
    # the Deconvolution, at the fp32 blob the net fed it
    y1 = net.blobs["conv"].data.detach().cpu()
    a, w2g = y1.double().requires_grad_(True), w2.clone().requires_grad_(True)
    ga, gw2 = torch.autograd.grad(F.conv_transpose2d(a, w2g, None, **UP_ARGS), (a, w2g), g.double())
    g1 = net.blobs["conv"].diff.detach().cpu()
    assert close("Net deconv data gradient", g1, ga, 4e-6 * scale(ga))
    assert close("Net deconv weight gradient", up.blobs_[0].mutable_gpu_diff(), gw2, 2e-6 * scale(gw2) * math.sqrt(2 * 6 * 12))
    # the Convolution with its folded ReLU, at the fp32 diff the net fed it (the mask from the net's own activations)
    masked = g1.double() * torch.where(y1 > 0, 1.0, SLOPE).double()
    xd, w1g, b1g = x.double().requires_grad_(True), w1.clone().requires_grad_(True), b1.clone().requires_grad_(True)
    gx, gw1, gb1 = torch.autograd.grad(F.conv2d(xd, w1g, b1g, **CONV_ARGS), (xd, w1g, b1g), masked)
    assert close("Net conv data gradient", net.blobs["data"].diff, gx, 4e-6 * scale(gx))
    assert close("Net conv weight gradient", conv.blobs_[0].mutable_gpu_diff(), gw1, 2e-6 * scale(gw1) * math.sqrt(2 * 6 * 12))
    assert close("Net conv bias gradient", conv.blobs_[1].mutable_gpu_diff(), gb1, 2e-6 * scale(gb1))
    # parameter diffs accumulate: a second Backward on the same forward doubles them
    once = conv.blobs_[0].mutable_gpu_diff().clone()
    net.blobs["up"].diff = g.cuda()
    net.Backward()
    assert torch.allclose(conv.blobs_[0].mutable_gpu_diff(), 2 * once, rtol=1e-6, atol=0)
