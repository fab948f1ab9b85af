"""The Caffe adapter's Convolution / Deconvolution plug-ins on blobs that are not [N, C, H, W]: created BY TYPE STRING through LayerRegistry
(the test entry of csrc/caffe_adapter/volume_shim.cpp) the two volumetric layers of tests/test_conv_volume_python.py run forward and all
three gradients on the depth tier of the general kernels (include/flownet2_hip_conv_volume.h), against fp64 conv3d / conv_transpose3d; a
layer over one spatial axis, `axis: 2` and force_nd_im2col run as the folded 2-D layer; four spatial axes are refused by name.  Before, every
one of these aborted in LayerSetUp ("libflownet2_hip runs 2D convolutions only")."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_general_cases import rand

ADAPTER_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flownet2_amd", "csrc", "caffe_adapter", "_build",
                          "libfn2_caffe_adapter_test.so")
# (deconv, bottom shape, num_output, group, kernel_size, stride, pad, dilation entries, the same call of torch)
CONV3D = (False, (2, 4, 5, 6, 7), 6, 2, (3, 2, 3), (2, 1, 1), (1, 0, 2), (1, 2, 1), dict(stride=(2, 1, 1), padding=(1, 0, 2), dilation=(1, 2, 1), groups=2))
DECONV3D = (True, (2, 6, 3, 4, 9), 4, 1, (4,), (2,), (1,), (), dict(stride=2, padding=1))


@pytest.fixture(scope="module")
def entry():
    assert os.path.exists(ADAPTER_SO), "adapter test library not built"
    fn = C.CDLL(ADAPTER_SO).fn2_adapter_volume_layer
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    fn.argtypes = [ip, fp, fp, C.c_int, fp, fp, ip, ip, ip, ip, C.c_int, fp, fp, fp, fp, fp, fp, C.c_char_p, C.c_int]
    fn.restype = C.c_int
    return fn


def ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def run(entry, deconv, x, w, b, num_output, group, kernel, stride, pad, dilation, top_shape, axis=1, force_nd=False, g=None, wd0=None, bd0=None):
    """(top, bottom_diff, weight_diff, bias_diff) of the plug-in created by type string; the gradients only with a top diff `g`.  Raises
    RuntimeError with the plug-in's message where it refuses."""
    desc = [int(deconv), num_output, group, axis, int(force_nd), x.ndim, len(kernel), len(stride), len(pad), len(dilation)]
    desc += list(x.shape) + list(kernel) + list(stride) + list(pad) + list(dilation)
    layer = (C.c_int * len(desc))(*desc)
    shape, axes, wshape, waxes = (C.c_int * 8)(), C.c_int(), (C.c_int * 8)(), C.c_int()
    err = C.create_string_buffer(1024)
    top = np.empty(top_shape, np.float32)
    dx, dw, db = np.empty_like(x), np.empty_like(w), (np.empty_like(b) if b is not None else None)
    rc = entry(layer, ptr(x), ptr(w), w.size, ptr(b), ptr(top), shape, C.byref(axes), wshape, C.byref(waxes), int(g is not None), ptr(g), ptr(wd0),
               ptr(bd0), ptr(dx), ptr(dw), ptr(db), err, len(err))
    if rc != 0:
        raise RuntimeError(err.value.decode())
    assert tuple(shape[:axes.value]) == tuple(top_shape)             # the plug-in's top shape is Caffe's
    assert tuple(wshape[:waxes.value]) == w.shape                     # and its weight blob
    return top, dx, dw, db


def close(name, got, want):
    # 1e-4 of the result's scale: the tolerance of tests/test_conv_general_adapter.py and tests/test_conv_geometry_adapter.py
    assert got.shape == want.shape, name
    err, bound = float(np.abs(got.astype(np.float64) - want).max()), 1e-4 * max(1.0, float(np.abs(want).max()))
    print("%s: error %.3g, bound %.3g, ratio %.3f" % (name, err, bound, err / bound))
    assert err <= bound, name


def reference(f, x, w, b, g, args):
    xt, wt, bt = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, b))
    top = f(xt, wt, bt, **args)
    gx, gw, gb = torch.autograd.grad(top, (xt, wt, bt), torch.from_numpy(g(tuple(top.shape))).double())
    return top.detach().numpy(), gx.numpy(), gw.numpy(), gb.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("layer", [CONV3D, DECONV3D], ids=["conv3d", "deconv3d"])
def test_volumetric_plugins_run_three_passes_on_the_depth_kernels_and_accumulate(entry, layer):
    deconv, shape, num_output, group, kernel, stride, pad, dilation, args = layer
    x, b = rand(shape, 1), rand((num_output,), 3)
    k3 = kernel * 3 if len(kernel) == 1 else kernel
    w = rand(((shape[1], num_output // group) if deconv else (num_output, shape[1] // group)) + tuple(k3), 2, 0.1)
    made = {}
    top, gx, gw, gb = reference(F.conv_transpose3d if deconv else F.conv3d, x, w, b, lambda s: made.setdefault("g", rand(s, 4)), args)
    g = made["g"]
    close("top", run(entry, deconv, x, w, b, num_output, group, kernel, stride, pad, dilation, top.shape)[0], top)
    close("top without bias", run(entry, deconv, x, w, None, num_output, group, kernel, stride, pad, dilation, top.shape)[0],
          top - b.astype(np.float64).reshape(1, -1, 1, 1, 1))
    wd0, bd0 = rand(w.shape, 25), rand(b.shape, 26)                  # non-zero parameter diffs: the layer adds into them (beta = 1)
    t, dx, dw, db = run(entry, deconv, x, w, b, num_output, group, kernel, stride, pad, dilation, top.shape, g=g, wd0=wd0, bd0=bd0)
    close("top", t, top)
    close("bottom_diff", dx, gx)
    close("weight_diff", dw, gw + wd0.astype(np.float64))
    close("bias_diff", db, gb + bd0.astype(np.float64))
    assert float(np.abs(dw - wd0).max()) > 1e-2 and float(np.abs(db - bd0).max()) > 1e-2          # something was added


@pytest.mark.gpu
def test_axis_one_spatial_axis_and_force_nd_im2col_run_as_the_folded_layer(entry):
    # axis: 2 on [2, 3, 4, 9, 8]: the plain 3x3 / 2 / 1 layer on the [6, 4, 9, 8] view, bit for bit, with and without force_nd_im2col
    x, w, b = rand((2, 3, 4, 9, 8), 1), rand((6, 4, 3, 3), 2, 0.1), rand((6,), 3)
    g = rand((2, 3, 6, 5, 4), 4)
    wd0, bd0 = np.zeros_like(w), np.zeros_like(b)
    deep = run(entry, False, x, w, b, 6, 1, (3,), (2,), (1,), (), (2, 3, 6, 5, 4), axis=2, g=g, wd0=wd0, bd0=bd0)
    flat = run(entry, False, x.reshape(6, 4, 9, 8), w, b, 6, 1, (3,), (2,), (1,), (), (6, 6, 5, 4), g=g.reshape(6, 6, 5, 4), wd0=wd0, bd0=bd0)
    forced = run(entry, False, x.reshape(6, 4, 9, 8), w, b, 6, 1, (3,), (2,), (1,), (), (6, 6, 5, 4), force_nd=True, g=g.reshape(6, 6, 5, 4), wd0=wd0, bd0=bd0)
    for a, v, f in zip(deep, flat, forced):
        assert np.array_equal(a.reshape(v.shape), v) and np.array_equal(f, v)
    ref = reference(F.conv2d, x.reshape(6, 4, 9, 8), w, b, lambda s: g.reshape(s), dict(stride=2, padding=1))
    for name, got, want in zip(("top", "bottom_diff", "weight_diff", "bias_diff"), flat, ref):
        close("axis: 2 " + name, got, want)
    # one spatial axis, [N, C, L]: weight blob [num_output, C / group, k]
    x, w, b = rand((2, 6, 37), 1), rand((10, 3, 7), 2, 0.1), rand((10,), 3)
    made = {}
    ref = reference(F.conv1d, x, w, b, lambda s: made.setdefault("g", rand(s, 4)), dict(stride=2, padding=3, dilation=2, groups=2))
    got = run(entry, False, x, w, b, 10, 2, (7,), (2,), (3,), (2,), (2, 10, 16), g=made["g"], wd0=np.zeros_like(w), bd0=np.zeros_like(b))
    for name, a, want in zip(("top", "bottom_diff", "weight_diff", "bias_diff"), got, ref):
        close("1-axis " + name, a, want)
    # no spatial axis, [N, C]: an inner product
    x, w, b = rand((3, 5), 1), rand((7, 5), 2, 0.1), rand((7,), 3)
    top = run(entry, False, x, w, b, 7, 1, (1,), (), (), (), (3, 7))[0]
    close("0-axis top", top, x.astype(np.float64) @ w.astype(np.float64).T + b)


@pytest.mark.gpu
def test_the_plugin_refuses_four_spatial_axes_and_h_w_fields_by_name(entry):
    x, w, b = rand((1, 2, 3, 3, 3, 3), 1), rand((2, 2, 1, 1, 1, 1), 2), rand((2,), 3)
    with pytest.raises(RuntimeError, match="0 to 3 spatial axes; 4 were asked for"):
        run(entry, False, x, w, b, 2, 1, (1,), (), (), (), (1, 2, 3, 3, 3, 3))
    x, w = rand((1, 2, 3, 3, 3), 1), rand((2, 2, 1, 1, 1), 2)
    with pytest.raises(RuntimeError, match=r"kernel_size must be specified once, or once per spatial dimension \(kernel_size specified 2 times; 3 spatial dims\)"):
        run(entry, False, x, w, b, 2, 1, (1, 1), (), (), (), (1, 2, 3, 3, 3))
