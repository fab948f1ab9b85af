"""The Caffe adapter's Convolution / Deconvolution plug-ins on layers with rectangular taps, dilation and groups: created BY TYPE STRING
through LayerRegistry (the test entry of csrc/caffe_adapter/geometry_shim.cpp) they run forward and all three gradients on the general
kernels (include/flownet2_hip_conv_geometry.h), against the fp64 layers of tests/conv_geometry_cases.py.  Before, every one of these
aborted in LayerSetUp ("square kernel_size required" / "dilation 1 only" / "group 1 only")."""
import ctypes as C
import os

import numpy as np
import pytest

from conv_general_cases import rand
from conv_geometry_cases import ROWS, case, out_hw, row_id

ADAPTER_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flownet2_amd", "csrc", "caffe_adapter", "_build",
                          "libfn2_caffe_adapter_test.so")
# two rectangular (conv 3x2 with strides 2x3; deconv 4x2), two dilated (conv dilation 3x1 / stride 2; deconv dilation 2), two grouped
# (conv "everything at once" with group 3; the depthwise bilinear-upsampling deconv): both layer kinds in every pair
ADAPTER_ROWS = [ROWS[1], ROWS[11], ROWS[3], ROWS[12], ROWS[9], ROWS[15]]


@pytest.fixture(scope="module")
def entry():
    if not os.path.exists(ADAPTER_SO):
        pytest.skip("adapter test library not built")
    fn = C.CDLL(ADAPTER_SO).fn2_adapter_geometry_layer
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    fn.argtypes = [C.c_int, ip, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, C.c_int, fp, fp, ip, C.c_int, fp, fp, fp, fp, fp, fp, C.c_char_p, C.c_int]
    fn.restype = C.c_int
    return fn


def ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def run(entry, row, x, w, b, g=None, wd0=None, bd0=None):
    """(top, bottom_diff, weight_diff, bias_diff) of the plug-in created by type string; the gradients only with a top diff `g`."""
    tr, N, Cin, H, W, Cout = row[:6]
    taps = (C.c_int * 9)(*row[6:15])
    shape = (C.c_int * 4)()
    err = C.create_string_buffer(1024)
    top = np.empty((N, Cout) + out_hw(row), np.float32)
    dx, dw, db = np.empty_like(x), np.empty_like(w), (np.empty_like(b) if b is not None else None)
    rc = entry(int(tr), taps, Cout, ptr(x), N, Cin, H, W, ptr(w), w.size, ptr(b), ptr(top), shape, int(g is not None), ptr(g), ptr(wd0), ptr(bd0),
               ptr(dx), ptr(dw), ptr(db), err, len(err))
    assert rc == 0, err.value.decode()
    assert tuple(shape) == top.shape                                  # the plug-in's top shape is Caffe's
    return top, dx, dw, db


def close(name, got, want):
    # 1e-4 of the result's scale: the tolerance of tests/test_conv_general_adapter.py
    assert got.shape == want.shape, name
    err, bound = float(np.abs(got.astype(np.float64) - want).max()), 1e-4 * max(1.0, float(np.abs(want).max()))
    print("%s: error %.3g, bound %.3g, ratio %.3f" % (name, err, bound, err / bound))
    assert err <= bound, name


@pytest.mark.gpu
@pytest.mark.parametrize("row", ADAPTER_ROWS, ids=row_id)
def test_plugin_forward_runs_on_the_general_kernels(entry, row):
    c = case(row)
    x, w, b = (np.array(c[k]) for k in ("x", "w", "b"))
    close("top", run(entry, row, x, w, b)[0], c["top"])
    close("top without bias", run(entry, row, x, w, None)[0], c["top_nobias"])


@pytest.mark.gpu
@pytest.mark.parametrize("row", ADAPTER_ROWS, ids=row_id)
def test_plugin_backward_runs_on_the_general_kernels_and_accumulates(entry, row):
    c = case(row)
    x, w, b, g = (np.array(c[k]) for k in ("x", "w", "b", "g"))
    wd0, bd0 = rand(w.shape, 25), rand(b.shape, 26)                  # non-zero parameter diffs: the layer adds into them (beta = 1)
    top, gx, gw, gb = run(entry, row, x, w, b, g, wd0, bd0)
    close("top", top, c["top"])
    close("bottom_diff", gx, c["gx"])
    close("weight_diff", gw, c["gw"] + wd0.astype(np.float64))
    close("bias_diff", gb, c["gb"] + bd0.astype(np.float64))
    assert float(np.abs(gw - wd0).max()) > 1e-2 and float(np.abs(gb - bd0).max()) > 1e-2          # something was added
