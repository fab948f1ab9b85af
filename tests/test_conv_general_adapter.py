"""The Caffe adapter's Convolution / Deconvolution plug-ins on geometries no specialised family takes: created BY TYPE STRING through
LayerRegistry they run on the general kernels (csrc/conv_general.hip) instead of aborting, forward and all three gradients, against the
reference's own ConvolutionLayer / DeconvolutionLayer compiled in place (oracle/_ref).  Before the general kernels existed every one of
these raised RuntimeError("... has no kernel for ...") from the plug-in's Reshape."""
import numpy as np
import pytest

from conv_general_cases import CONV, DECONV, out_hw, rand, row_id
from oracle import ref

# five rows of tests/conv_general_cases.py: the two geometries the dispatchers are pinned to refuse, a ragged 4x4 / 2 convolution, and two
# deconvolutions (FlowNet's taps on 5 inputs; stride 3)
ROWS = [(False,) + CONV[5], (False,) + CONV[6], (False,) + CONV[2], (True,) + DECONV[0], (True,) + DECONV[3]]


@pytest.fixture()
def libraries():
    if not (ref.available() and ref.adapter_available()):
        pytest.skip("reference / adapter libraries not built")


def close(name, got, want):
    # fp32 sums of the same products in different orders: 1e-4 of the result's scale, the tolerance tests/test_caffe_adapter.py uses for the
    # FlowNet shapes (that of the reference's own convolution tests)
    assert got.shape == want.shape, name
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4 * max(1.0, float(np.abs(want).max())), err_msg=name)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_plugin_forward_runs_on_the_general_kernels(libraries, row):
    tr, N, Cin, H, W, Cout, k, s, p = row
    x, w, b = rand((N, Cin, H, W), 11), rand((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), 12, 0.1), rand((Cout,), 13)
    ref.use("ref")
    want = ref.convolution(x, w, b, kernel=k, stride=s, pad=p, deconv=tr)
    ref.use("adapter")
    try:
        got = ref.convolution_by_registry(x, w, b, kernel=k, stride=s, pad=p, deconv=tr)
        got_nb = ref.convolution_by_registry(x, w, None, kernel=k, stride=s, pad=p, deconv=tr)
    finally:
        ref.use("ref")
    assert want.shape == (N, Cout) + out_hw(row)
    close("top", got, want)
    close("top without bias", got_nb, want - b.reshape(1, -1, 1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_plugin_backward_runs_on_the_general_kernels_and_accumulates(libraries, row):
    tr, N, Cin, H, W, Cout, k, s, p = row
    x, w, b = rand((N, Cin, H, W), 21), rand((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), 22, 0.1), rand((Cout,), 23)
    g = rand((N, Cout) + out_hw(row), 24)
    wd0, bd0 = rand(w.shape, 25), rand(b.shape, 26)          # non-zero parameter diffs: both sides add into them (beta = 1)
    ref.use("ref")
    dx, dw, db = ref.convolution_backward(x, w, b, g, wd0, bd0, kernel=k, stride=s, pad=p, deconv=tr)
    ref.use("adapter")
    try:
        gx, gw, gb = ref.convolution_backward(x, w, b, g, wd0, bd0, kernel=k, stride=s, pad=p, deconv=tr, by_registry=True)
    finally:
        ref.use("ref")
    close("bottom_diff", gx, dx)
    close("weight_diff", gw, dw)
    close("bias_diff", gb, db)
    assert float(np.abs(gw - wd0).max()) > 1e-2 and float(np.abs(gb - bd0).max()) > 1e-2          # something was added
