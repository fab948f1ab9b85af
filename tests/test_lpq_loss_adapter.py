"""The Caffe adapter's LpqLoss plug-in, created BY TYPE STRING through LayerRegistry (the test entry of csrc/caffe_adapter/lpq_shim.cpp):
the bits of the C ABI calls of include/flownet2_hip_lpq_loss.h, forward and backward, and a schedule that follows Net::set_iter."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lpq_cases as LC

pytestmark = pytest.mark.gpu

ADAPTER_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flownet2_amd", "csrc", "caffe_adapter", "_build",
                          "libfn2_caffe_adapter_test.so")
STARTS, PS, QS = [0, 3, 10], [1.0, 2.0, 0.8], [1.0, 0.2, 0.6]
TOP_DIFF = 0.5


@pytest.fixture(scope="module")
def entry():
    assert os.path.exists(ADAPTER_SO), "adapter test library not built (flownet2_amd/csrc/caffe_adapter/build_adapter.sh)"
    fn = C.CDLL(ADAPTER_SO).fn2_adapter_lpq_layer
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    fn.argtypes = [fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int, fp, C.c_int, fp, C.c_float, C.c_float, C.c_int, C.c_int,
                   C.c_int, C.c_int, C.c_float, fp, fp, fp, C.c_char_p, C.c_int]
    fn.restype = C.c_int
    return fn


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def plug_in(entry, b0, b1, starts, ps, qs, p_eps, flags, it, step=0, passes=1, expect=0):
    loss, d0 = np.empty(1, np.float32), np.empty_like(b0)
    d1 = np.empty_like(b0) if b1 is not None else None
    err = C.create_string_buffer(1024)
    rc = entry(fptr(b0), fptr(b1), *b0.shape, len(starts), (C.c_int * max(len(starts), 1))(*starts), len(ps),
               fptr(np.asarray(ps, np.float32)), len(qs), fptr(np.asarray(qs, np.float32)), p_eps, LC.Q_EPS, flags, it, step, passes, TOP_DIFF,
               fptr(loss), fptr(d0), fptr(d1), err, len(err))
    assert rc == expect, err.value.decode()
    return (loss[0], d0, d1) if rc == 0 else err.value.decode()


def c_abi(b0, b1, p, q, p_eps, flags):
    one, _, _ = LC.sizes()
    t0, t1 = torch.from_numpy(b0).cuda(), (torch.from_numpy(b1).cuda() if b1 is not None else None)
    ws, loss = torch.zeros(one, dtype=torch.uint8, device="cuda"), torch.zeros(1, device="cuda")
    d0, d1 = torch.empty_like(t0), (torch.empty_like(t0) if b1 is not None else None)
    assert LC.forward(t0, t1, loss, b0.shape, p, q, p_eps, LC.Q_EPS, flags & 1, flags & 2, ws, one) == LC.OK
    assert LC.backward(t0, t1, TOP_DIFF, d0, d1, b0.shape, p, q, p_eps, LC.Q_EPS, flags & 1, flags & 2, ws, one) == LC.OK
    torch.cuda.synchronize()
    return loss.cpu().numpy()[0], d0.cpu().numpy(), (d1.cpu().numpy() if d1 is not None else None)


def same_bits(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(np.ascontiguousarray(x, np.float32).view(np.uint32), np.ascontiguousarray(y, np.float32).view(np.uint32))


@pytest.mark.parametrize("name", ["2x2x5x7", "2x3x9x8_prescale", "one_bottom"])
def test_plug_in_gives_the_bits_of_the_c_abi(entry, name):
    shape, two, prescale, normalize, _ = LC.SHAPES[name]
    b0, b1 = LC.make_inputs(shape, two, seed=31)
    flags = int(prescale) | 2 * int(normalize)
    # constant parameters (one p, one q, no start), with a net and without one
    for it in (-1, 0, 12345):
        same_bits(plug_in(entry, b0, b1, [], [2.0], [0.2], 0.0, flags, it), c_abi(b0, b1, 2.0, 0.2, 0.0, flags))
    same_bits(plug_in(entry, b0, b1, [0], [0.8], [0.6], 1e-3, flags, 0), c_abi(b0, b1, 0.8, 0.6, 1e-3, flags))


def test_schedule_follows_set_iter(entry):
    b0, b1 = LC.make_inputs((2, 2, 5, 7), True, seed=32)
    want = {0: 0, 2: 0, 3: 1, 9: 1, 10: 2, 10 ** 6: 2}
    for it, k in want.items():
        same_bits(plug_in(entry, b0, b1, STARTS, PS, QS, 1e-3, 2, it), c_abi(b0, b1, PS[k], QS[k], 1e-3, 2))
    # without a net the layer stays at iteration 0
    same_bits(plug_in(entry, b0, b1, STARTS, PS, QS, 1e-3, 2, -1), c_abi(b0, b1, PS[0], QS[0], 1e-3, 2))
    # one layer object walked through its episodes (iterations 2, 6, 10), then one that is taken back (10, 6, 2): a pure function of iter
    same_bits(plug_in(entry, b0, b1, STARTS, PS, QS, 1e-3, 2, 2, step=4, passes=3), c_abi(b0, b1, PS[2], QS[2], 1e-3, 2))
    same_bits(plug_in(entry, b0, b1, STARTS, PS, QS, 1e-3, 2, 10, step=-4, passes=3), c_abi(b0, b1, PS[0], QS[0], 1e-3, 2))


def test_layer_setup_messages(entry):
    b0, b1 = LC.make_inputs((1, 1, 3, 3), True, seed=33)
    assert "Incompatible sizes: (pq_episode_starts_at_iter -> 2, p -> 1, q -> 1)" in plug_in(entry, b0, b1, [0, 5], [1.0], [1.0], 0.0, 0, 0, expect=-1)
    assert "Lpq schedule parameters must not be empty" in plug_in(entry, b0, b1, [], [], [], 0.0, 0, 0, expect=-1)
    assert "is not ordered or contains duplicates: 0 5 5" in plug_in(entry, b0, b1, [0, 5, 5], [1, 2, 3], [1, 2, 3], 0.0, 0, 0, expect=-1)
    assert "First entry in pq_episode_starts_at_frame is not 0" in plug_in(entry, b0, b1, [1, 5], [1, 2], [1, 2], 0.0, 0, 0, expect=-1)
