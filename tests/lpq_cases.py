"""Inputs, cases and raw C ABI calls shared by the LpqLoss tests (tests/test_lpq_loss*.py)."""
import ctypes as C

import numpy as np

from flownet2_amd import _lib

OK, INVALID, WORKSPACE = 0, -1, -3

# (p, q, p_epsilon); q_epsilon is the proto's default 1e-2 throughout.  The last one is the 0 / 0 case of the header: p_eps == 0 with a
# p that is none of 0, 1, 2 gives NaN at every unmasked element whose difference is exactly zero.
PQ_CASES = [(2.0, 0.2, 0.0), (2.0, 0.5, 0.0), (1.0, 1.0, 0.0), (2.0, 1.0, 0.0), (1.0, 2.0, 0.0), (0.8, 0.6, 1e-3), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0),
            (0.8, 0.6, 0.0)]
Q_EPS = 1e-2
NO_POWF = [(1.0, 1.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)]          # neither power calls powf: the bits are ref32's

# name -> (shape, two bottoms, prescale, normalize, float offset of every blob inside its allocation)
# the kernel gives a thread four neighbouring pixels where H * W % 4 == 0 (16-byte loads where the pointers allow, else 4-byte loads),
# one pixel otherwise, 256 threads x at most 1024 workgroups: the two `trip2` shapes are the smallest plane counts above 1024 * 256
# units of either kind, so some threads run their grid-stride loop twice.
SHAPES = {
    "2x2x5x7": ((2, 2, 5, 7), True, False, True, 0),
    "1x1x3x3": ((1, 1, 3, 3), True, False, False, 0),
    "2x3x9x8_prescale": ((2, 3, 9, 8), True, True, True, 0),
    "one_bottom": ((2, 2, 5, 7), False, False, True, 0),
    "2x3x9x8_offset4": ((2, 3, 9, 8), True, True, False, 1),
    "2x2x5x7_offset4": ((2, 2, 5, 7), True, False, False, 1),
    "trip2_scalar": ((1, 2, 513, 513), True, False, True, 0),
    "trip2_quad": ((1, 1, 1024, 1028), True, True, True, 0),
}


def make_inputs(shape, two_bottoms, seed):
    """Differences of magnitude 1e-3 .. 30 (log-uniform, random sign), exact zeros, a NaN in one channel of a pixel and a pixel with NaN
    in every channel.  Returns float32 (b0, b1 or None)."""
    rng = np.random.default_rng(seed)
    N, Cc, H, W = shape
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(30.0), shape))
    d = (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    zeros = rng.random(shape) < 0.08
    zeros[0, 0, 0, 0] = True
    zeros[-1, :, H - 1, W - 1] = True                       # a pixel whose every channel is exactly zero
    d[zeros] = 0.0
    if two_bottoms:
        b1 = (rng.standard_normal(shape) * 5).astype(np.float32)
        b0 = (b1 + d).astype(np.float32)
        b0[zeros] = b1[zeros]
        nan_in = b1                                         # NaNs come with the ground truth
    else:
        b0, b1, nan_in = d, None, d
    nan_in[0, 0, 1, 1] = np.nan                             # one channel of a pixel (the only channel where C == 1)
    nan_in[0, :, 2, 2] = np.nan                             # every channel of a pixel
    return b0, b1


def f(x):
    return C.c_float(float(x))


def ptr(t):
    """Device (torch) tensor, ctypes buffer, int address or None -> c_void_p."""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, int):
        return C.c_void_p(t)
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(C.addressof(t))


def sizes(nscales=1):
    one, multi, sync = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert _lib.lib().fn2_lpq_loss_sizes(int(nscales), C.byref(one), C.byref(multi), C.byref(sync)) == OK
    return one.value, multi.value, sync.value


def forward(b0, b1, loss, shape, p, q, pe, qe, prescale, normalize, ws, ws_bytes, stream=None):
    return _lib.lib().fn2_lpq_loss_forward(ptr(b0), ptr(b1), ptr(loss), *[int(s) for s in shape], f(p), f(q), f(pe), f(qe), int(prescale),
                                           int(normalize), ptr(ws), int(ws_bytes), stream)


def backward(b0, b1, top_diff, d0, d1, shape, p, q, pe, qe, prescale, normalize, ws, ws_bytes, stream=None):
    return _lib.lib().fn2_lpq_loss_backward(ptr(b0), ptr(b1), f(top_diff), ptr(d0), ptr(d1), *[int(s) for s in shape], f(p), f(q), f(pe), f(qe),
                                            int(prescale), int(normalize), ptr(ws), int(ws_bytes), stream)


def ptr_array(items):
    if items is None:
        return None
    return (C.c_void_p * len(items))(*[ptr(t).value for t in items])


def forward_multi(b0s, b1s, shapes, weights, p, q, pe, qe, prescale, normalize, losses, total, ws, ws_bytes, sync, n=None, stream=None):
    n = len(shapes) if n is None else n
    flat = (C.c_int * (4 * len(shapes)))(*[int(d) for s in shapes for d in s]) if shapes is not None else None
    lw = (C.c_float * len(weights))(*[float(w) for w in weights]) if weights is not None else None
    return _lib.lib().fn2_lpq_loss_forward_multi(n, ptr_array(b0s), ptr_array(b1s), flat, lw, f(p), f(q), f(pe), f(qe), int(prescale),
                                                 int(normalize), ptr(losses), ptr(total), ptr(ws), int(ws_bytes), ptr(sync), stream)


def backward_multi(b0s, b1s, d0s, d1s, shapes, weights, p, q, pe, qe, prescale, normalize, total_diff, ws, ws_bytes, n=None, stream=None):
    n = len(shapes) if n is None else n
    flat = (C.c_int * (4 * len(shapes)))(*[int(d) for s in shapes for d in s]) if shapes is not None else None
    lw = (C.c_float * len(weights))(*[float(w) for w in weights]) if weights is not None else None
    return _lib.lib().fn2_lpq_loss_backward_multi(n, ptr_array(b0s), ptr_array(b1s), ptr_array(d0s), ptr_array(d1s), flat, lw, f(p), f(q), f(pe),
                                                  f(qe), int(prescale), int(normalize), ptr(total_diff), ptr(ws), int(ws_bytes), stream)


def refusals(b0, b1, loss, d0, d1, ws, ws_bytes, sync, losses, total):
    """(label, expected status, thunk) for every call the header says is refused on the host.  The pointers may be device tensors (the
    GPU test checks that none of them is written) or any non-null host addresses (the host test: a refusal never dereferences one)."""
    S, P = (2, 2, 5, 7), (2.0, 0.2, 0.0, 1e-2, 0, 1)
    nan = float("nan")
    out = []

    def fwd(label, want, b0_=b0, shape=S, pq=P, ws_=ws, nbytes=ws_bytes):
        out.append(("forward: " + label, want, lambda: forward(b0_, b1, loss, shape, *pq, ws_, nbytes)))

    def bwd(label, want, b0_=b0, d0_=d0, d1_=d1, shape=S, pq=P, ws_=ws, nbytes=ws_bytes):
        out.append(("backward: " + label, want, lambda: backward(b0_, b1, 0.5, d0_, d1_, shape, *pq, ws_, nbytes)))

    for add in (fwd, bwd):
        add("bottom[0] NULL", INVALID, b0_=None)
        add("N = 0", INVALID, shape=(0, 2, 5, 7))
        add("C = 0", INVALID, shape=(2, 0, 5, 7))
        add("H < 0", INVALID, shape=(2, 2, -5, 7))
        add("W = 0", INVALID, shape=(2, 2, 5, 0))
        add("2^31 elements", INVALID, shape=(1 << 15, 1 << 8, 1 << 4, 1 << 4))
        add("p NaN", INVALID, pq=(nan,) + P[1:])
        add("q NaN", INVALID, pq=P[:1] + (nan,) + P[2:])
        add("p_epsilon NaN", INVALID, pq=P[:2] + (nan,) + P[3:])
        add("p_epsilon < 0", INVALID, pq=P[:2] + (-1e-3,) + P[3:])
        add("q_epsilon NaN", INVALID, pq=P[:3] + (nan,) + P[4:])
        add("q_epsilon < 0", INVALID, pq=P[:3] + (-1e-2,) + P[4:])
        add("workspace NULL", WORKSPACE, ws_=None)
        add("workspace too small", WORKSPACE, nbytes=ws_bytes - 1)
    bwd("no diff to write", INVALID, d0_=None, d1_=None)

    _, multi_bytes, _ = sizes(2)
    shapes, weights = [S, S], [0.5, 0.25]

    def fm(label, want, n=2, b0s=(b0, b0), shapes_=shapes, weights_=weights, pq=P, ws_=ws, nbytes=multi_bytes, sync_=sync):
        out.append(("forward_multi: " + label, want, lambda: forward_multi(list(b0s) if b0s is not None else None, [b1, b1], shapes_, weights_, *pq,
                                                                          losses, total, ws_, nbytes, sync_, n=n)))

    def bm(label, want, n=2, b0s=(b0, b0), d0s=(d0, d0), d1s=(d1, d1), shapes_=shapes, weights_=weights, pq=P, ws_=ws, nbytes=multi_bytes):
        out.append(("backward_multi: " + label, want, lambda: backward_multi(list(b0s) if b0s is not None else None, [b1, b1],
                                                                            list(d0s) if d0s is not None else None,
                                                                            list(d1s) if d1s is not None else None, shapes_, weights_,
                                                                            *pq, None, ws_, nbytes, n=n)))

    for add in (fm, bm):
        add("0 scales", INVALID, n=0)
        add("9 scales", INVALID, n=9)
        add("bottoms0 NULL", INVALID, b0s=None)
        add("a bottom[0] NULL", INVALID, b0s=(b0, None))
        add("bad extent", INVALID, shapes_=[S, (2, 2, 0, 7)])
        add("2^31 elements", INVALID, shapes_=[S, (1 << 15, 1 << 8, 1 << 4, 1 << 4)])
        add("q_epsilon < 0", INVALID, pq=P[:3] + (-1.0,) + P[4:])
        add("p_epsilon NaN", INVALID, pq=P[:2] + (nan,) + P[3:])
        add("workspace NULL", WORKSPACE, ws_=None)
        add("workspace too small", WORKSPACE, nbytes=multi_bytes - 1)
    fm("sync NULL", INVALID, sync_=None)
    bm("no diff to write", INVALID, d0s=None, d1s=None)
    return out
