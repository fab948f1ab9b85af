"""Split-bf16 ("bf16x3") arithmetic of the Correlation forward (csrc/correlation_bf16x3.hip): FN2_CONV_ARITH_BF16X3 beside FN2_CORR_ROUTE_OWN,
FN2_ROUTE_BF16X3 of fn2_correlation_route, fn2_correlation_forward_routed, functional.set_correlation_arithmetic.

Host: what the route function returns with and without the flag, the switches, the refusals that need no device.  GPU: the fp64 bound of the
exact kernels (2e-6 x scale, tests/test_gpu_parity.py) on four shapes in three output forms, three inputs whose result is exact and needs
each of the six piece products, blob forms, reproducibility (runs, batch, tile variants), refusals decided on the host, non-finite inputs,
the Python layer and the Net path, and a FlowNetC forward."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_torch64
from flownet2_amd import Fn2Error, _lib, nets, ops
from flownet2_amd._lib import check
from bf16x3_helpers import BIT, F_BF16X3, forced_variants, host
from test_conv_backward_routes import dev, rand, same_bits, scale_of

NONE, OWN = 0, 1                    # FN2_CORR_ROUTE_*
SPLIT = OWN | BIT
SENTINEL = -12345.0
FNC = (20, 1, 20, 1, 2)             # pad, kernel_size, max_displacement, stride_1, stride_2 of FlowNetC's layer
TOPC = 441
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N, C, H, W).  A k-step is 32 channels, a patch 4 x 4 class positions = 8 x 8 pixels, a task 4 or 2 neighbouring patches
SHAPES = {
    "A": (2, 32, 13, 20),           # one k-step; odd H (the last class row exists for one y parity only); every displacement hits a border; two samples
    "B": (1, 96, 24, 40),           # three k-steps (C no power of two: the true division); five patch columns: several tasks per image row
    "C": (1, 256, 16, 24),          # FlowNetC's channel count, eight k-steps
    "wide": (1, 32, 6, 136),        # 17 patch columns: a last task of one patch; H smaller than a patch row pair
}
BASELINE = [(8, 256, 40, 56), (4, 256, 48, 96), (1, 256, 56, 128), (1, 256, 16, 16)]
# (N, C, H, W, pad, K, md, s1, s2): geometries in the style of tests/test_gpu_parity.py's CORR_CASES
OTHER_GEOMETRIES = [(2, 5, 9, 11, 4, 1, 4, 1, 2), (1, 7, 8, 10, 3, 3, 2, 2, 1), (2, 3, 7, 9, 3, 1, 3, 1, 1), (1, 33, 6, 7, 2, 1, 2, 1, 1),
                    (1, 16, 13, 17, 20, 1, 20, 1, 2), (2, 64, 24, 40, 20, 1, 20, 1, 2), (1, 256, 16, 24, 20, 1, 20, 1, 2), (1, 32, 9, 30, 8, 1, 8, 1, 1),
                    (1, 32, 41, 57, 20, 1, 20, 1, 2), (1, 16, 9, 70, 21, 1, 21, 1, 2), (1, 6, 11, 13, 7, 1, 6, 1, 3), (1, 32, 12, 72, 20, 1, 20, 1, 2)]


def params(pad=20, K=1, md=20, s1=1, s2=2, ctype=ops.MULTIPLY):
    return ops.corr_params(pad, K, md, s1, s2, ctype)


def route(p, shape, flags=0):
    return int(_lib.lib().fn2_correlation_route(C.byref(p), *[int(v) for v in shape], flags))


def supported(p, shape):
    return int(_lib.lib().fn2_correlation_bf16x3_supported(C.byref(p), *[int(v) for v in shape]))


def routed(p, r, b0, b1, top, shape, top_ch=0, top_c0=0, relu=0, slope=0.0):
    """fn2_correlation_forward_routed past the Python checks; b0 / b1 / top: tensors or None (NULL)."""
    N, Cc, H, W = shape
    ptr = lambda t: None if t is None else ops._ptr(t)
    stream = ops._stream() if torch.cuda.is_available() and any(t is not None for t in (b0, b1, top)) else None
    try:
        check(_lib.lib().fn2_correlation_forward_routed(C.byref(p), int(r), ptr(b0), ptr(b1), ptr(top), N, Cc, H, W, top_ch, top_c0, relu, C.c_float(slope),
                                                        None, 0, stream))
    finally:
        if stream is not None:
            torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# host


def test_route_with_and_without_the_flag():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "flownet2_hip_corr_route.h")).read()
    for name in _lib.CORR_ROUTE_EXPORTS:
        assert hasattr(L, name) and name + "(" in hdr, name
    p = params()
    for shape in list(SHAPES.values()) + BASELINE:
        assert route(p, shape) == OWN and supported(p, shape) == 1 and route(p, shape, F_BF16X3) == SPLIT, shape
    for (N, Cc, H, W, pad, K, md, s1, s2) in OTHER_GEOMETRIES:
        for ctype in (ops.MULTIPLY, ops.SUBTRACT):
            q = params(pad, K, md, s1, s2, ctype)
            assert route(q, (N, Cc, H, W)) == OWN
            assert route(q, (N, Cc, H, W), F_BF16X3) == (SPLIT if supported(q, (N, Cc, H, W)) else OWN)
    # FlowNetC parameters alone are not enough: whole k-steps of 32 channels, whole pixel quads
    assert supported(params(), (1, 256, 16, 24)) == 1 and supported(params(), (1, 16, 13, 17)) == 0 and supported(params(), (1, 32, 41, 57)) == 0
    A = SHAPES["A"]
    stays = {"SUBTRACT": (params(ctype=ops.SUBTRACT), A), "md 4": (params(4, 1, 4, 1, 2), A), "stride_2 1": (params(s2=1), A),
             "C = 48": (params(), (2, 48, 13, 20)), "W = 22": (params(), (2, 32, 13, 22)), "kernel_size 3": (params(21, 3, 20, 1, 2), A),
             "stride_1 2": (params(s1=2), A), "pad > md": (params(22, 1, 20, 1, 2), A)}
    for what, (q, shape) in stays.items():
        assert supported(q, shape) == 0 and route(q, shape) == OWN == route(q, shape, F_BF16X3), what
    for what, q in {"even kernel": params(20, 2, 20, 1, 2), "pad < max_displacement": params(4, 1, 20, 1, 2)}.items():
        with pytest.raises(Fn2Error):
            ops.correlation_out_shape(q, A[1], A[2], A[3])
        assert route(q, A) == NONE == route(q, A, F_BF16X3) and supported(q, A) == 0, what
    # the same answer for every batch, with batch-invariant mode on or off
    was = ops.get_batch_invariant()
    try:
        for mode in (False, True):
            ops.set_batch_invariant(mode)
            for shape in list(SHAPES.values()) + BASELINE:
                for flags, want in ((0, OWN), (F_BF16X3, SPLIT)):
                    assert route(p, (1,) + shape[1:], flags) == route(p, (8,) + shape[1:], flags) == want, (shape, mode)
            assert route(stays["C = 48"][0], (8, 48, 13, 20), F_BF16X3) == OWN
    finally:
        ops.set_batch_invariant(was)
    assert ops.correlation_forward_route(p, *A) == OWN and ops.correlation_forward_route(p, *A, bf16x3=True) == SPLIT
    assert ops.correlation_forward_route(params(s2=1), *A, bf16x3=True) == OWN
    assert (ops.CORR_ROUTE_NONE, ops.CORR_ROUTE_OWN, ops.CONV_ARITH_BF16X3, ops.ROUTE_BF16X3) == (NONE, OWN, BIT, F_BF16X3)
    assert L.fn2_correlation_bf16x3_num_variants() >= 1


def test_switches_are_independent(monkeypatch):
    from flownet2_amd import functional as Fn
    assert (Fn.correlation_arithmetic(), Fn.conv_arithmetic(), Fn.deconv_arithmetic()) == ("fp32", "fp32", "fp32")
    try:
        Fn.set_correlation_arithmetic("bf16x3")
        assert (Fn.correlation_arithmetic(), Fn.conv_arithmetic(), Fn.deconv_arithmetic()) == ("bf16x3", "fp32", "fp32")
        for bad in ("bf16", "", "FP32", None):
            with pytest.raises(ValueError):
                Fn.set_correlation_arithmetic(bad)
            assert Fn.correlation_arithmetic() == "bf16x3"
        Fn.set_conv_arithmetic("bf16x3")
        Fn.set_deconv_arithmetic("bf16x3")
        Fn.set_correlation_arithmetic("fp32")
        assert (Fn.correlation_arithmetic(), Fn.conv_arithmetic(), Fn.deconv_arithmetic()) == ("fp32", "bf16x3", "bf16x3")
        Fn.set_conv_arithmetic("fp32")
        Fn.set_deconv_arithmetic("fp32")
        Fn.set_correlation_arithmetic("bf16x3")
        Fn.set_conv_arithmetic("fp32")
        assert Fn.correlation_arithmetic() == "bf16x3"
        Fn.set_correlation_arithmetic()
        assert Fn.correlation_arithmetic() == "fp32"
        # $FN2_CORR_ARITH is read where functional reads the other two, when the module is first executed: a fresh interpreter shows it
        monkeypatch.setenv("FN2_CORR_ARITH", "bf16x3")
        monkeypatch.delenv("FN2_CONV_ARITH", raising=False)
        monkeypatch.delenv("FN2_DECONV_ARITH", raising=False)
        code = "from flownet2_amd import functional as Fn; print(Fn.correlation_arithmetic(), Fn.conv_arithmetic(), Fn.deconv_arithmetic())"
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.split() == ["bf16x3", "fp32", "fp32"], out.stderr[-2000:]
        assert Fn.correlation_arithmetic() == "fp32"          # (this interpreter read its environment long ago)
    finally:
        Fn.set_correlation_arithmetic("fp32")
        Fn.set_conv_arithmetic("fp32")
        Fn.set_deconv_arithmetic("fp32")
    assert Fn.correlation_arithmetic() == "fp32"


def test_refusals_that_need_no_device():
    FN2_ERR_INVALID_ARG, FN2_ERR_UNSUPPORTED = -1, -2
    p, A = params(), SHAPES["A"]
    cases = {"0x100 alone": (p, BIT, A, FN2_ERR_INVALID_ARG), "route 2": (p, 2, A, FN2_ERR_INVALID_ARG), "route 0": (p, NONE, A, FN2_ERR_INVALID_ARG),
             "the bit on C = 48": (p, SPLIT, (2, 48, 13, 20), FN2_ERR_UNSUPPORTED), "the bit on SUBTRACT": (params(ctype=ops.SUBTRACT), SPLIT, A, FN2_ERR_UNSUPPORTED),
             "the bit on W = 22": (p, SPLIT, (2, 32, 13, 22), FN2_ERR_UNSUPPORTED), "NULL blobs, split": (p, SPLIT, A, FN2_ERR_INVALID_ARG),
             "NULL blobs, own": (p, OWN, A, FN2_ERR_INVALID_ARG), "refused parameters": (params(4, 1, 20, 1, 2), SPLIT, A, FN2_ERR_INVALID_ARG)}
    for what, (q, r, shape, status) in cases.items():
        with pytest.raises(Fn2Error) as e:
            routed(q, r, None, None, None, shape)
        assert e.value.status == status, what
    for r in (OWN, SPLIT):
        with pytest.raises(Fn2Error):          # a slice outside the top blob
            routed(p, r, None, None, None, A, top_ch=TOPC + 2, top_c0=3)
        routed(p, r, None, None, None, (0,) + A[1:])          # N == 0: FN2_OK
        routed(p, r, None, None, None, (0,) + A[1:], top_ch=TOPC + 10, top_c0=3, relu=1, slope=0.1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU

_REF = {}


def inputs(name, N=None):
    n, Cc, H, W = SHAPES[name]
    shape = (n if N is None else N, Cc, H, W)
    return rand(shape, 1), rand(shape, 2)


def ref64(name):
    """fp64 reference of inputs(name), computed once and shared."""
    if name not in _REF:
        b0, b1 = inputs(name)
        _REF[name] = ref_torch64.correlation(torch.from_numpy(b0).double(), torch.from_numpy(b1).double(), *FNC).numpy()
        _REF[name].setflags(write=False)
    return _REF[name]


def run(b0, b1, bf16x3=True, out=None, out_c0=0, relu=False, slope=0.0, p=None):
    o = None if out is None else dev(out)
    y = ops.correlation_forward(params() if p is None else p, dev(b0), dev(b1), out=o, out_c0=out_c0, relu=relu, negative_slope=slope, bf16x3=bf16x3)
    torch.cuda.synchronize()
    return host(y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp64_bound(name):
    """error / bound, worst of the three forms (measured on an MI355X; profiles/corr_bf16x3_bench.md): A 0.029, B 0.066, C 0.058, wide 0.030."""
    b0, b1 = inputs(name)
    ref = ref64(name)
    assert route(params(), SHAPES[name], F_BF16X3) == SPLIT
    for form, relu, slope in (("plain", False, 0.0), ("slice + ReLU(0.1)", True, 0.1), ("ReLU(0.0)", True, 0.0)):
        want = np.where(ref > 0, ref, ref * slope) if relu else ref
        if form.startswith("slice"):
            blob = run(b0, b1, out=np.full((ref.shape[0], TOPC + 10, ref.shape[2], ref.shape[3]), SENTINEL, np.float32), out_c0=3, relu=True, slope=slope)
            got = blob[:, 3:3 + TOPC]
        else:
            got = run(b0, b1, relu=relu, slope=slope)
        assert got.shape == want.shape
        ratio = float(np.abs(got - want).max()) / (2e-6 * scale_of(want))
        print("correlation bf16x3 fp64 error / bound: %s %s: %.3f" % (name, form, ratio))
        assert ratio <= 1.0, (name, form, ratio)


def exact_inputs(kind):
    shape = SHAPES["A"]
    N, Cc, H, W = shape
    rng = np.random.default_rng(11)
    if kind in ("select-0", "select-1"):          # one nonzero channel per pixel in one map = one term per output
        dense = rand(shape, 21)
        hot = np.zeros(shape, np.float32)
        ch = rng.integers(0, Cc, (N, H, W))
        n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
        hot[n, ch, y, x] = rng.choice([1.0, -1.0, 0.5, -2.0], (N, H, W))
        return (dense, hot) if kind == "select-0" else (hot, dense)          # select-0 needs hh, mh, lh; its mirror hh, hm, hl
    # mid-x-mid: needs mm
    b0 = (1.0 + rng.integers(0, 4, shape) / 1024.0).astype(np.float32)
    b1 = np.zeros(shape, np.float32)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                for c in rng.choice(Cc, 4, replace=False):
                    b1[n, c, y, x] = rng.choice([1.0, -1.0]) * (1.0 + rng.integers(0, 4) / 1024.0)
    return b0, b1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["select-0", "select-1", "mid-x-mid"])
def test_exact_values(kind):
    assert SHAPES["A"][1] == 32          # 1 / C is exact
    b0, b1 = exact_inputs(kind)
    ref = ref_torch64.correlation(torch.from_numpy(b0).double(), torch.from_numpy(b1).double(), *FNC).numpy()
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref) and np.abs(ref).max() > 1.0 / 64          # the reference is itself an fp32 value
    if kind == "mid-x-mid":
        assert (np.round(b0 * 1024) % 4 != 0).any() and (np.round(np.abs(b1[b1 != 0]) * 1024) % 4 != 0).any()
    got = run(b0, b1)
    assert same_bits(got + np.float32(0.0), ref32 + np.float32(0.0)), (kind, float(np.abs(got - ref32).max()))      # (+ 0.0: -0.0 == 0.0)


@pytest.mark.gpu
def test_blob_forms():
    for name in ("A", "C"):
        N, Cc, H, W = SHAPES[name]
        b0, b1 = inputs(name)
        plain = run(b0, b1)
        assert (plain < 0).any() and (plain > 0).any()
        blob = run(b0, b1, out=np.full((N, TOPC + 10, H, W), SENTINEL, np.float32), out_c0=3)
        assert (blob[:, :3] == SENTINEL).all() and (blob[:, 3 + TOPC:] == SENTINEL).all()
        assert same_bits(blob[:, 3:3 + TOPC], plain), name
        for slope in (0.1, 0.0):
            want = np.where(plain > 0, plain, plain * np.float32(slope)).astype(np.float32)
            assert same_bits(run(b0, b1, relu=True, slope=slope) + np.float32(0.0), want + np.float32(0.0)), (name, slope)
            blob = run(b0, b1, out=np.full((N, TOPC + 10, H, W), SENTINEL, np.float32), out_c0=3, relu=True, slope=slope)
            assert same_bits(blob[:, 3:3 + TOPC] + np.float32(0.0), want + np.float32(0.0)) and (blob[:, :3] == SENTINEL).all() and (blob[:, 3 + TOPC:] == SENTINEL).all()
        # route OWN of the routed entry is fn2_correlation_forward_fused
        d0, d1 = dev(b0), dev(b1)
        for (top_ch, c0, relu, slope) in ((0, 0, 0, 0.0), (TOPC + 10, 3, 1, 0.1)):
            t_routed = torch.full((N, max(top_ch, TOPC), H, W), SENTINEL, device="cuda")
            t_fused = t_routed.clone()
            routed(params(), OWN, d0, d1, t_routed, SHAPES[name], top_ch, c0, relu, slope)
            check(_lib.lib().fn2_correlation_forward_fused(C.byref(params()), ops._ptr(d0), ops._ptr(d1), ops._ptr(t_fused), N, Cc, H, W, top_ch, c0, relu,
                                                           C.c_float(slope), None, 0, ops._stream()))
            torch.cuda.synchronize()
            assert same_bits(host(t_routed), host(t_fused)) and same_bits(host(t_fused), run(b0, b1, bf16x3=False, relu=bool(relu), slope=slope,
                                                                          out=None if not top_ch else np.full((N, top_ch, H, W), SENTINEL, np.float32), out_c0=c0))
        assert not same_bits(run(b0, b1, bf16x3=False), plain)          # (another arithmetic: not the exact kernel's bits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_reproducible_across_runs_batch_and_variants(name):
    L = _lib.lib()
    b0, b1 = inputs(name, N=3)
    batch = run(b0, b1, relu=True, slope=0.1)
    assert same_bits(run(b0, b1, relu=True, slope=0.1), batch)
    assert same_bits(run(b0[:1], b1[:1], relu=True, slope=0.1), batch[:1])
    ran = 0
    with forced_variants("correlation_bf16x3") as (nv, force):
        for v in range(nv):
            force(v)
            assert same_bits(run(b0, b1, relu=True, slope=0.1), batch), v
            assert same_bits(run(b0[:1], b1[:1], relu=True, slope=0.1), batch[:1]), v
            ran += 1
        force(nv)
        with pytest.raises(Fn2Error):
            run(b0, b1, relu=True, slope=0.1)
    assert ran == nv >= 1
    assert same_bits(run(b0, b1, relu=True, slope=0.1), batch)


@pytest.mark.gpu
def test_refusals_are_decided_on_the_host():
    shape = SHAPES["A"]
    N, Cc, H, W = shape
    p = params()
    b0, b1 = dev(rand(shape, 1)), dev(rand(shape, 2))
    flat = torch.from_numpy(rand((N * Cc * H * W + 4,), 3)).cuda()
    off = flat[1:1 + N * Cc * H * W].view(shape)          # a view offset by one float
    assert off.data_ptr() % 16 == 4 and b0.data_ptr() % 16 == 0
    top = torch.full((N, TOPC + 10, H, W), SENTINEL, device="cuda")
    top_flat = torch.full((N * (TOPC + 10) * H * W + 4,), SENTINEL, device="cuda")
    top_off = top_flat[1:1 + N * (TOPC + 10) * H * W].view(top.shape)
    untouched = lambda: bool((top == SENTINEL).all()) and bool((top_flat == SENTINEL).all())
    b48 = dev(rand((N, 48, H, W), 4))
    calls = {
        "misaligned bottom0": dict(b0=off), "misaligned bottom1": dict(b1=off), "misaligned top": dict(top=top_off),
        "slice past its blob": dict(top_ch=TOPC + 2, top_c0=3), "negative top_c0": dict(top_c0=-1),
        "C = 48": dict(b0=b48, b1=b48, shape=(N, 48, H, W)), "SUBTRACT with the bit": dict(p=params(ctype=ops.SUBTRACT)),
        "null bottom0": dict(b0=None), "null bottom1": dict(b1=None), "null top": dict(top=None), "0x100 alone": dict(route=BIT), "route 2": dict(route=2),
    }
    for what, kw in calls.items():
        a = dict(p=p, route=SPLIT, b0=b0, b1=b1, top=top, shape=shape, top_ch=TOPC + 10, top_c0=3)
        a.update(kw)
        with pytest.raises(Fn2Error):
            routed(a["p"], a["route"], a["b0"], a["b1"], a["top"], a["shape"], a["top_ch"], a["top_c0"], 1, 0.1)
            pytest.fail("%s was not refused" % what)
        assert untouched(), what
    # ... and the call none of this applies to writes exactly the layer's channels
    routed(p, SPLIT, b0, b1, top, shape, TOPC + 10, 3, 1, 0.1)
    assert not bool((top[:, 3:3 + TOPC] == SENTINEL).any()) and bool((top[:, :3] == SENTINEL).all()) and bool((top[:, 3 + TOPC:] == SENTINEL).all())
    # the Python entry: a layer the split kernel does not take runs the exact path
    sub = params(ctype=ops.SUBTRACT)
    assert torch.equal(ops.correlation_forward(sub, b0, b1, bf16x3=True), ops.correlation_forward(sub, b0, b1))
    assert torch.equal(ops.correlation_forward(p, b48, b48, bf16x3=True), ops.correlation_forward(p, b48, b48))


@pytest.mark.gpu
def test_non_finite_inputs_reach_their_own_outputs_only():
    shape = (2, 32, 44, 44)
    b0, b1 = rand(shape, 1), rand(shape, 2)
    clean = run(b0, b1)
    assert np.isfinite(clean).all()
    bad0, bad1 = b0.copy(), b1.copy()
    bad0[0, 5, 21, 21] = np.inf          # both 41 x 41 displacement windows lie inside the map
    bad1[1, 17, 22, 20] = np.nan
    mask = np.zeros(clean.shape, bool)
    mask[0, :, 21, 21] = True
    for q in range(21):
        for o in range(21):
            mask[1, q * 21 + o, 22 - 2 * (q - 10), 20 - 2 * (o - 10)] = True
    assert mask.sum() == 2 * TOPC
    got = run(bad0, bad1)
    assert np.array_equal(~np.isfinite(got), mask)
    assert np.array_equal(got.view(np.uint32)[~mask], clean.view(np.uint32)[~mask])


@pytest.mark.gpu
def test_python_layer_and_net_path():
    from flownet2_amd import functional as Fn
    from flownet2_amd.layers import Blob, LayerParameter, LayerRegistry
    shape = SHAPES["A"]
    N, Cc, H, W = shape
    p = params()
    b0, b1 = dev(rand(shape, 1)), dev(rand(shape, 2))
    g = dev(rand((N, TOPC, H, W), 13))
    kw = dict(pad=20, kernel_size=1, max_displacement=20, stride_1=1, stride_2=2)
    want, exact = ops.correlation_forward(p, b0, b1, bf16x3=True), ops.correlation_forward(p, b0, b1)
    want_relu = ops.correlation_forward(p, b0, b1, relu=True, negative_slope=0.1, bf16x3=True)
    exact_relu = ops.correlation_forward(p, b0, b1, relu=True, negative_slope=0.1)
    assert not torch.equal(want, exact) and not torch.equal(want_relu, exact_relu)

    def grads():
        x0, x1 = b0.clone().requires_grad_(True), b1.clone().requires_grad_(True)
        y = Fn.correlation(x0, x1, **kw)
        assert y.requires_grad
        (y * g).sum().backward()
        return y.detach(), x0.grad.clone(), x1.grad.clone()

    def relu_into(training):
        blob = torch.full((N, TOPC + 10, H, W), SENTINEL, device="cuda")
        if training:
            x0, x1 = b0.clone().requires_grad_(True), b1.clone().requires_grad_(True)
            y = Fn.correlation_relu_into(x0, x1, blob, 3, 0.1, training=True, **kw)
            assert y.requires_grad
            (y * g).sum().backward()
            assert x0.grad is not None and x1.grad is not None
        else:
            with torch.no_grad():
                Fn.correlation_relu_into(b0, b1, blob, 3, 0.1, **kw)
        assert bool((blob[:, :3] == SENTINEL).all()) and bool((blob[:, 3 + TOPC:] == SENTINEL).all())
        return blob[:, 3:3 + TOPC].detach().clone()

    def layer(ctype="MULTIPLY"):
        l = LayerRegistry.CreateLayer(LayerParameter(type="Correlation", correlation_param=dict(correlation_type=ctype, **kw)))
        bottom, top = [Blob(*shape), Blob(*shape)], [Blob()]
        bottom[0].data, bottom[1].data = b0, b1
        l.SetUp(bottom, top)
        l.Forward(bottom, top)
        return top[0].data.clone()

    assert Fn.correlation_arithmetic() == "fp32"
    y_off, g0_off, g1_off = grads()
    assert torch.equal(y_off, exact) and torch.equal(relu_into(False), exact_relu) and torch.equal(relu_into(True), exact_relu)
    assert torch.equal(layer(), exact)
    sub_off = layer("SUBTRACT")
    Fn.set_correlation_arithmetic("bf16x3")
    try:
        with torch.no_grad():
            assert torch.equal(Fn.correlation(b0, b1, **kw), want)
        y_on, g0_on, g1_on = grads()
        assert torch.equal(y_on, want)
        assert torch.equal(g0_on, g0_off) and torch.equal(g1_on, g1_off)          # the backward is unchanged and exact
        assert torch.equal(relu_into(False), want_relu) and torch.equal(relu_into(True), want_relu)
        assert torch.equal(layer(), want)
        assert torch.equal(layer("SUBTRACT"), sub_off)
    finally:
        Fn.set_correlation_arithmetic("fp32")
    assert torch.equal(layer(), exact)


@pytest.mark.gpu
def test_flownetc_end_to_end(monkeypatch):
    from flownet2_amd import functional as Fn
    B, H, W = 1, 128, 128          # the smallest size with every layer on an own kernel (tests/test_deconv_bf16x3.py); same weights and images
    assert route(params(), (B, 256, H // 8, W // 8), F_BF16X3) == SPLIT
    conv_calls, corr_calls = [], []
    fwd, cfwd = ops.conv_forward, ops.correlation_forward

    def recorded(x, packed, bias, desc, r, transposed=False, *a, **k):
        conv_calls.append(int(r))
        return fwd(x, packed, bias, desc, r, transposed, *a, **k)

    def recorded_corr(*a, **k):
        corr_calls.append(bool(k.get("bf16x3", False)))
        return cfwd(*a, **k)

    monkeypatch.setattr(ops, "conv_forward", recorded)
    monkeypatch.setattr(ops, "correlation_forward", recorded_corr)
    P = {k: v.cuda() for k, v in nets.init_params("C", 0).items()}
    rng = np.random.default_rng(5)
    i0 = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)).cuda()
    i1 = torch.roll(i0, (2, -3), (2, 3)).contiguous()
    assert (Fn.correlation_arithmetic(), Fn.conv_arithmetic(), Fn.deconv_arithmetic()) == ("fp32", "fp32", "fp32")
    epd = lambda a, b: float(((a - b) ** 2).sum(1).sqrt().mean())
    with torch.no_grad():
        exact = nets.deploy_forward("C", P, i0, i1, Fn)
        assert corr_calls == [False] and conv_calls and not any(r & BIT for r in conv_calls)
        del conv_calls[:], corr_calls[:]
        Fn.set_correlation_arithmetic("bf16x3")
        try:
            split = nets.deploy_forward("C", P, i0, i1, Fn)
            assert corr_calls == [True] and conv_calls and not any(r & BIT for r in conv_calls)
            again = nets.deploy_forward("C", P, i0, i1, Fn)
            Fn.set_conv_arithmetic("bf16x3")
            Fn.set_deconv_arithmetic("bf16x3")
            try:
                every = nets.deploy_forward("C", P, i0, i1, Fn)
                every_again = nets.deploy_forward("C", P, i0, i1, Fn)
            finally:
                Fn.set_conv_arithmetic("fp32")
                Fn.set_deconv_arithmetic("fp32")
        finally:
            Fn.set_correlation_arithmetic("fp32")
    assert torch.equal(split, again) and torch.equal(every, every_again)
    assert any(r & BIT for r in conv_calls)
    e1, e2 = epd(split, exact), epd(every, exact)
    print("mean end-point difference vs fp32: correlation in bf16x3 %.3e px, convolutions and deconvolutions too %.3e px" % (e1, e2))
    assert np.isfinite(e1) and e1 <= 1e-4, e1
    assert np.isfinite(e2) and e2 <= 1e-4, e2
