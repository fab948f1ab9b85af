"""Split-bf16 ("bf16x3") arithmetic of the 5x5 / 2 / 2 weight gradient (csrc/conv_wgrad_bf16x3.hip): fn2_conv_backward_weights_arith,
fn2_conv_backward_weights_arith_run, functional.set_conv_weight_gradient_arithmetic.

Host: which layers get the arithmetic bit with and without the flag, the workspace sizes, the refused classes, the switch.  GPU: the fp64
bound of the exact weight gradient (2e-6 x scale x sqrt(N Ht Wt)) on five shapes, accumulate, three inputs whose result is exact and needs
each of the six piece products, reproducibility (runs, tile variants), non-finite inputs, refusals decided on the host, the Python layer,
and a small FlowNetC training step against the branch-pinned fp64 graph.

Measured on an MI355X, error / bound of test_fp64_bound (split, exact kernel on the same inputs): A 0.006, 0.005; B 0.008, 0.006; C 0.003, 0.003; D 0.015, 0.010; wide 0.015, 0.013."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from flownet2_amd import Fn2Error, _lib, nets, ops
from flownet2_amd._lib import check
from bf16x3_helpers import BIT, F_BF16X3, F_FORCE, forced_variants, host
from test_conv_backward_routes import dev, flownetc_training_layers, rand, same_bits, scale_of

SENTINEL = np.float32(-7.25)
CHUNK = 8                           # pixels of a row per chunk (= per k-step), every tile variant
# convolution descriptors (N, Cin, H, W, Cout), all 5x5 / 2 / 2; a = top_diff [N, Cout, Ht, Wt], b = bottom [N, Cin, H, W]
SHAPES = {
    "A": (2, 64, 16, 24, 96),       # 8 x 12: 1.5 `a` blocks of 64 channels; K parts that cross the sample boundary; rows of 1.5 chunks
    "B": (1, 40, 17, 32, 64),       # 9 x 16: odd bottom height; a ragged `b` block of 40 channels
    "C": (3, 64, 24, 32, 128),      # 12 x 16: 576 pixels of K; N = 3, so the parts divide unevenly
    "D": (1, 32, 9, 8, 16),         # 5 x 4: `a` rows of 4 pixels (half a k-group of 8); a quarter `a` block
    "wide": (1, 32, 9, 136, 64),    # 5 x 68: rows wider than two chunks and not a multiple of the chunk
}


def desc(name, N=None):
    n, Cin, H, W, Cout = SHAPES[name]
    return ops.conv_desc(n if N is None else N, Cin, H, W, Cout, 5, 2, 2)


def top_hw(name):
    _, _, H, W, _ = SHAPES[name]
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def arith_of(d, tr=0, flags=F_BF16X3):
    return int(_lib.lib().fn2_conv_backward_weights_arith(C.byref(d), int(tr), flags))


def ws_bytes(d, tr, arith):
    return int(_lib.lib().fn2_conv_backward_weights_workspace_bytes_arith(C.byref(d), int(tr), arith))


def supported(d, tr=0):
    return int(_lib.lib().fn2_conv_wgrad_bf16x3_supported(C.byref(d), int(tr)))


def ksplit(d):
    return int(_lib.lib().fn2_conv_wgrad_bf16x3_ksplit(C.byref(d), 0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# host


def test_arith_flag_gives_the_bit_to_conv2_and_conv3_only():
    layers = flownetc_training_layers()                       # batch 8 @448x320
    was = ops.get_batch_invariant()
    try:
        for inv in (False, True):
            ops.set_batch_invariant(inv)
            took = set()
            for (name, kind, n, ci, h, w, co, k, s, p) in layers:
                d, tr = ops.conv_desc(n, ci, h, w, co, k, s, p), int(kind == "deconv")
                assert arith_of(d, tr, 0) == 0 and arith_of(d, tr, F_FORCE) == 0, name          # flags 0; FN2_ROUTE_FORCE means nothing here
                assert arith_of(d, 1, F_BF16X3) == 0, name                                        # every transposed layer
                got = arith_of(d, tr, F_BF16X3)
                assert got in (0, BIT) and got == arith_of(d, tr, F_BF16X3 | F_FORCE), name
                assert bool(got) == bool(supported(d, tr)) or not ops.conv_backward_weights_supported(d, tr), name
                if got:
                    took.add(name)
                    assert (k, s, p, tr) == (5, 2, 2, 0)
            assert took == {"conv2", "conv3"}, (took, inv)
            for s in SHAPES:
                assert {arith_of(desc(s, N=n)) for n in (1, 2, 3, 8, 64)} == {BIT}, (s, inv)
                assert arith_of(desc(s), 0, 0) == 0 and arith_of(desc(s), 1) == 0, (s, inv)
    finally:
        ops.set_batch_invariant(was)
    assert ops.conv_backward_weights_arith(desc("A"), False, bf16x3=True) == BIT
    assert ops.conv_backward_weights_arith(desc("A"), False) == 0 and ops.conv_backward_weights_arith(desc("A"), True, bf16x3=True) == 0


def test_workspace_sizes_and_refused_classes():
    L = _lib.lib()
    for (name, kind, n, ci, h, w, co, k, s, p) in flownetc_training_layers():
        d, tr = ops.conv_desc(n, ci, h, w, co, k, s, p), int(kind == "deconv")
        assert ws_bytes(d, tr, 0) == int(L.fn2_conv_backward_weights_workspace_bytes(C.byref(d), tr)), name       # arith 0: the existing value
        if arith_of(d, tr):
            assert ws_bytes(d, tr, BIT) > 0, name
        else:
            assert ws_bytes(d, tr, BIT) == 0, name                # a refused layer with the bit
        assert ws_bytes(d, tr, 0x200) == 0 and ws_bytes(d, tr, BIT | 1) == 0, name
    for s in SHAPES:
        d = desc(s)
        assert ws_bytes(d, 0, 0) == int(L.fn2_conv_backward_weights_workspace_bytes(C.byref(d), 0)) > 0, s
        assert ws_bytes(d, 0, BIT) > 0 and ws_bytes(d, 1, BIT) == 0, s
    refused = {
        "3x3 / 2": ops.conv_desc(2, 64, 16, 24, 96, 3, 2, 1), "4x4 / 2": ops.conv_desc(2, 64, 16, 24, 96, 4, 2, 1),
        "1x1": ops.conv_desc(2, 64, 16, 24, 96, 1, 1, 0), "pad 1": ops.conv_desc(2, 64, 16, 24, 96, 5, 2, 1),
        "Wa % 4 != 0": ops.conv_desc(2, 64, 16, 20, 96, 5, 2, 2), "Wb % 4 != 0": ops.conv_desc(2, 64, 16, 22, 96, 5, 2, 2),
        "stride 1": ops.conv_desc(2, 64, 16, 24, 96, 5, 1, 2), "fewer than 16 channels": ops.conv_desc(2, 64, 16, 24, 2, 5, 2, 2),
    }
    for what, d in refused.items():
        assert supported(d) == 0 and arith_of(d) == 0 and ws_bytes(d, 0, BIT) == 0 and ksplit(d) == 0, what
    assert supported(desc("A"), 1) == 0 and L.fn2_conv_wgrad_bf16x3_supported(None, 0) == 0
    assert L.fn2_conv_wgrad_bf16x3_num_variants() >= 2
    # the K split is the kernel's own function of the geometry: more than one part at A and C
    assert ksplit(desc("A")) > 1 and ksplit(desc("C")) > 1
    Wt = top_hw("wide")[1]
    assert Wt > 2 * CHUNK and Wt % CHUNK != 0


def test_switch_is_its_own_and_reads_the_environment():
    import os
    import subprocess
    import sys
    from flownet2_amd import functional as Fn
    assert Fn.conv_weight_gradient_arithmetic() == "fp32"
    try:
        Fn.set_conv_weight_gradient_arithmetic("bf16x3")
        assert Fn.conv_weight_gradient_arithmetic() == "bf16x3" and Fn.conv_backward_arithmetic() == "fp32" and Fn.conv_arithmetic() == "fp32"
        assert Fn.deconv_arithmetic() == "fp32"
        assert Fn.arithmetic("wgrad") == Fn.conv_weight_gradient_arithmetic() and Fn.winograd_arithmetic() == Fn.get_winograd_arithmetic() == "fp32"
        with pytest.raises(ValueError):
            Fn.set_conv_weight_gradient_arithmetic("bf16")
        assert Fn.conv_weight_gradient_arithmetic() == "bf16x3"
    finally:
        Fn.set_conv_weight_gradient_arithmetic("fp32")
    Fn.set_conv_backward_arithmetic("bf16x3")
    try:
        assert Fn.conv_weight_gradient_arithmetic() == "fp32"
    finally:
        Fn.set_conv_backward_arithmetic("fp32")
    code = "from flownet2_amd import functional as Fn; print(Fn.conv_weight_gradient_arithmetic(), Fn.conv_backward_arithmetic(), Fn.conv_arithmetic())"
    env = dict(os.environ, FN2_WGRAD_ARITH="bf16x3")
    env.pop("FN2_CONV_ARITH", None)
    env.pop("FN2_DGRAD_ARITH", None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["bf16x3", "fp32", "fp32"], (out.stdout, out.stderr)
    env["FN2_WGRAD_ARITH"] = "bf16"
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True)
    assert out.returncode != 0 and "ValueError" in out.stderr


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU

B_C0, A_C0 = 3, 4                   # bottom: channels [3, 3 + Cin) of a blob of Cin + 5; top_diff: [4, 4 + Cout) of Cout + 6


@functools.lru_cache(maxsize=None)
def inputs(name, N=None):
    """(bottom blob, top_diff blob), shared: not written to"""
    n, Cin, H, W, Cout = SHAPES[name]
    n = n if N is None else N
    Ht, Wt = top_hw(name)
    xb, gb = rand((n, Cin + 5, H, W), 1), rand((n, Cout + 6, Ht, Wt), 2)
    return xb, gb


def ref64(x, g):
    """weight_diff in float64 on the CPU, as test_weight_gradient builds it: x = bottom [N, Cin, H, W], g = top_diff [N, Cout, Ht, Wt]"""
    x64, g64 = torch.from_numpy(np.ascontiguousarray(x)).double(), torch.from_numpy(np.ascontiguousarray(g)).double()
    wshape = (g.shape[1], x.shape[1], 5, 5)
    return torch.ops.aten.convolution_backward(g64, x64, torch.zeros(wshape, dtype=torch.float64), None, [2, 2], [2, 2], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1].numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    n, Cin, H, W, Cout = SHAPES[name]
    xb, gb = inputs(name)
    ref = ref64(xb[:, B_C0:B_C0 + Cin], gb[:, A_C0:A_C0 + Cout])
    return ref


def guarded(a):
    """a on the device at the start of an allocation five times its size (test_conv_backward_routes.guarded)"""
    buf = torch.zeros(5 * a.size, device="cuda")
    buf[:a.size] = dev(a.reshape(-1))
    return buf[:a.size].view(a.shape)


def run(name, xb, gb, N=None, bf16x3=True, **kw):
    """the ops wrapper on channel slices of wider blobs, inside over-allocations"""
    return host(ops.conv_backward_weights(guarded(xb), guarded(gb), desc(name, N), False, bottom_c0=B_C0, top_c0=A_C0, bf16x3=bf16x3, **kw))


def run_whole(name, x, g, N=None, bf16x3=True):
    """whole blobs"""
    return host(ops.conv_backward_weights(dev(x), dev(g), desc(name, N), False, bf16x3=bf16x3))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp64_bound(name):
    """error / bound, measured on an MI355X (split, exact kernel on the same inputs): A 0.006, 0.005; B 0.008, 0.006; C 0.003, 0.003; D 0.015, 0.010; wide 0.015, 0.013."""
    n, Cin, H, W, Cout = SHAPES[name]
    Ht, Wt = top_hw(name)
    assert arith_of(desc(name)) == BIT
    xb, gb = inputs(name)
    ref = reference(name)
    bound = 2e-6 * scale_of(ref) * np.sqrt(n * Ht * Wt)
    got = run(name, xb, gb)
    exact = run(name, xb, gb, bf16x3=False)
    assert got.shape == ref.shape
    ratio = float(np.abs(got - ref).max()) / bound
    print("wgrad bf16x3 fp64 error / bound: %s split: %.3f" % (name, ratio))
    print("wgrad bf16x3 fp64 error / bound: %s exact: %.3f" % (name, float(np.abs(exact - ref).max()) / bound))
    assert ratio <= 1.0, (name, ratio)
    assert not same_bits(got, exact)                            # the flag does reach another kernel


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_accumulate(name):
    xb, gb = inputs(name)
    got = run(name, xb, gb)
    start = rand(got.shape, 3)
    acc = run(name, xb, gb, out=dev(start), accumulate=True)
    assert same_bits(acc, start + got)
    assert same_bits(run(name, xb, gb, out=dev(start), accumulate=False), got)


def exact_inputs(kind):
    """(bottom, top_diff) at shape A with N = 1 whose weight gradient is an fp32 number"""
    _, Cin, H, W, Cout = SHAPES["A"]
    Ht, Wt = top_hw("A")
    rng = np.random.default_rng(11)
    if kind == "b-one-hot":         # needs hh, mh, lh: one nonzero bottom pixel per channel, a signed power of two
        g = rand((1, Cout, Ht, Wt), 21)
        x = np.zeros((1, Cin, H, W), np.float32)
        x[0, np.arange(Cin), rng.integers(0, H, Cin), rng.integers(0, W, Cin)] = rng.choice([1.0, -1.0, 0.5, -2.0], Cin)
        return x, g
    if kind == "a-one-hot":         # needs hh, hm, hl
        x = rand((1, Cin, H, W), 22)
        g = np.zeros((1, Cout, Ht, Wt), np.float32)
        g[0, np.arange(Cout), rng.integers(0, Ht, Cout), rng.integers(0, Wt, Cout)] = rng.choice([1.0, -1.0, 2.0, -0.5], Cout)
        return x, g
    # mid-x-mid: needs mm.  1 + i / 1024 = h + m with h = 1, m = i / 1024; every sum is at most four products below 8 on a 2^-20 grid
    g = (1.0 + rng.integers(0, 4, (1, Cout, Ht, Wt)) / 1024.0).astype(np.float32)
    x = np.zeros((1, Cin, H, W), np.float32)
    for cb in range(Cin):
        for f in rng.choice(H * W, 4, replace=False):
            x[0, cb].reshape(-1)[f] = rng.choice([1.0, -1.0]) * (1.0 + rng.integers(0, 4) / 1024.0)
    return x, g


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["b-one-hot", "a-one-hot", "mid-x-mid"])
def test_exact_values(kind):
    x, g = exact_inputs(kind)
    ref = ref64(x, g)
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref) and np.abs(ref).max() > 0.5          # the reference is itself an fp32 value
    if kind == "mid-x-mid":
        assert (np.round(g * 1024) % 4 != 0).any() and (np.round(np.abs(x[x != 0]) * 1024) % 4 != 0).any() and np.abs(ref).max() < 8
    got = run_whole("A", x, g, N=1)
    assert same_bits(got + np.float32(0.0), ref32 + np.float32(0.0)), (kind, float(np.abs(got - ref32).max()))      # (+ 0.0: -0.0 == 0.0)


def raw(d, arith, x, x_ch, x_c0, g, g_ch, g_c0, dw, ws, ws_bytes_, accumulate=0, tr=0, null=()):
    ptr = {"x": ops._ptr(x), "g": ops._ptr(g), "dw": ops._ptr(dw), "ws": ops._ptr(ws)}
    for n in null:
        ptr[n] = None
    try:
        check(_lib.lib().fn2_conv_backward_weights_arith_run(C.byref(d), int(tr), int(arith), ptr["x"], x_ch, x_c0, ptr["g"], g_ch, g_c0, ptr["dw"],
                                                             accumulate, ptr["ws"], ws_bytes_, ops._stream()))
    finally:
        torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_reproducible_across_runs_and_variants(name):
    L = _lib.lib()
    n, Cin, H, W, Cout = SHAPES[name]
    xb, gb = inputs(name)
    base = run(name, xb, gb)
    assert same_bits(run(name, xb, gb), base)
    assert same_bits(run_whole(name, xb[:, B_C0:B_C0 + Cin], gb[:, A_C0:A_C0 + Cout]), base)          # whole blobs: the same bits
    ran = 0
    with forced_variants("conv_wgrad_bf16x3") as (nv, force):
        for v in range(nv):
            force(v)
            assert same_bits(run(name, xb, gb), base), v
            ran += 1
        force(nv)                  # one past the last
        dw = torch.full((Cout, Cin, 5, 5), float(SENTINEL), device="cuda")
        with pytest.raises(Fn2Error):
            ops.conv_backward_weights(dev(xb), dev(gb), desc(name), False, out=dw, bottom_c0=B_C0, top_c0=A_C0, bf16x3=True)
        torch.cuda.synchronize()
        assert bool((dw == float(SENTINEL)).all())
    assert ran == nv >= 2
    assert same_bits(run(name, xb, gb), base)


def non_finite_case(name, N, a_spot, b_spot):
    """Inf at a_spot = (n, ca, y, x) of top_diff, NaN at b_spot = (n, cb, Y, X) of bottom: exactly their own weight elements are non-finite"""
    _, Cin, H, W, Cout = SHAPES[name]
    Ht, Wt = top_hw(name)
    xb, gb = inputs(name, N)
    x, g = xb[:, B_C0:B_C0 + Cin].copy(), gb[:, A_C0:A_C0 + Cout].copy()
    assert (g != 0).all() and (x != 0).all()
    clean = run_whole(name, x, g, N=N)
    assert np.isfinite(clean).all()
    want = np.zeros(clean.shape, bool)
    (n, ca0, y, xx) = a_spot
    g[n, ca0, y, xx] = np.inf
    want[ca0] = True
    (n, cb0, Y, X) = b_spot
    x[n, cb0, Y, X] = np.nan
    taps = 0
    for ky in range(5):
        for kx in range(5):
            if (Y + 2 - ky) % 2 == 0 and (X + 2 - kx) % 2 == 0 and 0 <= (Y + 2 - ky) // 2 < Ht and 0 <= (X + 2 - kx) // 2 < Wt:
                want[:, cb0, ky, kx] = True
                taps += 1
    got = run_whole(name, x, g, N=N)
    assert np.array_equal(~np.isfinite(got), want), (name, taps, int((~np.isfinite(got)).sum()), int(want.sum()))
    assert np.array_equal(got.view(np.uint32)[~want], clean.view(np.uint32)[~want])
    return taps


@pytest.mark.gpu
def test_non_finite_inputs_reach_their_own_elements_only():
    """Shape B with N = 2: the NaN in channel 37 of the ragged `b` block, in the last bottom row (16 = 2 Ha - 2: the tap ky = 0 would need
    the row y = 9 beyond `a`; row 8 of sample 1 is a chunk of one valid row) and an inner column.  And shape A (rows of 12 = 1.5 chunks):
    the NaN in column Wb - 2, which the taps kx = 0 would meet at the padding pixel x = Wa of the last x block."""
    _, Cin, H, W, Cout = SHAPES["B"]
    assert (H, W) == (17, 32)
    assert non_finite_case("B", 2, (0, 5, 3, 7), (1, 37, 16, 13)) == 2 * 2           # ky in {2, 4} (ky = 0: y = 9 = Ha, outside); kx in {1, 3}
    _, Cin, H, W, Cout = SHAPES["A"]
    assert (H, W) == (16, 24)
    assert non_finite_case("A", 2, (1, 70, 7, 11), (0, 9, 8, 22)) == 3 * 2           # ky in {0, 2, 4}; kx in {2, 4} (kx = 0: x = 12 = Wa, outside)


@pytest.mark.gpu
def test_refusals_are_decided_on_the_host():
    N, Cin, H, W, Cout = SHAPES["A"]
    Ht, Wt = top_hw("A")
    d = desc("A")
    x, g = dev(rand((N, Cin + 5, H, W), 1)), dev(rand((N, Cout + 6, Ht, Wt), 2))
    dw = torch.full((Cout, Cin, 5, 5), float(SENTINEL), device="cuda")
    need = ws_bytes(d, 0, BIT)
    ws = torch.empty(need // 4 + 16, device="cuda")
    untouched = lambda: bool((dw == float(SENTINEL)).all())
    d3 = ops.conv_desc(N, Cin, H, W, Cout, 3, 2, 1)           # bottom and top_diff of the same sizes
    assert ((H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1) == (Ht, Wt) and ops.conv_backward_weights_supported(d3, False)
    calls = {
        "the bit on a 3x3 / 2 descriptor": dict(d=d3), "the bit on a transposed descriptor": dict(tr=1),
        "an unknown bit": dict(arith=0x200), "the bit and another": dict(arith=BIT | 0x200), "the bit and a low one": dict(arith=BIT | 1),
        "null bottom": dict(null=("x",)), "null top_diff": dict(null=("g",)), "null weight_diff": dict(null=("dw",)),
        "null workspace": dict(null=("ws",)),
        "bottom slice past its blob": dict(x_ch=Cin + 2, x_c0=3), "top_diff slice past its blob": dict(g_ch=Cout + 3, g_c0=4),
        "negative bottom slice": dict(x_c0=-1), "negative top_diff slice": dict(g_c0=-1),
        "a workspace one byte short": dict(ws_bytes=need - 1),
    }
    for what, kw in calls.items():
        a = dict(d=d, tr=0, arith=BIT, x_ch=Cin + 5, x_c0=B_C0, g_ch=Cout + 6, g_c0=A_C0, ws_bytes=need, null=())
        a.update(kw)
        with pytest.raises(Fn2Error):
            raw(a["d"], a["arith"], x, a["x_ch"], a["x_c0"], g, a["g_ch"], a["g_c0"], dw, ws, a["ws_bytes"], tr=a["tr"], null=a["null"])
            pytest.fail("%s was not refused" % what)
        assert untouched(), what
    # ... and the call none of this applies to writes the layer's gradient; arith 0 is fn2_conv_backward_weights
    raw(d, BIT, x, Cin + 5, B_C0, g, Cout + 6, A_C0, dw, ws, need)
    assert not bool((dw == float(SENTINEL)).any())
    assert torch.equal(dw, ops.conv_backward_weights(x, g, d, False, bottom_c0=B_C0, top_c0=A_C0, bf16x3=True))
    need0 = ws_bytes(d, 0, 0)
    ws0 = torch.empty(need0 // 4 + 16, device="cuda")
    raw(d, 0, x, Cin + 5, B_C0, g, Cout + 6, A_C0, dw, ws0, need0)
    assert torch.equal(dw, ops.conv_backward_weights(x, g, d, False, bottom_c0=B_C0, top_c0=A_C0))
    # the ops wrapper with bf16x3 on a layer the kernel does not take: the exact kernel
    x3 = ops.conv_backward_weights(x, g, d3, False, bottom_c0=B_C0, top_c0=A_C0, bf16x3=True)
    assert torch.equal(x3, ops.conv_backward_weights(x, g, d3, False, bottom_c0=B_C0, top_c0=A_C0))


@pytest.mark.gpu
def test_python_layer(monkeypatch):
    from flownet2_amd import functional as Fn
    monkeypatch.delenv("FN2_STRICT", raising=False)
    N, Cin, H, W, Cout = 2, 64, 16, 24, 128
    Ht, Wt = 8, 12
    d = ops.conv_desc(N, Cin, H, W, Cout, 5, 2, 2)
    assert arith_of(d) == BIT
    w, b = dev(rand((Cout, Cin, 5, 5), 2, 0.1)), dev(rand((Cout,), 3, 0.1))
    wide = dev(rand((N, Cin + 5, H, W), 9))
    x = wide[:, 2:2 + Cin]
    g = dev(rand((N, Cout, Ht, Wt), 13))

    def grads():
        xg, wg, bg = x.detach().clone().requires_grad_(True), torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
        y = Fn.conv_mfma_relu(xg, wg, bg, 2, 2, 0.1, True)
        (y * g).sum().backward()
        return y.detach(), xg.grad.clone(), wg.grad.clone(), bg.grad.clone()

    assert Fn.conv_weight_gradient_arithmetic() == "fp32" and Fn.conv_backward_arithmetic() == "fp32" and Fn.conv_arithmetic() == "fp32"
    before = Fn.LIBRARY_FALLBACKS[0]
    y_off, gx_off, gw_off, gb_off = grads()
    off_fallbacks = Fn.LIBRARY_FALLBACKS[0] - before
    # the weight gradient by hand: ReLUBackward of this layer's own activation, then the kernels called directly
    td = (g * torch.where(y_off > 0, torch.ones_like(g), torch.full_like(g, 0.1))).contiguous()
    want_exact = ops.conv_backward_weights(wide, td, d, False, bottom_c0=2)
    want_split = ops.conv_backward_weights(wide, td, d, False, bottom_c0=2, bf16x3=True)
    assert torch.equal(gw_off, want_exact) and not torch.equal(want_split, want_exact)
    before = Fn.LIBRARY_FALLBACKS[0]
    Fn.set_conv_weight_gradient_arithmetic("bf16x3")
    try:
        y_on, gx_on, gw_on, gb_on = grads()
        assert Fn.LIBRARY_FALLBACKS[0] - before == off_fallbacks
        assert torch.equal(gw_on, want_split)
        assert torch.equal(y_on, y_off) and torch.equal(gx_on, gx_off) and torch.equal(gb_on, gb_off)
    finally:
        Fn.set_conv_weight_gradient_arithmetic("fp32")
    y2, gx2, gw2, gb2 = grads()
    assert torch.equal(gw2, want_exact) and torch.equal(y2, y_off) and torch.equal(gx2, gx_off)


def smallest_flownetc_with_split_conv2_and_conv3():
    """(batch, H, W) with the fewest pixels at which conv2's and conv3's weight gradients take the split kernel (found on the host).  From
    128 x 128 on: the loss at 1/64 resolution downsamples the ground truth to a map that must be at least 2 x 2."""
    sizes = sorted(((B * H * W, B, H, W) for B in (1, 2) for H in range(128, 449, 64) for W in range(128, 513, 64)))
    for _, B, H, W in sizes:
        layers = {l[0]: l for l in flownetc_training_layers(B, H, W)}
        if all(arith_of(ops.conv_desc(*layers[n][2:])) == BIT for n in ("conv2", "conv3")):
            return B, H, W
    raise AssertionError("no size gives conv2 and conv3 to the split weight gradient")


@pytest.mark.gpu
def test_small_flownetc_training_step_matches_the_branch_pinned_fp64_graph():
    """Relative L2 error of the parameter gradients against the fp64 graph on the ReLU branches of the fp32 run, with the bounds of
    test_fp64_graph_is_pinned_by_the_oracle_restatements: all values together <= 1e-5, the worst parameter <= 5e-5.  Measured on an
    MI355X: at batch 1, 128 x 128: fp32 weight gradients all 1.182e-06, worst 2.540e-06 (upsample_flow6to5.b); bf16x3 weight gradients of conv2 and
    conv3 all 1.182e-06, worst 2.540e-06 (upsample_flow6to5.b)."""
    from flownet2_amd import functional as Fn
    from oracle import fp64_graph
    from test_train_parity import _batch
    B, H, W = smallest_flownetc_with_split_conv2_and_conv3()
    print("FlowNetC training step at batch %d, %d x %d" % (B, W, H))
    cuda = torch.device("cuda:0")
    P = nets.init_params("C", seed=0)
    a, b, gt = _batch(B, H, W, 4)
    Pd = {k: v.to(cuda).requires_grad_(True) for k, v in P.items()}
    took = []
    bww = ops.conv_backward_weights

    def step():
        for v in Pd.values():
            v.grad = None
        pre = [(im.to(cuda) * (1.0 / 255.0)) - 0.43 for im in (a, b)]
        loss = nets.multiscale_loss(nets.flownet_c_core(Pd, pre[0], pre[1], Fn), gt.to(cuda), Fn)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: v.grad.detach().clone() for k, v in Pd.items()}

    def recording(x, dd, desc_, tr=False, **k):
        if k.get("bf16x3") and ops.conv_backward_weights_arith(desc_, tr, True):
            took.append((desc_.Cin, desc_.Cout, desc_.kernel, desc_.stride))
        return bww(x, dd, desc_, tr, **k)

    assert Fn.conv_weight_gradient_arithmetic() == "fp32"
    fallbacks = Fn.LIBRARY_FALLBACKS[0]
    with fp64_graph.record_relu_branches() as rec:
        loss_off, g_off = step()
    _, g_p = fp64_graph.flownetc_train_reference(P, a, b, gt, device=cuda, masks=rec.branches)
    off = fp64_graph.grad_agreement(g_off, g_p)
    ops.conv_backward_weights = recording
    Fn.set_conv_weight_gradient_arithmetic("bf16x3")
    try:
        with fp64_graph.record_relu_branches() as rec_on:
            loss_on, g_on = step()
        loss_again, g_again = step()
    finally:
        Fn.set_conv_weight_gradient_arithmetic("fp32")
        ops.conv_backward_weights = bww
    assert Fn.LIBRARY_FALLBACKS[0] == fallbacks
    on = fp64_graph.grad_agreement(g_on, g_p)
    print("fp32 weight gradients:   all %.3e, worst %.3e (%s)" % (off["all"], off["worst"], off["worst_name"]))
    print("bf16x3 weight gradients: all %.3e, worst %.3e (%s); %d weight-gradient calls in split arithmetic" %
          (on["all"], on["worst"], on["worst_name"], len(took)))
    assert off["all"] <= 1e-5 and off["worst"] <= 5e-5, (off["all"], off["worst_name"], off["worst"])
    assert len(took) >= 4 and all(t[2:] == (5, 2) for t in took)          # conv2 and conv3, two steps
    assert loss_on == loss_off == loss_again and fp64_graph.relu_sign_flips(rec.branches, rec_on.branches)[0] == 0       # the forward is unchanged
    assert all(torch.equal(g_on[k], g_again[k]) for k in g_on)           # bit-reproducible
    changed = sorted(k for k in g_on if not torch.equal(g_on[k], g_off[k]))
    assert changed == ["conv2.w", "conv3.w"], changed
    assert on["all"] <= 1e-5 and on["worst"] <= 5e-5, (on["all"], on["worst_name"], on["worst"])
