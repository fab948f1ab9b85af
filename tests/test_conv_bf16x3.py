"""Split-bf16 ("bf16x3") arithmetic of the direct 5x5 / 2 convolution (csrc/conv_bf16x3.hip): FN2_CONV_ARITH_BF16X3 beside FN2_CONV_ROUTE_DIRECT,
FN2_ROUTE_BF16X3 of fn2_conv_route, functional.set_conv_arithmetic.

Host: what the route function returns with and without the flag, the operand sizes, the production layers that change.  GPU: the fp64 bound
of the exact direct kernel (4e-6 x scale) on three shapes under every flag combination, three inputs whose result is exact and needs each of
the six piece products, blob forms, reproducibility (runs, batch, tile variants), refusals decided on the host, non-finite inputs, the
Python layer, and a FlowNetC forward.

Shapes B and C are so small that fn2_conv_route hands them to the small-map kernel (PLANE) at their own batch, flag or no flag -- the flag
changes DIRECT layers only.  The host test pins that, and that the same layers at a batch the small-map kernel does not take come back as
DIRECT | 0x100; the GPU tests run A, B and C on the combined route by naming it, as fn2_conv_forward allows for any family that takes the
layer."""
import ctypes as C

import numpy as np
import pytest
import torch

from flownet2_amd import Fn2Error, _lib, nets, ops
from flownet2_amd._lib import check
from bf16x3_helpers import BIT, F_BF16X3, F_FORCE, forced_variants, host
from test_conv_backward_routes import dev, flownetc_training_layers, rand, same_bits, scale_of
from test_conv_forward_routes import DIRECT, FWD, PLANE, SENTINEL, TOL, WINOGRAD, flag_sets, production_layers

SPLIT = DIRECT | BIT
# (N, Cin, H, W, Cout), all 5x5 / 2 / 2
SHAPES = {
    "A": (2, 12, 17, 28, 64),       # the direct-5x5 case: odd H, Cin = 1.5 chunks of 8 channels
    "B": (1, 40, 9, 12, 128),       # two 64-channel groups; every tile variant hangs over both image edges
    "C": (2, 128, 20, 28, 64),      # K = 3200, the reduction length of conv3
}
# the tile variants are 32x4 and 16x8 output pixels: A (9x14 outputs), B (5x6) and C (10x14) are narrower than both and A / C taller than
# the 4- and 8-row tiles (several tile rows, the last one hanging over); one shape wider than the 32- and 16-pixel tiles
SHAPES["wide"] = (1, 8, 9, 140, 64)        # 5x70 outputs: 3 / 5 tile columns, the last hanging over


def desc(name, N=None):
    n, Cin, H, W, Cout = SHAPES[name]
    return ops.conv_desc(n if N is None else N, Cin, H, W, Cout, 5, 2, 2)


def out_hw(name):
    _, _, H, W, _ = SHAPES[name]
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def lib_route(d, flags=0):
    return int(_lib.lib().fn2_conv_route(C.byref(d), flags))


def floats(d, route):
    return int(_lib.lib().fn2_conv_packed_weight_floats(C.byref(d), route))


def ref64(x, w, b, relu, slope):
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None if b is None else torch.from_numpy(b).double(),
                                   stride=2, padding=2)
    return (torch.nn.functional.leaky_relu(y, slope) if relu else y).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# host


def fwd_desc(n, N=None):
    _, tr, b, Cin, H, W, Cout, k, s, p = FWD[n]
    return ops.conv_desc(b if N is None else N, Cin, H, W, Cout, k, s, p)


def test_route_flag_changes_direct_5x5_layers_only():
    convs = [n for n in FWD if not FWD[n][1]]
    # without the flag nothing changes
    for n in convs:
        assert lib_route(fwd_desc(n)) == FWD[n][0] and lib_route(fwd_desc(n), F_FORCE) == FWD[n][0], n
    assert [lib_route(desc(s)) for s in "ABC"] == [DIRECT, PLANE, PLANE]       # B and C: small maps, the small-map kernel's at this batch
    # with it: the DIRECT 5x5 / 2 layers, nothing else
    for n in convs:
        want = SPLIT if (FWD[n][0] == DIRECT and FWD[n][7:10] == (5, 2, 2)) else FWD[n][0]
        assert lib_route(fwd_desc(n), F_BF16X3) == want and lib_route(fwd_desc(n), F_FORCE | F_BF16X3) == want, n
    assert lib_route(fwd_desc("direct-5x5"), F_BF16X3) == SPLIT and lib_route(fwd_desc("plane-5x5"), F_BF16X3) == PLANE
    assert lib_route(desc("A"), F_BF16X3) == SPLIT == lib_route(desc("A"), F_FORCE | F_BF16X3)
    L = _lib.lib()
    for s in "ABC":
        d = desc(s)
        assert L.fn2_conv_bf16x3_supported(C.byref(d)) == 1, s
        if lib_route(d) != DIRECT:          # exactly what it returns without the flag ...
            assert lib_route(d, F_BF16X3) == lib_route(d) == PLANE, s
        big = desc(s, N=2048)               # ... and the split route at a batch the small-map kernel leaves to the direct one
        assert lib_route(big) == DIRECT and lib_route(big, F_BF16X3) == SPLIT and lib_route(big, F_FORCE | F_BF16X3) == SPLIT, s
    # FN2_ROUTE_FORCE composes: it still moves what it moved, the flag beside it changes nothing there
    small = ops.conv_desc(2, 24, 6, 8, 64, 3, 1, 1)
    assert lib_route(small, F_BF16X3) == PLANE and lib_route(small, F_FORCE | F_BF16X3) == WINOGRAD
    # batch-invariant mode: decided as for one sample, the same answer for every batch
    was = ops.get_batch_invariant()
    ops.set_batch_invariant(True)
    try:
        for s in "ABC":
            one, eight = lib_route(desc(s, N=1), F_BF16X3), lib_route(desc(s, N=8), F_BF16X3)
            assert one == eight == (SPLIT if s == "A" else PLANE), s
        assert lib_route(fwd_desc("direct-5x5", 1), F_BF16X3) == lib_route(fwd_desc("direct-5x5", 8), F_BF16X3) == SPLIT
    finally:
        ops.set_batch_invariant(was)
    assert ops.ROUTE_BF16X3 == F_BF16X3 and ops.CONV_ARITH_BF16X3 == BIT and ops.ROUTE_FORCE == F_FORCE
    assert ops.conv_forward_route(desc("A"), bf16x3=True) == SPLIT and ops.conv_forward_route(desc("A")) == DIRECT
    assert ops.conv_forward_route(desc("A"), True, True) == SPLIT
    assert set(ops.CONV_FWD_ROUTES) == set(range(6))          # the arithmetic is a bit beside the route, not a sixth route


def test_operand_sizes():
    L = _lib.lib()
    for s in SHAPES:
        d = desc(s)
        assert floats(d, SPLIT) > 0 and floats(d, SPLIT) != floats(d, DIRECT) and floats(d, DIRECT) > 0, s
        assert floats(d, WINOGRAD | BIT) == 0 and floats(d, PLANE | BIT) == 0 and floats(d, BIT) == 0, s
        assert L.fn2_conv_workspace_bytes(C.byref(d), SPLIT) == 0 and L.fn2_conv_workspace_bytes(C.byref(d), PLANE | BIT) == 0
        # three bf16 planes of [Cout / 16 groups][7 k-steps of 8 channels x 4 taps per chunk + 1][64 lanes][8]
        n, Cin, H, W, Cout = SHAPES[s]
        assert floats(d, SPLIT) == (Cout // 16) * (7 * ((Cin + 7) // 8) + 1) * 3 * 64 * 4, s
    for n in ("direct-3x3s2", "wino-threshold", "plane-3x3s1"):
        assert floats(fwd_desc(n), SPLIT) == 0 and L.fn2_conv_bf16x3_supported(C.byref(fwd_desc(n))) == 0, n
    assert L.fn2_conv_bf16x3_supported(C.byref(ops.conv_desc(2, 12, 17, 28, 96, 5, 2, 2))) == 0           # 64-channel workgroup tiles
    assert L.fn2_conv_bf16x3_supported(C.byref(ops.conv_desc(2, 12, 17, 30, 64, 5, 2, 2))) == 0           # rows of whole 16-byte pieces
    assert L.fn2_conv_bf16x3_supported(C.byref(ops.conv_desc(2, 12, 17, 28, 64, 5, 2, 1))) == 0
    assert L.fn2_conv_bf16x3_num_variants() >= 1


def test_production_layers_that_change_are_the_direct_5x5_layers():
    took, direct5 = set(), set()
    for (graph, name, kind, n, ci, h, w, co, k, s, p) in production_layers():
        if kind == "deconv":
            continue
        d = ops.conv_desc(n, ci, h, w, co, k, s, p)
        plain, flagged = lib_route(d), lib_route(d, F_BF16X3)
        if flagged & BIT:
            assert flagged == SPLIT and floats(d, SPLIT) > 0
            took.add((graph, name))
        else:
            assert flagged == plain, (graph, name)
        if plain == DIRECT and k == 5:
            direct5.add((graph, name))
    assert took == direct5 and {("C@8x448x320", "conv2"), ("C@8x448x320", "conv3")} <= took


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU


def inputs(name, N=None):
    n, Cin, H, W, Cout = SHAPES[name]
    return rand((n if N is None else N, Cin, H, W), 1), rand((Cout, Cin, 5, 5), 2, 0.1), rand((Cout,), 3, 0.1)


def pack(name, w, route=SPLIT, N=None):
    return ops.conv_pack_weights(dev(w), desc(name, N), route)


def run(name, packed, x_blob, bias, relu, slope, in_c0=0, out_blob=None, out_c0=0, N=None, route=SPLIT):
    o = None if out_blob is None else dev(out_blob)
    y = ops.conv_forward(dev(x_blob), packed, None if bias is None else dev(bias), desc(name, N), route, False, relu, slope, out=o, out_c0=out_c0, in_c0=in_c0)
    torch.cuda.synchronize()
    return host(y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp64_bound(name):
    """error / bound, worst of the six flag sets (measured on an MI355X): A 0.19, B 0.20, C 0.45, wide 0.11."""
    x, w, b = inputs(name)
    packed = pack(name, w)
    for relu, has_b, slope in flag_sets("direct-5x5"):
        bb = b if has_b else None
        got = run(name, packed, x, bb, relu, slope)
        ref = ref64(x, w, bb, relu, slope)
        assert got.shape == ref.shape
        ratio = float(np.abs(got - ref).max()) / (TOL[(False, DIRECT)] * scale_of(ref))
        print("bf16x3 fp64 error / bound: %s relu=%d bias=%d slope=%g: %.3f" % (name, relu, has_b, slope, ratio))
        assert ratio <= 1.0, (name, relu, has_b, slope, ratio)


def exact_inputs(kind):
    N, Cin, H, W, Cout = SHAPES["A"]
    rng = np.random.default_rng(11)
    if kind == "select-x":          # needs hh, mh, lh
        x = rand((N, Cin, H, W), 21)
        w = np.zeros((Cout, Cin, 5, 5), np.float32)
        w[np.arange(Cout), rng.integers(0, Cin, Cout), rng.integers(0, 5, Cout), rng.integers(0, 5, Cout)] = rng.choice([1.0, -1.0, 0.5, -2.0], Cout)
        return x, w
    if kind == "select-w":          # needs hh, hm, hl: one nonzero pixel in every 5x5 window
        w = rand((Cout, Cin, 5, 5), 22, 0.1)
        x = np.zeros((N, Cin, H, W), np.float32)
        for n in range(N):
            for y in range(n, H, 5):
                for xx in range(2 * n, W, 5):
                    x[n, (3 * y + 5 * xx + n) % Cin, y, xx] = rng.choice([1.0, -1.0, 2.0, -0.5])
        return x, w
    # mid-x-mid: needs mm
    x = (1.0 + rng.integers(0, 4, (N, Cin, H, W)) / 1024.0).astype(np.float32)
    w = np.zeros((Cout, Cin, 5, 5), np.float32)
    for co in range(Cout):
        for f in rng.choice(Cin * 25, 4, replace=False):
            w[co].reshape(-1)[f] = rng.choice([1.0, -1.0]) * (1.0 + rng.integers(0, 4) / 1024.0)
    return x, w


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["select-x", "select-w", "mid-x-mid"])
def test_exact_values(kind):
    x, w = exact_inputs(kind)
    ref = ref64(x, w, None, False, 0.1)
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref) and np.abs(ref).max() > 0.5          # the reference is itself an fp32 value
    if kind == "mid-x-mid":
        assert (np.round(x * 1024) % 4 != 0).any() and np.abs(ref).max() < 8
    got = run("A", pack("A", w), x, None, False, 0.1)
    assert same_bits(got + np.float32(0.0), ref32 + np.float32(0.0)), (kind, float(np.abs(got - ref32).max()))      # (+ 0.0: -0.0 == 0.0)


@pytest.mark.gpu
def test_blob_forms_and_flags():
    N, Cin, H, W, Cout = SHAPES["A"]
    Ho, Wo = out_hw("A")
    x, w, b = inputs("A")
    packed = pack("A", w)
    fresh = {f: run("A", packed, x, b if f[1] else None, f[0], f[2]) for f in flag_sets("direct-5x5")}
    assert (fresh[(True, True, 0.1)] != fresh[(False, True, 0.1)]).any() and (fresh[(True, True, 0.1)] != fresh[(True, True, 0.0)]).any()
    assert (fresh[(False, True, 0.1)] < 0).any() and not (fresh[(True, True, 0.0)] < 0).any()
    assert (fresh[(True, True, 0.1)] != fresh[(True, False, 0.1)]).any()
    base = fresh[(True, True, 0.1)]
    wide = rand((N, Cin + 5, H, W), 9)
    wide[:, 2:2 + Cin] = x
    for in_slice, out_slice in [(False, True), (True, False), (True, True)]:
        blob = np.full((N, Cout + 7, Ho, Wo), SENTINEL) if out_slice else None
        got = run("A", packed, wide if in_slice else x, b, True, 0.1, 2 if in_slice else 0, blob, 3 if out_slice else 0)
        if out_slice:
            assert (got[:, :3] == SENTINEL).all() and (got[:, 3 + Cout:] == SENTINEL).all(), (in_slice, out_slice)
            got = got[:, 3:3 + Cout]
        assert same_bits(got, base), (in_slice, out_slice)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_reproducible_across_runs_batch_and_variants(name):
    L = _lib.lib()
    x, w, b = inputs(name, N=3)
    packed = pack(name, w, N=3)
    batch = run(name, packed, x, b, True, 0.1, N=3)
    assert same_bits(run(name, packed, x, b, True, 0.1, N=3), batch)
    assert same_bits(run(name, pack(name, w, N=1), x[:1], b, True, 0.1, N=1), batch[:1])
    was = ops.get_batch_invariant()
    ops.set_batch_invariant(True)
    try:
        assert same_bits(run(name, packed, x, b, True, 0.1, N=3), batch)
        assert same_bits(run(name, packed, x[:1], b, True, 0.1, N=1), batch[:1])
    finally:
        ops.set_batch_invariant(was)
    ran = 0
    with forced_variants("conv_bf16x3") as (nv, force):
        for v in range(nv):
            force(v)
            assert same_bits(run(name, packed, x, b, True, 0.1, N=3), batch), v          # (every variant applies: they all block 64 channels)
            ran += 1
        force(nv)
        with pytest.raises(Fn2Error):
            run(name, packed, x, b, True, 0.1, N=3)
    assert ran == nv >= 2


def raw_forward(d, route, x, in_ch, in_c0, packed, top, top_ch, top_c0, null=()):
    ptr = {"bottom": ops._ptr(x), "packed": ops._ptr(packed), "top": ops._ptr(top)}
    for n in null:
        ptr[n] = None
    try:
        check(_lib.lib().fn2_conv_forward(C.byref(d), int(route), ptr["bottom"], in_ch, in_c0, ptr["packed"], None, ptr["top"], top_ch, top_c0, 1,
                                          C.c_float(0.1), None, 0, ops._stream()))
    finally:
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_refusals_are_decided_on_the_host():
    N, Cin, H, W, Cout = SHAPES["A"]
    Ho, Wo = out_hw("A")
    d = desc("A")
    x = dev(rand((N, Cin + 8, H, W), 4))
    w = rand((Cout, Cin, 5, 5), 2, 0.1)
    split_op, exact_op = pack("A", w), pack("A", w, DIRECT)
    top = torch.full((N, Cout + 8, Ho, Wo), float(SENTINEL), device="cuda")
    untouched = lambda: bool((top == float(SENTINEL)).all())
    d3 = ops.conv_desc(N, Cin, H, W, Cout, 3, 2, 1)          # a DIRECT layer of another geometry: top of the same size
    assert lib_route(d3) == DIRECT and ((H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1) == (Ho, Wo)
    calls = {
        "3x3 / 2 descriptor": dict(d=d3), "WINOGRAD | 0x100": dict(route=WINOGRAD | BIT), "PLANE | 0x100": dict(route=PLANE | BIT), "0x100 alone": dict(route=BIT),
        "null bottom": dict(null=("bottom",)), "null operand": dict(null=("packed",)), "null top": dict(null=("top",)),
        "bottom slice past its blob": dict(in_ch=Cin + 1, in_c0=2), "top slice past its blob": dict(top_ch=Cout + 2, top_c0=3),
        "negative top slice": dict(top_ch=Cout + 8, top_c0=-1),
    }
    for what, kw in calls.items():
        a = dict(d=d, route=SPLIT, in_ch=Cin + 8, in_c0=0, top_ch=Cout + 8, top_c0=0, null=())
        a.update(kw)
        with pytest.raises(Fn2Error):
            raw_forward(a["d"], a["route"], x, a["in_ch"], a["in_c0"], split_op, top, a["top_ch"], a["top_c0"], a["null"])
            pytest.fail("%s was not refused" % what)
        assert untouched(), what
    # an operand packed for the other arithmetic: ops.conv_forward's length check
    xs = x[:, :Cin].contiguous()
    for operand, route in ((exact_op, SPLIT), (split_op, DIRECT)):
        with pytest.raises(ValueError):
            ops.conv_forward(xs, operand, None, d, route, False, True, 0.1, out=top)
        assert untouched()
    with pytest.raises(ValueError):
        ops.conv_pack_weights(dev(rand((Cout, Cin, 3, 3), 2)), d3, SPLIT)
    for r in (WINOGRAD | BIT, BIT):
        with pytest.raises(ValueError):
            ops.conv_pack_weights(dev(w), d, r)
    with pytest.raises(Fn2Error):
        check(_lib.lib().fn2_conv_pack_weights(C.byref(d), PLANE | BIT, ops._ptr(dev(w)), ops._ptr(split_op), ops._stream()))
    torch.cuda.synchronize()
    # ... and the call none of this applies to writes exactly the layer's channels
    raw_forward(d, SPLIT, x, Cin + 8, 0, split_op, top, Cout + 8, 0)
    assert not bool((top[:, :Cout] == float(SENTINEL)).any()) and bool((top[:, Cout:] == float(SENTINEL)).all())


@pytest.mark.gpu
def test_non_finite_inputs_reach_their_own_windows_only():
    N, Cin, H, W, Cout = SHAPES["A"]
    Ho, Wo = out_hw("A")
    x, w, b = inputs("A")
    assert (w != 0).all()
    packed = pack("A", w)
    clean = run("A", packed, x, b, True, 0.1)
    assert np.isfinite(clean).all()
    bad = x.copy()
    spots = [(0, 3, 4, 7, np.inf), (1, 10, 13, 21, np.nan)]          # channel 10: the ragged second chunk.  Different samples: no window holds both
    covered = np.zeros((N, Ho, Wo), bool)
    for (n, c, yy, xx, v) in spots:
        bad[n, c, yy, xx] = v
        for oy in range(Ho):
            for ox in range(Wo):
                if 0 <= yy - (2 * oy - 2) < 5 and 0 <= xx - (2 * ox - 2) < 5:
                    covered[n, oy, ox] = True
    assert 0 < covered.sum() < covered.size // 4
    got = run("A", packed, bad, b, True, 0.1)
    mask = np.broadcast_to(covered[:, None], got.shape)
    assert np.array_equal(~np.isfinite(got), mask)
    assert np.array_equal(got.view(np.uint32)[~mask], clean.view(np.uint32)[~mask])


@pytest.mark.gpu
def test_python_layer(monkeypatch):
    from flownet2_amd import functional as Fn
    monkeypatch.delenv("FN2_STRICT", raising=False)          # (A's 12-channel data gradient is the library's, counted, in either arithmetic)
    N, Cin, H, W, Cout = SHAPES["A"]
    Ho, Wo = out_hw("A")
    d = desc("A")
    w, b = dev(rand((Cout, Cin, 5, 5), 2, 0.1)), dev(rand((Cout,), 3, 0.1))
    wide = dev(rand((N, Cin + 5, H, W), 9))
    x = wide[:, 2:2 + Cin]
    assert not x.is_contiguous()
    want = ops.conv_forward(x.contiguous(), ops.conv_pack_weights(w, d, SPLIT), b, d, SPLIT, False, True, 0.1)
    exact = ops.conv_forward(x.contiguous(), ops.conv_pack_weights(w, d, DIRECT), b, d, DIRECT, False, True, 0.1)
    assert not torch.equal(want, exact)
    g = dev(rand((N, Cout, Ho, Wo), 13))

    def grads():
        xg, wg, bg = x.detach().clone().requires_grad_(True), torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
        y = Fn.conv_mfma_relu(xg, wg, bg, 2, 2, 0.1, True)
        assert y.requires_grad and y.grad_fn is not None
        # the gradients as functions of the SAME activation mask: the backward reads the saved output's sign only
        (y * g).sum().backward()
        return y.detach(), xg.grad.clone(), wg.grad.clone(), bg.grad.clone()

    assert Fn.conv_arithmetic() == "fp32"
    before = Fn.LIBRARY_FALLBACKS[0]
    y_off, gx_off, gw_off, gb_off = grads()
    assert torch.equal(y_off, exact)
    bwd_fallbacks = Fn.LIBRARY_FALLBACKS[0] - before         # what the backward of this layer hands to the library: not a matter of the forward
    before = Fn.LIBRARY_FALLBACKS[0]
    Fn.set_conv_arithmetic("bf16x3")
    try:
        assert Fn.conv_arithmetic() == "bf16x3" and Fn.conv_forward_route(d) == SPLIT
        assert Fn.conv_route_name(x.shape, w, 2, 2) == "direct+bf16x3" and Fn.conv_route_name((N, Cin, H, W), dev(rand((Cout, Cin, 3, 3), 2)), 2, 1) == "direct"
        assert torch.equal(Fn.conv_mfma_relu(x, w, b, 2, 2, 0.1, True), want)
        blob = torch.full((N, Cout + 7, Ho, Wo), float(SENTINEL), device="cuda")
        Fn.conv_mfma_relu(x, w, b, 2, 2, 0.1, True, out=blob, out_c0=3)
        assert torch.equal(blob[:, 3:3 + Cout], want) and bool((blob[:, :3] == float(SENTINEL)).all()) and bool((blob[:, 3 + Cout:] == float(SENTINEL)).all())
        assert Fn.LIBRARY_FALLBACKS[0] == before             # the forward never falls back
        y_on, gx_on, gw_on, gb_on = grads()
        assert torch.equal(y_on, want) and Fn.LIBRARY_FALLBACKS[0] == before + bwd_fallbacks
        # every backward route stays exact fp32: where the two forwards agree in sign everywhere the gradients are the same bits
        assert torch.equal((y_on > 0), (y_off > 0))
        assert torch.equal(gx_on, gx_off) and torch.equal(gw_on, gw_off) and torch.equal(gb_on, gb_off)
        with pytest.raises(ValueError):
            Fn.set_conv_arithmetic("bf16")
        assert Fn.conv_arithmetic() == "bf16x3"
    finally:
        Fn.set_conv_arithmetic("fp32")
    assert Fn.conv_arithmetic() == "fp32" and Fn.conv_forward_route(d) == DIRECT
    assert torch.equal(Fn.conv_mfma_relu(x, w, b, 2, 2, 0.1, True), exact)
    keys = [key for key in Fn._PACKED_T if key[0] == id(w) and key[1][0] == "fwd"]
    assert sorted(key[1][1] for key in keys) == [DIRECT, SPLIT]
    assert Fn.LIBRARY_FALLBACKS[0] == before + bwd_fallbacks


def smallest_flownetc_with_direct_conv2():
    """(batch, H, W) with the fewest pixels at which fn2_conv_route sends FlowNetC's conv2 to the direct kernel (found on the host)."""
    sizes = sorted(((B * H * W, B, H, W) for B in (1, 2, 3, 4) for H in range(64, 449, 64) for W in range(64, 513, 64)))
    for _, B, H, W in sizes:
        conv2 = [l for l in flownetc_training_layers(B, H, W) if l[0] == "conv2"][0]
        if lib_route(ops.conv_desc(*conv2[2:]), F_BF16X3) == SPLIT:
            return B, H, W
    raise AssertionError("no size routes conv2 to the direct kernel")


@pytest.mark.gpu
def test_flownetc_end_to_end(monkeypatch):
    from flownet2_amd import functional as Fn
    B, H, W = smallest_flownetc_with_direct_conv2()
    print("FlowNetC at batch %d, %d x %d" % (B, W, H))
    routes = []
    fwd = ops.conv_forward
    monkeypatch.setattr(ops, "conv_forward", lambda x, packed, bias, desc, route, *a, **k: routes.append(int(route)) or fwd(x, packed, bias, desc, route, *a, **k))
    P = {k: v.cuda() for k, v in nets.init_params("C", 0).items()}
    rng = np.random.default_rng(5)
    i0 = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)).cuda()
    i1 = torch.roll(i0, (2, -3), (2, 3)).contiguous()
    assert Fn.conv_arithmetic() == "fp32"
    with torch.no_grad():
        exact = nets.deploy_forward("C", P, i0, i1, Fn)
        assert routes and not any(r & BIT for r in routes)
        del routes[:]
        Fn.set_conv_arithmetic("bf16x3")
        try:
            split = nets.deploy_forward("C", P, i0, i1, Fn)
            took = [r for r in routes if r & BIT]
            again = nets.deploy_forward("C", P, i0, i1, Fn)
        finally:
            Fn.set_conv_arithmetic("fp32")
    assert took and all(r == SPLIT for r in took)
    assert torch.equal(split, again)
    epd = float(((split - exact) ** 2).sum(1).sqrt().mean())
    print("mean end-point difference bf16x3 vs fp32: %.3e px (%d layer calls in split arithmetic)" % (epd, len(took)))
    assert np.isfinite(epd) and epd <= 1e-4, epd
