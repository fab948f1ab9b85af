"""Split-bf16 ("bf16x3") arithmetic of the Deconvolution{4, 2, 1} GEMM (csrc/deconv_bf16x3.hip): FN2_CONV_ARITH_BF16X3 beside
FN2_DECONV_ROUTE_GEMM, FN2_ROUTE_BF16X3 of fn2_deconv_route, functional.set_deconv_arithmetic.

Host: what the route function returns with and without the flag, the operand sizes, the production layers that change.  GPU: the fp64 bound
of the exact GEMM route (3e-6 x scale) on four shapes under every flag combination, three inputs whose result is exact and needs each of the
six piece products, blob forms and the workspace tail, reproducibility (runs, batch, tile variants), refusals decided on the host,
non-finite inputs, the Python layer, and a FlowNetC forward."""
import ctypes as C

import numpy as np
import pytest
import torch

from flownet2_amd import Fn2Error, _lib, nets, ops
from flownet2_amd._lib import check
from bf16x3_helpers import BIT, F_BF16X3, F_FORCE, forced_variants, host
from test_conv_backward_routes import dev, flownetc_training_layers, rand, same_bits, scale_of
from test_conv_forward_routes import D_GEMM, D_HEAD, D_NONE, D_PLANE, DIRECT, FWD, HEAD, SENTINEL, TOL, flag_sets, production_layers

SPLIT = D_GEMM | BIT
# (N, Cin, H, W, Cout), all Deconvolution{4, 2, 1}.  The workgroup tiles are 128 and 64 rows x 128 pixels, a k-step is 32 channels
SHAPES = {
    "A": (3, 70, 5, 8, 36),         # two k-steps + 6 ragged channels; a 40-pixel plane, smaller than the pixel tile; M = 576 hangs over a 128-row tile
    "B": (2, 33, 6, 22, 64),        # a single ragged channel; P = 132: one quad past the 128-pixel tile
    "C": (1, 1026, 10, 14, 64),     # deconv4's reduction length
    "D": (2, 8, 4, 4, 16),          # one partial k-step; M = 256
}


def desc(name, N=None):
    n, Cin, H, W, Cout = SHAPES[name]
    return ops.conv_desc(n if N is None else N, Cin, H, W, Cout, 4, 2, 1)


def deconv_route(d, flags=0):
    return int(_lib.lib().fn2_deconv_route(C.byref(d), flags))


def floats(d, route):
    return int(_lib.lib().fn2_deconv_packed_weight_floats(C.byref(d), route))


def ws_bytes(d, route):
    return int(_lib.lib().fn2_deconv_workspace_bytes(C.byref(d), route))


def supported(d):
    return int(_lib.lib().fn2_deconv_bf16x3_supported(C.byref(d)))


def ref64(x, w, b, relu, slope):
    y = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None if b is None else torch.from_numpy(b).double(),
                                             stride=2, padding=1)
    return (torch.nn.functional.leaky_relu(y, slope) if relu else y).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# host


def fwd_desc(n, N=None):
    _, tr, b, Cin, H, W, Cout, k, s, p = FWD[n]
    return ops.conv_desc(b if N is None else N, Cin, H, W, Cout, k, s, p)


def test_flag_changes_gemm_layers_only():
    L = _lib.lib()
    deconvs = [n for n in FWD if FWD[n][1]]
    # flags 0: nothing changes, in the case table and in the production graphs
    for n in FWD:
        route = L.fn2_deconv_route if FWD[n][1] else L.fn2_conv_route
        assert int(route(C.byref(fwd_desc(n)), 0)) == FWD[n][0] == int(route(C.byref(fwd_desc(n)), F_FORCE)), n
    for s in SHAPES:
        assert deconv_route(desc(s)) == D_GEMM and supported(desc(s)) == 1, s
        assert deconv_route(desc(s), F_BF16X3) == SPLIT == deconv_route(desc(s), F_FORCE | F_BF16X3), s
    # with it: the GEMM layers the kernel takes; PLANE and HEAD as without it
    for n in deconvs:
        want = SPLIT if (FWD[n][0] == D_GEMM and supported(fwd_desc(n))) else FWD[n][0]
        assert deconv_route(fwd_desc(n), F_BF16X3) == want, n
    assert supported(fwd_desc("deconv-gemm")) == 1          # (16 Cout % 32 == 0 is all the kernel asks of the channels: Cout 34 is its)
    assert deconv_route(fwd_desc("deconv-plane"), F_BF16X3) == D_PLANE and deconv_route(fwd_desc("deconv-head"), F_BF16X3) == D_HEAD
    assert supported(fwd_desc("deconv-plane")) == 0 and supported(ops.conv_desc(2, 64, 5, 8, 64, 3, 2, 1)) == 0
    assert deconv_route(ops.conv_desc(2, 64, 5, 8, 64, 3, 2, 1), F_BF16X3) == D_NONE
    # the Convolution side is untouched: a 1x1 layer stays on the exact direct kernel
    assert int(L.fn2_conv_route(C.byref(fwd_desc("direct-1x1")), F_BF16X3)) == DIRECT
    # batch-invariant mode: the same answer for every batch
    was = ops.get_batch_invariant()
    ops.set_batch_invariant(True)
    try:
        for s in SHAPES:
            assert deconv_route(desc(s, N=1), F_BF16X3) == deconv_route(desc(s, N=8), F_BF16X3) == SPLIT, s
            assert deconv_route(desc(s, N=1)) == deconv_route(desc(s, N=8)) == D_GEMM, s
        for n in deconvs:
            assert deconv_route(fwd_desc(n, 1), F_BF16X3) == deconv_route(fwd_desc(n, 8), F_BF16X3), n
    finally:
        ops.set_batch_invariant(was)
    assert ops.deconv_forward_route(desc("A"), bf16x3=True) == SPLIT and ops.deconv_forward_route(desc("A")) == D_GEMM
    assert set(ops.DECONV_FWD_ROUTES) == set(range(4))          # the arithmetic is a bit beside the route, not a fourth route


def test_operand_sizes():
    L = _lib.lib()
    for s in SHAPES:
        d = desc(s)
        n, Cin, H, W, Cout = SHAPES[s]
        assert floats(d, SPLIT) > 0 and floats(d, D_GEMM) > 0 and floats(d, SPLIT) != floats(d, D_GEMM), s
        # three bf16 planes of [M / 16 = Cout row groups][k-steps of 32 channels + 1 spare][64 lanes][8]
        assert floats(d, SPLIT) == Cout * ((Cin + 31) // 32 + 1) * 3 * 64 * 4, s
        assert floats(d, D_PLANE | BIT) == 0 and floats(d, D_HEAD | BIT) == 0 and floats(d, BIT) == 0, s
        assert ws_bytes(d, SPLIT) == ws_bytes(d, D_GEMM) == 4 * n * 16 * Cout * H * W, s
        assert ws_bytes(d, D_PLANE | BIT) == 0 and ws_bytes(d, D_HEAD | BIT) == 0 and ws_bytes(d, BIT) == 0, s
    for n in ("deconv-plane", "deconv-head"):          # layers the kernel does not take
        assert floats(fwd_desc(n), SPLIT) == 0 and ws_bytes(fwd_desc(n), SPLIT) == 0 and supported(fwd_desc(n)) == 0, n
        assert floats(fwd_desc(n), FWD[n][0] | BIT) == 0, n
    assert floats(ops.conv_desc(2, 64, 5, 8, 64, 3, 2, 1), SPLIT) == 0
    assert L.fn2_deconv_bf16x3_num_variants() >= 2


def test_production_layers_that_change_are_the_gemm_layers():
    took, gemm = set(), set()
    L = _lib.lib()
    for (graph, name, kind, n, ci, h, w, co, k, s, p) in production_layers():
        d = ops.conv_desc(n, ci, h, w, co, k, s, p)
        if kind != "deconv":
            continue
        plain, flagged = deconv_route(d), deconv_route(d, F_BF16X3)
        assert not plain & BIT and plain == flagged & ~BIT, (graph, name)          # the flag adds the bit, nothing else
        if flagged & BIT:
            assert flagged == SPLIT and floats(d, SPLIT) > 0
            took.add((graph, name))
        if plain == D_GEMM and supported(d):
            gemm.add((graph, name))
        if plain in (D_PLANE, D_HEAD):
            assert flagged == plain, (graph, name)
    assert took == gemm and {("C@8x448x320", "deconv4"), ("C@8x448x320", "deconv3"), ("C@8x448x320", "deconv2")} <= took


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU


def inputs(name, N=None):
    n, Cin, H, W, Cout = SHAPES[name]
    return rand((n if N is None else N, Cin, H, W), 1), rand((Cin, Cout, 4, 4), 2, 0.1), rand((Cout,), 3, 0.1)


def pack(name, w, route=SPLIT, N=None):
    return ops.conv_pack_weights(dev(w), desc(name, N), route, True)


def run(name, packed, x_blob, bias, relu, slope, in_c0=0, out_blob=None, out_c0=0, N=None, route=SPLIT):
    o = None if out_blob is None else dev(out_blob)
    y = ops.conv_forward(dev(x_blob), packed, None if bias is None else dev(bias), desc(name, N), route, True, relu, slope, out=o, out_c0=out_c0, in_c0=in_c0)
    torch.cuda.synchronize()
    return host(y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp64_bound(name):
    """error / bound, worst of the six flag sets (measured on an MI355X): A 0.074, B 0.052, C 0.248, D 0.026."""
    x, w, b = inputs(name)
    packed = pack(name, w)
    for relu, has_b, slope in flag_sets("deconv-gemm"):
        bb = b if has_b else None
        got = run(name, packed, x, bb, relu, slope)
        ref = ref64(x, w, bb, relu, slope)
        assert got.shape == ref.shape
        ratio = float(np.abs(got - ref).max()) / (TOL[(True, D_GEMM)] * scale_of(ref))
        print("deconv bf16x3 fp64 error / bound: %s relu=%d bias=%d slope=%g: %.3f" % (name, relu, has_b, slope, ratio))
        assert ratio <= 1.0, (name, relu, has_b, slope, ratio)


def exact_inputs(kind):
    N, Cin, H, W, Cout = SHAPES["A"]
    rng = np.random.default_rng(11)
    if kind == "select-x":          # needs hh, mh, lh: one nonzero weight per output channel = at most one term per output
        x = rand((N, Cin, H, W), 21)
        w = np.zeros((Cin, Cout, 4, 4), np.float32)
        w[rng.integers(0, Cin, Cout), np.arange(Cout), rng.integers(0, 4, Cout), rng.integers(0, 4, Cout)] = rng.choice([1.0, -1.0, 0.5, -2.0], Cout)
        return x, w
    if kind == "select-w":          # needs hh, hm, hl: nonzero pixels two apart, in one channel each = disjoint 4x4 footprints
        w = rand((Cin, Cout, 4, 4), 22, 0.1)
        x = np.zeros((N, Cin, H, W), np.float32)
        for n in range(N):
            for y in range(n % 2, H, 2):
                for xx in range((n // 2) % 2, W, 2):
                    x[n, (3 * y + 5 * xx + 7 * n) % Cin, y, xx] = rng.choice([1.0, -1.0, 2.0, -0.5])
        return x, w
    # mid-x-mid: needs mm
    x = (1.0 + rng.integers(0, 4, (N, Cin, H, W)) / 1024.0).astype(np.float32)
    w = np.zeros((Cin, Cout, 4, 4), np.float32)
    for co in range(Cout):
        for f in rng.choice(Cin * 16, 4, replace=False):
            w[f // 16, co, (f % 16) // 4, f % 4] = rng.choice([1.0, -1.0]) * (1.0 + rng.integers(0, 4) / 1024.0)
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


def raw_forward(d, route, x, in_ch, in_c0, packed, top, top_ch, top_c0, ws="need", ws_bytes_=None, null=()):
    """fn2_deconv_forward past the Python checks.  ws: "need" = a workspace of the size the GEMM route asks for, None = no workspace."""
    need = ws_bytes(desc("A") if d is None else d, D_GEMM)
    if isinstance(ws, str):
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    ptr = {"bottom": ops._ptr(x), "packed": ops._ptr(packed), "top": ops._ptr(top)}
    for n in null:
        ptr[n] = None
    try:
        check(_lib.lib().fn2_deconv_forward(C.byref(d), int(route), ptr["bottom"], in_ch, in_c0, ptr["packed"], None, ptr["top"], top_ch, top_c0, 1,
                                            C.c_float(0.1), None if ws is None else ops._ptr(ws), need if ws_bytes_ is None else ws_bytes_, ops._stream()))
    finally:
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_blob_forms_flags_and_workspace_tail():
    N, Cin, H, W, Cout = SHAPES["A"]
    x, w, b = inputs("A")
    packed = pack("A", w)
    fresh = {f: run("A", packed, x, b if f[1] else None, f[0], f[2]) for f in flag_sets("deconv-gemm")}
    assert (fresh[(True, True, 0.1)] != fresh[(False, True, 0.1)]).any() and (fresh[(True, True, 0.1)] != fresh[(True, True, 0.0)]).any()
    assert (fresh[(False, True, 0.1)] < 0).any() and not (fresh[(True, True, 0.0)] < 0).any()
    assert (fresh[(True, True, 0.1)] != fresh[(True, False, 0.1)]).any()
    base = fresh[(True, True, 0.1)]
    wide = rand((N, Cin + 5, H, W), 9)
    wide[:, 2:2 + Cin] = x
    for in_slice, out_slice in [(False, True), (True, False), (True, True)]:
        blob = np.full((N, Cout + 7, 2 * H, 2 * W), SENTINEL) if out_slice else None
        got = run("A", packed, wide if in_slice else x, b, True, 0.1, 2 if in_slice else 0, blob, 3 if out_slice else 0)
        if out_slice:
            assert (got[:, :3] == SENTINEL).all() and (got[:, 3 + Cout:] == SENTINEL).all(), (in_slice, out_slice)
            got = got[:, 3:3 + Cout]
        assert same_bits(got, base), (in_slice, out_slice)
    # the column matrix ends where fn2_deconv_workspace_bytes says: a longer workspace keeps its tail
    d = desc("A")
    need = ws_bytes(d, SPLIT)
    ws = torch.full((need // 4 + 4096,), float(SENTINEL), device="cuda")
    top = torch.full((N, Cout, 2 * H, 2 * W), float(SENTINEL), device="cuda")
    raw_forward(d, SPLIT, dev(x), Cin, 0, packed, top, Cout, 0, ws=ws, ws_bytes_=4 * ws.numel())
    assert bool((ws[need // 4:] == float(SENTINEL)).all()) and not bool((ws[:need // 4] == float(SENTINEL)).any())
    assert same_bits(host(top), fresh[(True, False, 0.1)])


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
    with forced_variants("deconv_bf16x3") as (nv, force):
        for v in range(nv):
            force(v)
            assert same_bits(run(name, packed, x, b, True, 0.1, N=3), batch), v
            ran += 1
        force(nv)
        with pytest.raises(Fn2Error):
            run(name, packed, x, b, True, 0.1, N=3)
    assert ran == nv >= 2


@pytest.mark.gpu
def test_refusals_are_decided_on_the_host():
    N, Cin, H, W, Cout = SHAPES["A"]
    d = desc("A")
    x = dev(rand((N, Cin + 8, H, W), 4))
    w = rand((Cin, Cout, 4, 4), 2, 0.1)
    split_op, exact_op = pack("A", w), pack("A", w, D_GEMM)
    top = torch.full((N, Cout + 8, 2 * H, 2 * W), float(SENTINEL), device="cuda")
    untouched = lambda: bool((top == float(SENTINEL)).all())
    d3 = ops.conv_desc(N, Cin, H, W, Cout, 3, 2, 1)          # not a Deconvolution{4, 2, 1}
    need = ws_bytes(d, SPLIT)
    calls = {
        "3x3 / 2 descriptor": dict(d=d3), "PLANE | 0x100": dict(route=D_PLANE | BIT), "HEAD | 0x100": dict(route=D_HEAD | BIT), "0x100 alone": dict(route=BIT),
        "null bottom": dict(null=("bottom",)), "null operand": dict(null=("packed",)), "null top": dict(null=("top",)),
        "bottom slice past its blob": dict(in_ch=Cin + 1, in_c0=2), "top slice past its blob": dict(top_ch=Cout + 2, top_c0=3),
        "negative top slice": dict(top_ch=Cout + 8, top_c0=-1), "negative bottom slice": dict(in_c0=-1),
        "no workspace": dict(ws=None), "short workspace": dict(ws_bytes_=need - 4),
    }
    for what, kw in calls.items():
        a = dict(d=d, route=SPLIT, in_ch=Cin + 8, in_c0=0, top_ch=Cout + 8, top_c0=0, null=(), ws="need", ws_bytes_=None)
        a.update(kw)
        with pytest.raises(Fn2Error):
            raw_forward(a["d"], a["route"], x, a["in_ch"], a["in_c0"], split_op, top, a["top_ch"], a["top_c0"], a["ws"], a["ws_bytes_"], a["null"])
            pytest.fail("%s was not refused" % what)
        assert untouched(), what
    # an operand packed for the other arithmetic: ops.conv_forward's length check
    xs = x[:, :Cin].contiguous()
    for operand, route in ((exact_op, SPLIT), (split_op, D_GEMM)):
        with pytest.raises(ValueError):
            ops.conv_forward(xs, operand, None, d, route, True, True, 0.1, out=top)
        assert untouched()
    for r in (D_PLANE | BIT, D_HEAD | BIT, BIT):
        with pytest.raises(ValueError):
            ops.conv_pack_weights(dev(w), d, r, True)
        with pytest.raises(Fn2Error):
            check(_lib.lib().fn2_deconv_pack_weights(C.byref(d), r, ops._ptr(dev(w)), ops._ptr(split_op), ops._stream()))
    with pytest.raises(Fn2Error):
        check(_lib.lib().fn2_deconv_pack_weights(C.byref(d3), SPLIT, ops._ptr(dev(w)), ops._ptr(split_op), ops._stream()))
    torch.cuda.synchronize()
    # ... and the call none of this applies to writes exactly the layer's channels
    raw_forward(d, SPLIT, x, Cin + 8, 0, split_op, top, Cout + 8, 0)
    assert not bool((top[:, :Cout] == float(SENTINEL)).any()) and bool((top[:, Cout:] == float(SENTINEL)).all())


@pytest.mark.gpu
def test_non_finite_inputs_reach_their_own_footprints_only():
    N, Cin, H, W, Cout = SHAPES["A"]
    x, w, b = inputs("A")
    assert (w != 0).all() and Cin % 32 != 0
    packed = pack("A", w)
    clean = run("A", packed, x, b, True, 0.1)
    assert np.isfinite(clean).all()
    # (a) NaN and Inf in the channels of a wider blob just outside the layer's slice: not one bit changes (the ragged k-step reads zeros)
    wide = rand((N, Cin + 5, H, W), 9)
    wide[:, 2:2 + Cin] = x
    assert same_bits(run("A", packed, wide, b, True, 0.1, 2), clean)
    wide[:, :2] = np.nan
    wide[:, 2 + Cin] = np.inf
    wide[:, 3 + Cin:] = np.nan
    assert same_bits(run("A", packed, wide, b, True, 0.1, 2), clean)
    # (b) inside the slice: exactly the 4x4 footprints, in every output channel
    bad = x.copy()
    spots = [(0, 3, 2, 5, np.inf), (1, 67, 4, 0, np.nan)]          # channel 67: the ragged third k-step.  Different samples: no output sees both
    covered = np.zeros((N, 2 * H, 2 * W), bool)
    for (n, c, yy, xx, v) in spots:
        bad[n, c, yy, xx] = v
        covered[n, max(2 * yy - 1, 0):min(2 * yy + 3, 2 * H), max(2 * xx - 1, 0):min(2 * xx + 3, 2 * W)] = True
    assert covered.sum() == 16 + 9 and not covered[2].any()
    got = run("A", packed, bad, b, True, 0.1)
    mask = np.broadcast_to(covered[:, None], got.shape)
    assert np.array_equal(~np.isfinite(got), mask)
    assert np.array_equal(got.view(np.uint32)[~mask], clean.view(np.uint32)[~mask])


@pytest.mark.gpu
def test_python_layer(monkeypatch):
    from flownet2_amd import functional as Fn
    monkeypatch.delenv("FN2_STRICT", raising=False)          # (what the backward of this layer hands to the library is counted in either arithmetic)
    N, Cin, H, W, Cout = SHAPES["A"]
    d = desc("A")
    w, b = dev(rand((Cin, Cout, 4, 4), 2, 0.1)), dev(rand((Cout,), 3, 0.1))
    wide = dev(rand((N, Cin + 5, H, W), 9))
    x = wide[:, 2:2 + Cin]
    assert not x.is_contiguous()
    want = ops.conv_forward(x.contiguous(), ops.conv_pack_weights(w, d, SPLIT, True), b, d, SPLIT, True, True, 0.1)
    exact = ops.conv_forward(x.contiguous(), ops.conv_pack_weights(w, d, D_GEMM, True), b, d, D_GEMM, True, True, 0.1)
    assert not torch.equal(want, exact)
    g = dev(rand((N, Cout, 2 * H, 2 * W), 13))

    def grads():
        xg, wg, bg = x.detach().clone().requires_grad_(True), torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
        y = Fn.deconv_relu(xg, wg, bg, 0.1, True)
        assert y.requires_grad and y.grad_fn is not None
        (y * g).sum().backward()
        return y.detach(), xg.grad.clone(), wg.grad.clone(), bg.grad.clone()

    assert Fn.deconv_arithmetic() == "fp32" and Fn.conv_arithmetic() == "fp32"
    before = Fn.LIBRARY_FALLBACKS[0]
    y_off, gx_off, gw_off, gb_off = grads()
    assert torch.equal(y_off, exact)
    bwd_fallbacks = Fn.LIBRARY_FALLBACKS[0] - before
    before = Fn.LIBRARY_FALLBACKS[0]
    Fn.set_deconv_arithmetic("bf16x3")
    try:
        assert Fn.deconv_arithmetic() == "bf16x3" and Fn.conv_arithmetic() == "fp32"          # a switch of its own
        assert Fn.deconv_forward_route(d) == SPLIT
        assert Fn.conv_forward_route(ops.conv_desc(2, 12, 17, 28, 64, 5, 2, 2)) == DIRECT
        assert torch.equal(Fn.deconv_relu(x, w, b, 0.1, True), want)
        blob = torch.full((N, Cout + 7, 2 * H, 2 * W), float(SENTINEL), device="cuda")
        Fn.deconv_relu(x, w, b, 0.1, True, out=blob, out_c0=3)
        assert torch.equal(blob[:, 3:3 + Cout], want) and bool((blob[:, :3] == float(SENTINEL)).all()) and bool((blob[:, 3 + Cout:] == float(SENTINEL)).all())
        assert Fn.LIBRARY_FALLBACKS[0] == before             # the forward never falls back
        y_on, gx_on, gw_on, gb_on = grads()
        assert torch.equal(y_on, want) and Fn.LIBRARY_FALLBACKS[0] == before + bwd_fallbacks
        # every backward route stays exact fp32: where the two forwards agree in sign everywhere the gradients are the same bits
        assert torch.equal((y_on > 0), (y_off > 0))
        assert torch.equal(gx_on, gx_off) and torch.equal(gw_on, gw_off) and torch.equal(gb_on, gb_off)
        with pytest.raises(ValueError):
            Fn.set_deconv_arithmetic("bf16")
        assert Fn.deconv_arithmetic() == "bf16x3"
        Fn.set_conv_arithmetic("bf16x3")                     # ... and the other switch does not move this one
        try:
            assert Fn.deconv_arithmetic() == "bf16x3" and Fn.conv_arithmetic() == "bf16x3"
            Fn.set_deconv_arithmetic("fp32")
            assert Fn.conv_arithmetic() == "bf16x3" and Fn.deconv_forward_route(d) == D_GEMM
            assert Fn.conv_forward_route(ops.conv_desc(2, 12, 17, 28, 64, 5, 2, 2)) == (DIRECT | BIT)
        finally:
            Fn.set_conv_arithmetic("fp32")
    finally:
        Fn.set_deconv_arithmetic("fp32")
    assert Fn.deconv_arithmetic() == "fp32" and Fn.deconv_forward_route(d) == D_GEMM
    assert torch.equal(Fn.deconv_relu(x, w, b, 0.1, True), exact)
    keys = [key for key in Fn._PACKED_T if key[0] == id(w) and key[1][0] == "fwd"]
    assert sorted(key[1][1] for key in keys) == [D_GEMM, SPLIT]
    assert Fn.LIBRARY_FALLBACKS[0] == before + bwd_fallbacks


def smallest_flownetc_with_split_deconv():
    """(batch, H, W) with the fewest pixels at which some Deconvolution of FlowNetC takes the combined route through functional.deconv_relu
    and every Convolution / Deconvolution of the graph runs on a kernel of this library (found on the host).  The second condition: on 64-
    and 64 x 128-pixel inputs conv6's map is 1 or 2 pixels, fn2_deconv_route has nothing for deconv5 and upsample_flow6to5 there, and they go
    to the counted library convolution, which does not return the same bits from run to run -- in exact fp32 either (measured: three fp32
    forwards at 1 x 64 x 64 gave three results).  Reproducibility is a claim about this library's kernels."""
    from flownet2_amd import functional as Fn
    sizes = sorted(((B * H * W, B, H, W) for B in (1, 2) for H in range(64, 449, 64) for W in range(64, 513, 64)))
    Fn.set_deconv_arithmetic("bf16x3")
    try:
        for _, B, H, W in sizes:
            split, own = False, True
            for l in flownetc_training_layers(B, H, W):
                d, tr = ops.conv_desc(*l[2:]), l[1] == "deconv"
                lib = deconv_route(d) if tr else int(_lib.lib().fn2_conv_route(C.byref(d), 0))
                served = (Fn.deconv_forward_route(d) if tr else Fn.conv_forward_route(d)) != 0
                own = own and (served or lib == (D_HEAD if tr else HEAD))          # (the 2-channel heads have entry points of their own)
                split = split or (tr and Fn.deconv_forward_route(d) == SPLIT)
            if split and own:
                return B, H, W
    finally:
        Fn.set_deconv_arithmetic("fp32")
    raise AssertionError("no size routes a deconvolution to the GEMM")


@pytest.mark.gpu
def test_flownetc_end_to_end(monkeypatch):
    from flownet2_amd import functional as Fn
    B, H, W = smallest_flownetc_with_split_deconv()
    print("FlowNetC at batch %d, %d x %d" % (B, W, H))
    calls = []
    fwd = ops.conv_forward

    def recorded(x, packed, bias, desc, route, transposed=False, *a, **k):
        calls.append((int(route), bool(transposed)))
        return fwd(x, packed, bias, desc, route, transposed, *a, **k)

    monkeypatch.setattr(ops, "conv_forward", recorded)
    P = {k: v.cuda() for k, v in nets.init_params("C", 0).items()}
    rng = np.random.default_rng(5)
    i0 = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)).cuda()
    i1 = torch.roll(i0, (2, -3), (2, 3)).contiguous()
    assert Fn.conv_arithmetic() == "fp32" and Fn.deconv_arithmetic() == "fp32"
    epd = lambda a, b: float(((a - b) ** 2).sum(1).sqrt().mean())
    with torch.no_grad():
        exact = nets.deploy_forward("C", P, i0, i1, Fn)
        assert calls and not any(r & BIT for r, _ in calls)
        del calls[:]
        Fn.set_deconv_arithmetic("bf16x3")
        try:
            split = nets.deploy_forward("C", P, i0, i1, Fn)
            took = [(r, tr) for r, tr in calls if r & BIT]
            again = nets.deploy_forward("C", P, i0, i1, Fn)
            Fn.set_conv_arithmetic("bf16x3")
            try:
                both = nets.deploy_forward("C", P, i0, i1, Fn)
            finally:
                Fn.set_conv_arithmetic("fp32")
        finally:
            Fn.set_deconv_arithmetic("fp32")
    assert took and all(r == SPLIT and tr for r, tr in took)
    assert torch.equal(split, again)
    e1, e2 = epd(split, exact), epd(both, exact)
    print("mean end-point difference vs fp32: deconvolutions in bf16x3 %.3e px (%d layer calls), convolutions too %.3e px" % (e1, len(took), e2))
    assert np.isfinite(e1) and e1 <= 1e-4, e1
    assert np.isfinite(e2) and e2 <= 1e-4, e2
