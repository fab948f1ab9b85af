"""Split-bf16 ("bf16x3") arithmetic of the stride-2 data gradient (csrc/tconv_bf16x3.hip): FN2_CONV_ARITH_BF16X3 beside FN2_BWD_ROUTE_TCONV,
fn2_conv_backward_data_route_flags, functional.set_conv_backward_arithmetic.

Host: what the route function returns with and without the flag, the operand sizes, the production layers that change.  GPU: the fp64 bound
of the exact transposed-convolution route (TOL[TCONV] = 1e-5 x scale) plain and masked on five shapes, three inputs whose result is exact
and needs each of the six piece products, the masked form, blob forms, reproducibility (runs, batch, tile variants), refusals decided on the
host, non-finite inputs, the Python layer, and a small FlowNetC training step against the branch-pinned fp64 graph.

Measured on an MI355X, error / bound of test_fp64_bound (plain, masked): A 0.105, 0.105; B 0.044, 0.042; C 0.139, 0.158; D 0.020, 0.015;
wide 0.023, 0.021.

The route computes exactly Cin channels (Cin % 64 == 0 is what the TCONV route asks for), so it has no padded path through the workspace:
a bottom_room below the computed channels is an argument error, decided on the host, in either arithmetic."""
import ctypes as C

import numpy as np
import pytest
import torch

from flownet2_amd import Fn2Error, _lib, nets, ops
from flownet2_amd._lib import check
from bf16x3_helpers import BIT, F_BF16X3, forced_variants, host
from test_conv_backward_routes import DGRAD, TOL, dev, flownetc_training_layers, rand, same_bits, scale_of

NONE, WINOGRAD, TCONV, PLANE, DIRECT, DECONV_PLANE = 0, 1, 2, 3, 4, 5        # FN2_BWD_ROUTE_*
SPLIT = TCONV | BIT
SENTINEL = np.float32(-7.25)
KST = 13                            # k-steps per chunk of 16 top_diff channels: the 9 / 6 / 6 / 4 taps of the four parity classes in pairs
# convolution descriptors (N, Cin, H, W, Cout), all 5x5 / 2 / 2; top_diff is [N, Cout, Ht, Wt]
SHAPES = {
    "A": (2, 64, 16, 24, 96),       # the existing tconv-5x5 class
    "B": (1, 64, 17, 32, 40),       # odd bottom height; 40 top_diff channels: 2.5 chunks of 16
    "C": (2, 128, 20, 32, 256),     # reduction length 256 x 9, as for conv3
    "D": (1, 64, 9, 7, 8),          # odd bottom width: the mask read and the store take their scalar tails; half a chunk
}
# the tile variants are 32x4 and 16x8 class positions (= top_diff pixels): one shape whose top_diff (5 x 68) is wider than two of the widest
# tile: 3 / 5 tile columns, the last hanging over
SHAPES["wide"] = (1, 64, 9, 136, 16)
WIDEST_TILE = 32


def desc(name, N=None):
    n, Cin, H, W, Cout = SHAPES[name]
    return ops.conv_desc(n if N is None else N, Cin, H, W, Cout, 5, 2, 2)


def top_hw(name):
    _, _, H, W, _ = SHAPES[name]
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def route_flags(d, tr=0, flags=0):
    return int(_lib.lib().fn2_conv_backward_data_route_flags(C.byref(d), int(tr), flags))


def route_plain(d, tr=0):
    return int(_lib.lib().fn2_conv_backward_data_route(C.byref(d), int(tr)))


def floats(d, route, tr=0):
    return int(_lib.lib().fn2_conv_backward_data_packed_weight_floats(C.byref(d), int(tr), route))


def layout_floats(Cin, Cout):
    """three bf16 planes of [Cin / 16 groups][13 k-steps per chunk of 16 top_diff channels + 1][64 lanes][8]"""
    return (Cin // 16) * (KST * ((Cout + 15) // 16) + 1) * 3 * 64 * 4


def ref64(top, w, H, W):
    Ht, Wt = top.shape[2:]
    op = (H - (2 * (Ht - 1) + 1), W - (2 * (Wt - 1) + 1))
    return torch.nn.functional.conv_transpose2d(torch.from_numpy(top).double(), torch.from_numpy(w).double(), None, stride=2, padding=2,
                                                output_padding=op).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# host


def dgrad_desc(name, N=None):
    _, tr, n, Cin, H, W, Cout, k, s, p = DGRAD[name]
    return ops.conv_desc(n if N is None else N, Cin, H, W, Cout, k, s, p), int(tr)


def takes(d, tr):
    """the class this pull request routes: TCONV layers of kernel 5 / stride 2 / pad 2"""
    return route_plain(d, tr) == TCONV and not tr and (d.kernel, d.stride, d.pad) == (5, 2, 2)


def test_route_flag_changes_tconv_5x5_layers_only():
    L = _lib.lib()
    cases = [(n,) + dgrad_desc(n) for n in DGRAD]
    cases += [(l[0], ops.conv_desc(*l[2:]), int(l[1] == "deconv")) for l in flownetc_training_layers()]
    changed = []
    for name, d, tr in cases:
        plain = route_plain(d, tr)
        if name in DGRAD:
            assert plain == DGRAD[name][0], name
        assert route_flags(d, tr, 0) == plain, name              # flags 0: exactly fn2_conv_backward_data_route
        assert route_flags(d, tr, 1) == plain, name              # FN2_ROUTE_FORCE means nothing here
        want = SPLIT if takes(d, tr) else plain
        assert route_flags(d, tr, F_BF16X3) == want, name
        assert bool(L.fn2_tconv_bf16x3_supported(C.byref(d), tr)) == (want == SPLIT), name
        if want != plain:
            changed.append(name)
        if tr or plain != TCONV:                                  # every non-TCONV route and every transposed layer: unchanged
            assert route_flags(d, tr, F_BF16X3) == plain, name
    assert "tconv-5x5" in changed and "tconv-5x5-c128" in changed and "conv2" in changed and "conv3" in changed
    assert "tconv-3x3-odd" not in changed and "tconv-3x3-9x7" not in changed and "conv4" not in changed        # the 3x3 / 2 / 1 class stays exact
    for s in SHAPES:
        assert route_plain(desc(s)) == TCONV and route_flags(desc(s), 0, F_BF16X3) == SPLIT, s
    # the same in batch-invariant mode and for every batch
    was = ops.get_batch_invariant()
    try:
        for inv in (False, True):
            ops.set_batch_invariant(inv)
            for s in SHAPES:
                assert {route_flags(desc(s, N=n), 0, F_BF16X3) for n in (1, 2, 3, 8, 64)} == {SPLIT}, (s, inv)
                assert {route_flags(desc(s, N=n), 0, 0) for n in (1, 2, 3, 8, 64)} == {TCONV}, (s, inv)
            for name, d, tr in cases:
                assert route_flags(d, tr, F_BF16X3) == (SPLIT if takes(d, tr) else route_plain(d, tr)), (name, inv)
    finally:
        ops.set_batch_invariant(was)
    assert ops.conv_backward_data_route(desc("A"), False, bf16x3=True) == SPLIT and ops.conv_backward_data_route(desc("A"), False) == TCONV
    assert ops.conv_backward_data_route(desc("A")) == TCONV


def test_operand_sizes():
    L = _lib.lib()
    for s in SHAPES:
        d = desc(s)
        n, Cin, H, W, Cout = SHAPES[s]
        assert floats(d, SPLIT) > 0 and floats(d, TCONV) > 0 and floats(d, SPLIT) != floats(d, TCONV), s
        assert floats(d, SPLIT) == layout_floats(Cin, Cout), s
        assert floats(d, WINOGRAD | BIT) == 0 and floats(d, PLANE | BIT) == 0 and floats(d, BIT) == 0 and floats(d, DIRECT | BIT) == 0, s
        assert floats(d, SPLIT, tr=1) == 0, s
        for r in (SPLIT, PLANE | BIT, BIT):
            assert L.fn2_conv_backward_data_workspace_bytes(C.byref(d), 0, r) == 0
            assert L.fn2_conv_backward_data_pack_workspace_bytes(C.byref(d), 0, r) == 0
        assert L.fn2_conv_backward_data_workspace_bytes_with_room(C.byref(d), 0, SPLIT, Cin) == 0
        assert L.fn2_conv_backward_data_computed_channels(C.byref(d), 0, SPLIT) == Cin == L.fn2_conv_backward_data_computed_channels(C.byref(d), 0, TCONV)
        assert L.fn2_conv_backward_data_computed_channels(C.byref(d), 0, BIT) == 0 and L.fn2_conv_backward_data_computed_channels(C.byref(d), 0, PLANE | BIT) == 0
        assert L.fn2_conv_backward_data_masked_supported(C.byref(d), 0, SPLIT) == 1 and L.fn2_conv_backward_data_masked_supported(C.byref(d), 0, TCONV) == 1
        assert L.fn2_conv_backward_data_masked_supported(C.byref(d), 0, BIT) == 0 and L.fn2_conv_backward_data_masked_supported(C.byref(d), 0, WINOGRAD | BIT) == 0
    # layers the kernel refuses: the 3x3 / 2 / 1 class of the TCONV route, every other route, the Deconvolution routes
    for name in DGRAD:
        d, tr = dgrad_desc(name)
        if not takes(d, tr):
            assert floats(d, SPLIT, tr) == 0 and floats(d, DGRAD[name][0] | BIT, tr) == 0 and L.fn2_tconv_bf16x3_supported(C.byref(d), tr) == 0, name
            assert L.fn2_conv_backward_data_computed_channels(C.byref(d), tr, DGRAD[name][0] | BIT) == 0, name
        assert floats(d, DGRAD[name][0], tr) > 0, name
    assert L.fn2_tconv_bf16x3_supported(C.byref(ops.conv_desc(2, 32, 16, 24, 96, 5, 2, 2)), 0) == 0          # 64-channel workgroup tiles
    assert L.fn2_tconv_bf16x3_supported(C.byref(ops.conv_desc(2, 64, 16, 20, 96, 5, 2, 2)), 0) == 0          # top_diff rows of whole 16-byte pieces
    assert L.fn2_tconv_bf16x3_supported(C.byref(ops.conv_desc(2, 64, 16, 24, 96, 5, 2, 1)), 0) == 0
    assert L.fn2_tconv_bf16x3_supported(C.byref(desc("A")), 1) == 0 and L.fn2_tconv_bf16x3_supported(None, 0) == 0
    assert L.fn2_tconv_bf16x3_num_variants() >= 2
    Wt = top_hw("wide")[1]
    assert Wt > 2 * WIDEST_TILE and Wt % WIDEST_TILE != 0 and Wt % 16 != 0


def test_production_layers_that_change_are_conv2_and_conv3():
    took = set()
    for (name, kind, n, ci, h, w, co, k, s, p) in flownetc_training_layers():          # batch 8 @448x320
        d, tr = ops.conv_desc(n, ci, h, w, co, k, s, p), int(kind == "deconv")
        plain, flagged = route_plain(d, tr), route_flags(d, tr, F_BF16X3)
        if flagged & BIT:
            assert flagged == SPLIT and plain == TCONV and floats(d, SPLIT, tr) == layout_floats(ci, co) != floats(d, TCONV, tr)
            took.add(name)
        else:
            assert flagged == plain, name
    assert took == {"conv2", "conv3"}


def test_switch_is_its_own_and_reads_the_environment(monkeypatch):
    import subprocess
    import sys
    from flownet2_amd import functional as Fn
    assert Fn.conv_backward_arithmetic() == "fp32"
    try:
        Fn.set_conv_backward_arithmetic("bf16x3")
        assert Fn.conv_backward_arithmetic() == "bf16x3" and Fn.conv_arithmetic() == "fp32" and Fn.deconv_arithmetic() == "fp32"
        assert Fn.arithmetic("dgrad") == Fn.conv_backward_arithmetic() and Fn.winograd_arithmetic() == Fn.get_winograd_arithmetic() == "fp32"
        with pytest.raises(ValueError):
            Fn.set_conv_backward_arithmetic("bf16")
        assert Fn.conv_backward_arithmetic() == "bf16x3"
    finally:
        Fn.set_conv_backward_arithmetic("fp32")
    Fn.set_conv_arithmetic("bf16x3")
    try:
        assert Fn.conv_backward_arithmetic() == "fp32"
    finally:
        Fn.set_conv_arithmetic("fp32")
    code = "from flownet2_amd import functional as Fn; print(Fn.conv_backward_arithmetic(), Fn.conv_arithmetic())"
    import os
    env = dict(os.environ, FN2_DGRAD_ARITH="bf16x3")
    env.pop("FN2_CONV_ARITH", None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["bf16x3", "fp32"], (out.stdout, out.stderr)
    env["FN2_DGRAD_ARITH"] = "bf16"
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True)
    assert out.returncode != 0 and "ValueError" in out.stderr


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU


def inputs(name, N=None):
    n, Cin, H, W, Cout = SHAPES[name]
    Ht, Wt = top_hw(name)
    return rand((n if N is None else N, Cout, Ht, Wt), 1), rand((Cout, Cin, 5, 5), 2, 0.1)


def pack(name, w, route=SPLIT, N=None):
    return ops.conv_backward_data_pack_weights(dev(w), desc(name, N), False, route)


def mask_of(name, N=None, seed=5):
    """The layer's bottom = the activated output of the layer in front, as channels [4, 4 + Cin) of a wider blob: +x, -x, 0.0 and -0.0."""
    n, Cin, H, W, _ = SHAPES[name]
    y = rand((n if N is None else N, Cin + 6, H, W), seed)
    flat = y.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return y


def raw_plain(d, route, top, top_ch, top_c0, packed, out, out_ch, out_c0, room, null=()):
    ptr = {"top": ops._ptr(top), "packed": ops._ptr(packed), "out": ops._ptr(out)}
    for n in null:
        ptr[n] = None
    try:
        check(_lib.lib().fn2_conv_backward_data(C.byref(d), 0, int(route), ptr["top"], top_ch, top_c0, ptr["packed"], ptr["out"], out_ch, out_c0, room,
                                                None, 0, ops._stream()))
    finally:
        torch.cuda.synchronize()


def raw_masked(d, route, top, top_ch, top_c0, packed, out, out_ch, out_c0, y, y_ch, y_c0, slope, null=()):
    ptr = {"top": ops._ptr(top), "packed": ops._ptr(packed), "out": ops._ptr(out), "mask": ops._ptr(y)}
    for n in null:
        ptr[n] = None
    try:
        check(_lib.lib().fn2_conv_backward_data_masked(C.byref(d), 0, int(route), ptr["top"], top_ch, top_c0, ptr["packed"], ptr["out"], out_ch, out_c0,
                                                       ptr["mask"], y_ch, y_c0, C.c_float(slope), ops._stream()))
    finally:
        torch.cuda.synchronize()


def run(name, packed, top, N=None, route=SPLIT):
    """the plain call on whole blobs"""
    n, Cin, H, W, Cout = SHAPES[name]
    n = n if N is None else N
    t = dev(top)
    out = torch.full((n, Cin, H, W), float(SENTINEL), device="cuda")
    raw_plain(desc(name, N), route, t, t.shape[1], 0, packed, out, Cin, 0, Cin)
    return host(out)


def run_masked(name, packed, top, y_blob, y_c0, slope, N=None, route=SPLIT):
    n, Cin, H, W, Cout = SHAPES[name]
    n = n if N is None else N
    t, y = dev(top), dev(y_blob)
    out = torch.full((n, Cin, H, W), float(SENTINEL), device="cuda")
    raw_masked(desc(name, N), route, t, t.shape[1], 0, packed, out, Cin, 0, y, y.shape[1], y_c0, slope)
    return host(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp64_bound(name):
    """error / bound (plain, masked), measured on an MI355X: A 0.105, 0.105; B 0.044, 0.042; C 0.139, 0.158; D 0.020, 0.015; wide 0.023,
    0.021 (the exact route on the same inputs: A 0.089, B 0.069, C 0.169, D 0.021, wide 0.049)."""
    n, Cin, H, W, Cout = SHAPES[name]
    top, w = inputs(name)
    packed = pack(name, w)
    ref = ref64(top, w, H, W)
    got = run(name, packed, top)
    assert got.shape == ref.shape
    ratio = float(np.abs(got - ref).max()) / (TOL[TCONV] * scale_of(ref))
    print("dgrad bf16x3 fp64 error / bound: %s plain: %.3f" % (name, ratio))
    y = mask_of(name)
    slope = 0.1
    refm = ref * np.where(y[:, 4:4 + Cin] > 0, 1.0, slope)
    gotm = run_masked(name, packed, top, y, 4, slope)
    ratiom = float(np.abs(gotm - refm).max()) / (TOL[TCONV] * scale_of(refm))
    print("dgrad bf16x3 fp64 error / bound: %s masked: %.3f" % (name, ratiom))
    exact = run(name, pack(name, w, TCONV), top, route=TCONV)
    print("exact route fp64 error / bound: %s plain: %.3f" % (name, float(np.abs(exact - ref).max()) / (TOL[TCONV] * scale_of(ref))))
    assert ratio <= 1.0, (name, ratio)
    assert ratiom <= 1.0, (name, ratiom)


def exact_inputs(kind):
    N, Cin, H, W, Cout = SHAPES["A"]
    Ht, Wt = top_hw("A")
    rng = np.random.default_rng(11)
    if kind == "select-top":        # needs hh, mh, lh: one weight per bottom channel
        top = rand((N, Cout, Ht, Wt), 21)
        w = np.zeros((Cout, Cin, 5, 5), np.float32)
        w[rng.integers(0, Cout, Cin), np.arange(Cin), rng.integers(0, 5, Cin), rng.integers(0, 5, Cin)] = rng.choice([1.0, -1.0, 0.5, -2.0], Cin)
        return top, w
    if kind == "select-w":          # needs hh, hm, hl: at most one nonzero top_diff pixel in the 3x3 pixels a bottom pixel gathers from
        w = rand((Cout, Cin, 5, 5), 22, 0.1)
        top = np.zeros((N, Cout, Ht, Wt), np.float32)
        for n in range(N):
            for y in range(n, Ht, 3):
                for x in range(2 * n, Wt, 3):
                    top[n, (3 * y + 5 * x + n) % Cout, y, x] = rng.choice([1.0, -1.0, 2.0, -0.5])
        return top, w
    # mid-x-mid: needs mm
    top = (1.0 + rng.integers(0, 4, (N, Cout, Ht, Wt)) / 1024.0).astype(np.float32)
    w = np.zeros((Cout, Cin, 5, 5), np.float32)
    for cb in range(Cin):
        for f in rng.choice(Cout * 25, 4, replace=False):
            w[f // 25, cb].reshape(-1)[f % 25] = rng.choice([1.0, -1.0]) * (1.0 + rng.integers(0, 4) / 1024.0)
    return top, w


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["select-top", "select-w", "mid-x-mid"])
def test_exact_values(kind):
    N, Cin, H, W, Cout = SHAPES["A"]
    top, w = exact_inputs(kind)
    ref = ref64(top, w, H, W)
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref) and np.abs(ref).max() > 0.5          # the reference is itself an fp32 value
    if kind == "mid-x-mid":
        assert (np.round(top * 1024) % 4 != 0).any() and np.abs(ref).max() < 8
    got = run("A", pack("A", w), top)
    assert same_bits(got + np.float32(0.0), ref32 + np.float32(0.0)), (kind, float(np.abs(got - ref32).max()))      # (+ 0.0: -0.0 == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "D"])
def test_masked_form(name):
    n, Cin, H, W, Cout = SHAPES[name]
    top, w = inputs(name)
    packed = pack(name, w)
    plain = run(name, packed, top)
    y = mask_of(name)
    yv = y[:, 4:4 + Cin]
    for slope in (0.1, 0.0):
        want = plain * np.where(yv > 0, np.float32(1.0), np.float32(slope))          # bias_leaky_relu_bwd's expression, fp32
        got = run_masked(name, packed, top, y, 4, slope)                              # the mask as channels [4, 4 + Cin) of a wider blob
        assert same_bits(got, want), (name, slope)
        assert same_bits(run_masked(name, packed, top, np.ascontiguousarray(yv), 0, slope), want), (name, slope)
    z = yv == 0
    assert z.any() and np.signbit(yv[z]).any() and np.abs(plain[z]).max() > 0          # the zeros of either sign take the slope
    # ops wrapper
    d = desc(name)
    assert ops.conv_backward_data_masked_supported(d, False, SPLIT)
    got = ops.conv_backward_data_masked(dev(top), packed, d, False, SPLIT, dev(y), 0.1, data_c0=4)
    assert same_bits(host(got), plain * np.where(yv > 0, np.float32(1.0), np.float32(0.1)))


@pytest.mark.gpu
def test_blob_forms():
    N, Cin, H, W, Cout = SHAPES["A"]
    Ht, Wt = top_hw("A")
    top, w = inputs("A")
    packed = pack("A", w)
    d = desc("A")
    base = run("A", packed, top)
    assert not (base == SENTINEL).any()
    wide = rand((N, Cout + 8, Ht, Wt), 9)
    wide[:, 5:5 + Cout] = top
    L = _lib.lib()
    Cp = int(L.fn2_conv_backward_data_computed_channels(C.byref(d), 0, SPLIT))
    assert Cp == Cin
    for top_slice, out_slice, room in [(True, False, Cp), (False, True, Cp), (True, True, Cp), (True, True, Cp + 2)]:
        t = dev(wide if top_slice else top)
        out = torch.full((N, Cin + 7 if out_slice else Cin, H, W), float(SENTINEL), device="cuda")
        if room > Cp and not out_slice:
            continue
        raw_plain(d, SPLIT, t, t.shape[1], 5 if top_slice else 0, packed, out, out.shape[1], 3 if out_slice else 0, room)
        got = host(out)
        if out_slice:
            assert (got[:, :3] == SENTINEL).all() and (got[:, 3 + Cin:] == SENTINEL).all(), (top_slice, out_slice, room)
            got = got[:, 3:3 + Cin]
        assert same_bits(got, base), (top_slice, out_slice, room)
    # a bottom_room below the computed channels: the route computes exactly Cin channels and has no padded path; refused on the host
    out = torch.full((N, Cin + 7, H, W), float(SENTINEL), device="cuda")
    for route, op in ((SPLIT, packed), (TCONV, pack("A", w, TCONV))):
        with pytest.raises(Fn2Error):
            raw_plain(d, route, dev(top), Cout, 0, op, out, Cin + 7, 3, Cp - 1)
        assert bool((out == float(SENTINEL)).all())
    # the ops wrapper: the same bits
    assert same_bits(host(ops.conv_backward_data(dev(wide), packed, d, False, SPLIT, top_c0=5)), base)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_reproducible_across_runs_batch_and_variants(name):
    L = _lib.lib()
    n, Cin, H, W, Cout = SHAPES[name]
    top, w = inputs(name, N=3)
    y = mask_of(name, N=3)
    packed = pack(name, w, N=3)
    batch = run(name, packed, top, N=3)
    masked = run_masked(name, packed, top, y, 4, 0.1, N=3)
    assert same_bits(run(name, packed, top, N=3), batch)
    assert same_bits(run(name, pack(name, w, N=1), top[:1], N=1), batch[:1])
    was = ops.get_batch_invariant()
    ops.set_batch_invariant(True)
    try:
        assert same_bits(run(name, packed, top, N=3), batch)
        assert same_bits(run(name, packed, top[:1], N=1), batch[:1])
    finally:
        ops.set_batch_invariant(was)
    ran = 0
    with forced_variants("tconv_bf16x3") as (nv, force):
        for v in range(nv):
            force(v)
            assert same_bits(run(name, packed, top, N=3), batch), v          # (every variant applies: they all block 64 channels)
            assert same_bits(run_masked(name, packed, top, y, 4, 0.1, N=3), masked), v
            ran += 1
        force(nv)                       # one past the last
        with pytest.raises(Fn2Error):
            run(name, packed, top, N=3)
    assert ran == nv >= 2


@pytest.mark.gpu
def test_refusals_are_decided_on_the_host():
    N, Cin, H, W, Cout = SHAPES["A"]
    Ht, Wt = top_hw("A")
    d = desc("A")
    top = dev(rand((N, Cout + 8, Ht, Wt), 4))
    w = rand((Cout, Cin, 5, 5), 2, 0.1)
    split_op, exact_op = pack("A", w), pack("A", w, TCONV)
    y = dev(mask_of("A"))
    out = torch.full((N, Cin + 8, H, W), float(SENTINEL), device="cuda")
    untouched = lambda: bool((out == float(SENTINEL)).all())
    d3 = ops.conv_desc(N, Cin, H, W, Cout, 3, 2, 1)          # a TCONV layer of the other class: bottom and top_diff of the same sizes
    assert route_plain(d3) == TCONV and ((H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1) == (Ht, Wt)
    calls = {
        "3x3 / 2 / 1 descriptor": dict(d=d3), "WINOGRAD | 0x100": dict(route=WINOGRAD | BIT), "PLANE | 0x100": dict(route=PLANE | BIT),
        "DIRECT | 0x100": dict(route=DIRECT | BIT), "0x100 alone": dict(route=BIT),
        "null top_diff": dict(null=("top",)), "null operand": dict(null=("packed",)), "null bottom_diff": dict(null=("out",)),
        "top_diff slice past its blob": dict(top_ch=Cout + 1, top_c0=2), "bottom_diff slice past its blob": dict(out_ch=Cin + 2, out_c0=3),
        "negative bottom slice": dict(out_c0=-1), "negative top slice": dict(top_c0=-1),
    }
    for what, kw in calls.items():
        a = dict(d=d, route=SPLIT, top_ch=Cout + 8, top_c0=0, out_ch=Cin + 8, out_c0=0, null=())
        a.update(kw)
        with pytest.raises(Fn2Error):
            raw_plain(a["d"], a["route"], top, a["top_ch"], a["top_c0"], split_op, out, a["out_ch"], a["out_c0"], Cin, a["null"])
            pytest.fail("%s was not refused" % what)
        assert untouched(), what
        if "out" in a["null"]:
            continue
        with pytest.raises(Fn2Error):
            raw_masked(a["d"], a["route"], top, a["top_ch"], a["top_c0"], split_op, out, a["out_ch"], a["out_c0"], y, Cin + 6, 4, 0.1, a["null"])
            pytest.fail("%s was not refused (masked)" % what)
        assert untouched(), what
    for what, kw in {"null mask": dict(null=("mask",)), "mask slice past its blob": dict(y_ch=Cin + 3)}.items():
        with pytest.raises(Fn2Error):
            raw_masked(d, SPLIT, top, Cout + 8, 0, split_op, out, Cin + 8, 0, y, kw.get("y_ch", Cin + 6), 4, 0.1, kw.get("null", ()))
        assert untouched(), what
    # too small a bottom_room
    with pytest.raises(Fn2Error):
        raw_plain(d, SPLIT, top, Cout + 8, 0, split_op, out, Cin + 8, 0, Cin - 1)
    assert untouched()
    # an operand packed for the other arithmetic: the length check of the ops wrappers
    ts = top[:, :Cout].contiguous()
    for operand, route in ((exact_op, SPLIT), (split_op, TCONV)):
        with pytest.raises(ValueError):
            ops.conv_backward_data(ts, operand, d, False, route)
        with pytest.raises(ValueError):
            ops.conv_backward_data_masked(ts, operand, d, False, route, y, 0.1, data_c0=4)
    with pytest.raises(ValueError):
        ops.conv_backward_data_pack_weights(dev(rand((Cout, Cin, 3, 3), 2)), d3, False, SPLIT)
    for r in (WINOGRAD | BIT, PLANE | BIT, BIT):
        with pytest.raises(ValueError):
            ops.conv_backward_data_pack_weights(dev(w), d, False, r)
        with pytest.raises(ValueError):
            ops.conv_backward_data(ts, split_op, d, False, r)
        assert not ops.conv_backward_data_masked_supported(d, False, r)
    with pytest.raises(Fn2Error):
        check(_lib.lib().fn2_conv_backward_data_pack_weights(C.byref(d), 0, PLANE | BIT, ops._ptr(dev(w)), ops._ptr(split_op), None, 0, ops._stream()))
    with pytest.raises(Fn2Error):
        check(_lib.lib().fn2_conv_backward_data_pack_weights(C.byref(d), 1, SPLIT, ops._ptr(dev(w)), ops._ptr(split_op), None, 0, ops._stream()))
    torch.cuda.synchronize()
    assert same_bits(host(split_op), host(pack("A", w)))          # (the refused pack calls wrote nothing)
    # ... and the call none of this applies to writes exactly the layer's channels
    raw_plain(d, SPLIT, top, Cout + 8, 0, split_op, out, Cin + 8, 0, Cin)
    assert not bool((out[:, :Cin] == float(SENTINEL)).any()) and bool((out[:, Cin:] == float(SENTINEL)).all())


@pytest.mark.gpu
def test_non_finite_inputs_reach_their_own_taps_only():
    n, Cin, H, W, Cout = SHAPES["B"]
    N = 2
    Ht, Wt = top_hw("B")
    top, w = inputs("B", N=N)
    assert (w != 0).all()
    packed = pack("B", w, N=N)
    clean = run("B", packed, top, N=N)
    assert np.isfinite(clean).all()
    bad = top.copy()
    spots = [(0, 3, 4, 7, np.inf), (1, 37, 8, 13, np.nan)]          # channel 37: the ragged third chunk.  Different samples
    covered = np.zeros((N, H, W), bool)
    for (s, c, yy, xx, v) in spots:
        bad[s, c, yy, xx] = v
        for ky in range(5):
            for kx in range(5):
                Y, X = 2 * yy - 2 + ky, 2 * xx - 2 + kx
                if 0 <= Y < H and 0 <= X < W:
                    covered[s, Y, X] = True
    assert 0 < covered.sum() < covered.size // 4
    got = run("B", packed, bad, N=N)
    mask = np.broadcast_to(covered[:, None], got.shape)
    assert np.array_equal(~np.isfinite(got), mask)
    assert np.array_equal(got.view(np.uint32)[~mask], clean.view(np.uint32)[~mask])


@pytest.mark.gpu
def test_python_layer(monkeypatch):
    from flownet2_amd import functional as Fn
    monkeypatch.delenv("FN2_STRICT", raising=False)
    N, Cin, H, W, Cout = 2, 64, 16, 24, 128                # tconv-5x5-c128: a layer with a forward kernel of its own
    Ht, Wt = 8, 12
    d = ops.conv_desc(N, Cin, H, W, Cout, 5, 2, 2)
    assert route_flags(d, 0, F_BF16X3) == SPLIT
    w, b = dev(rand((Cout, Cin, 5, 5), 2, 0.1)), dev(rand((Cout,), 3, 0.1))
    wide = dev(rand((N, Cin + 5, H, W), 9))
    x = wide[:, 2:2 + Cin]
    g = dev(rand((N, Cout, Ht, Wt), 13))

    def grads():
        xg, wg, bg = x.detach().clone().requires_grad_(True), torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
        y = Fn.conv_mfma_relu(xg, wg, bg, 2, 2, 0.1, True)
        (y * g).sum().backward()
        return y.detach(), xg.grad.clone(), wg.grad.clone(), bg.grad.clone()

    assert Fn.conv_backward_arithmetic() == "fp32" and Fn.conv_arithmetic() == "fp32"
    before = Fn.LIBRARY_FALLBACKS[0]
    y_off, gx_off, gw_off, gb_off = grads()
    off_fallbacks = Fn.LIBRARY_FALLBACKS[0] - before
    # the data gradient by hand: ReLUBackward of this layer's own activation, then the route called directly
    td = (g * torch.where(y_off > 0, torch.ones_like(g), torch.full_like(g, 0.1))).contiguous()
    want_exact = ops.conv_backward_data(td, ops.conv_backward_data_pack_weights(w, d, False, TCONV), d, False, TCONV)
    want_split = ops.conv_backward_data(td, ops.conv_backward_data_pack_weights(w, d, False, SPLIT), d, False, SPLIT)
    assert torch.equal(gx_off, want_exact) and not torch.equal(want_split, want_exact)
    before = Fn.LIBRARY_FALLBACKS[0]
    Fn.set_conv_backward_arithmetic("bf16x3")
    try:
        y_on, gx_on, gw_on, gb_on = grads()
        assert Fn.LIBRARY_FALLBACKS[0] - before == off_fallbacks
        assert torch.equal(y_on, y_off)                     # the forward is not this switch's
        assert torch.equal(gx_on, want_split)
        assert torch.equal(gw_on, gw_off) and torch.equal(gb_on, gb_off)
        assert Fn.relu_chain_supported((N, Cin, H, W), w, 2, 2)
    finally:
        Fn.set_conv_backward_arithmetic("fp32")
    y2, gx2, gw2, gb2 = grads()
    assert torch.equal(gx2, want_exact) and torch.equal(y2, y_off) and torch.equal(gw2, gw_off)
    assert Fn.relu_chain_supported((N, Cin, H, W), w, 2, 2)


def smallest_flownetc_with_split_conv2_and_conv3():
    """(batch, H, W) with the fewest pixels at which conv2's and conv3's data gradients take the split route (found on the host).  From
    128 x 128 on: the loss at 1/64 resolution downsamples the ground truth to a map that must be at least 2 x 2."""
    sizes = sorted(((B * H * W, B, H, W) for B in (1, 2) for H in range(128, 449, 64) for W in range(128, 513, 64)))
    for _, B, H, W in sizes:
        layers = {l[0]: l for l in flownetc_training_layers(B, H, W)}
        if all(route_flags(ops.conv_desc(*layers[n][2:]), 0, F_BF16X3) == SPLIT for n in ("conv2", "conv3")):
            return B, H, W
    raise AssertionError("no size routes conv2 and conv3 to the split data gradient")


@pytest.mark.gpu
def test_small_flownetc_training_step_matches_the_branch_pinned_fp64_graph():
    """Relative L2 error of the parameter gradients against the fp64 graph on the ReLU branches of the fp32 run (the forward is not the
    switch's: the branches are the same), with the bounds of test_fp64_graph_is_pinned_by_the_oracle_restatements: all values together
    <= 1e-5, the worst parameter <= 5e-5.  Measured on an MI355X at batch 1, 128 x 128: fp32 data gradients all 1.182e-06, worst 2.540e-06
    (upsample_flow6to5.b); bf16x3 data gradients all 1.189e-06, worst 2.547e-06 (conv1.b)."""
    from flownet2_amd import functional as Fn
    from oracle import fp64_graph
    from test_train_parity import _batch
    B, H, W = smallest_flownetc_with_split_conv2_and_conv3()
    print("FlowNetC training step at batch %d, %d x %d" % (B, W, H))
    cuda = torch.device("cuda:0")
    P = nets.init_params("C", seed=0)
    a, b, gt = _batch(B, H, W, 4)
    Pd = {k: v.to(cuda).requires_grad_(True) for k, v in P.items()}
    routes = []
    bwd, bwdm = ops.conv_backward_data, ops.conv_backward_data_masked

    def step():
        for v in Pd.values():
            v.grad = None
        pre = [(im.to(cuda) * (1.0 / 255.0)) - 0.43 for im in (a, b)]
        loss = nets.multiscale_loss(nets.flownet_c_core(Pd, pre[0], pre[1], Fn), gt.to(cuda), Fn)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: v.grad.detach().clone() for k, v in Pd.items()}

    assert Fn.conv_backward_arithmetic() == "fp32"
    fallbacks = Fn.LIBRARY_FALLBACKS[0]
    with fp64_graph.record_relu_branches() as rec:
        loss_off, g_off = step()
    _, g_p = fp64_graph.flownetc_train_reference(P, a, b, gt, device=cuda, masks=rec.branches)
    off = fp64_graph.grad_agreement(g_off, g_p)
    ops.conv_backward_data = lambda t, p, d, tr, route, *aa, **k: routes.append(int(route)) or bwd(t, p, d, tr, route, *aa, **k)
    ops.conv_backward_data_masked = lambda t, p, d, tr, route, *aa, **k: routes.append(int(route)) or bwdm(t, p, d, tr, route, *aa, **k)
    Fn.set_conv_backward_arithmetic("bf16x3")
    try:
        with fp64_graph.record_relu_branches() as rec_on:
            loss_on, g_on = step()
        loss_again, g_again = step()
    finally:
        Fn.set_conv_backward_arithmetic("fp32")
        ops.conv_backward_data, ops.conv_backward_data_masked = bwd, bwdm
    assert Fn.LIBRARY_FALLBACKS[0] == fallbacks
    on = fp64_graph.grad_agreement(g_on, g_p)
    print("fp32 data gradients:   all %.3e, worst %.3e (%s)" % (off["all"], off["worst"], off["worst_name"]))
    print("bf16x3 data gradients: all %.3e, worst %.3e (%s); %d data-gradient calls in split arithmetic" %
          (on["all"], on["worst"], on["worst_name"], sum(1 for r in routes if r & BIT)))
    assert off["all"] <= 1e-5 and off["worst"] <= 5e-5, (off["all"], off["worst_name"], off["worst"])
    took = [r for r in routes if r & BIT]
    assert len(took) >= 4 and all(r == SPLIT for r in took)          # conv2 and conv3, two steps
    assert loss_on == loss_off and fp64_graph.relu_sign_flips(rec.branches, rec_on.branches)[0] == 0       # the forward is unchanged
    assert all(torch.equal(g_on[k], g_again[k]) for k in g_on)       # bit-reproducible
    changed = sorted(k for k in g_on if not torch.equal(g_on[k], g_off[k]))
    assert changed and all(k.split(".")[0] in ("conv1", "conv2") for k in changed), changed       # what lies in front of the two data gradients
    assert on["all"] <= 1e-5 and on["worst"] <= 5e-5, (on["all"], on["worst_name"], on["worst"])

