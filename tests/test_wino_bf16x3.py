"""Split-bf16 ("bf16x3") arithmetic of the Winograd F(2x2, 3x3) forward (csrc/conv_wino_bf16x3.hip): FN2_CONV_ARITH_BF16X3 beside
FN2_CONV_ROUTE_WINOGRAD, FN2_ROUTE_WINO_BF16X3 of fn2_conv_route, functional.set_winograd_arithmetic.

Host: what the route function returns with and without the flag, the operand sizes, the production layers that change, the switch; a
numpy emulation of the stated arithmetic (fp32 transforms in the kernel's order, exact three-way split, the six products mm, lh, hl, mh,
hm, hh in fp32) that meets the fp64 bound on the GPU tests' inputs and, on three constructed input families, needs each of the six
products and none of the dropped three.  GPU: the fp64 bound of the exact Winograd kernel (TOL[(False, WINOGRAD)] x scale, imported) on four
shapes under every flag combination with the exact route as control, the constructed inputs bit for bit, blob forms, reproducibility
(runs, batch, tile variants), refusals decided on the host, non-finite inputs, the Python layer, and a FlowNetC forward.

The GPU tests name the combined route: shapes this small are the small-map kernel's (PLANE) by fn2_conv_route at their own batch.

The constructed families.  Every output channel has ONE nonzero weight g (one input channel, one tap), so a Winograd position holds one
product V U per tile and the order of summation over channels plays no part; U = G g G^T is then g x {0, 1, 1/2, 1/4}.
  * "split-v": pixels k 2^-16 with |k| < 2^17, g a power of two.  V (sums of 4 pixels) has up to 19 significant bits: three nonzero
    pieces; U is one piece.  Needs hh, mh, lh.  |Y's partial sums| < 4 x 2^19 units of 2^-18 |g|: exact in fp32.
  * "split-u": one pixel of +-1, +-2, +-1/2 per 5x5 block (never two in a 4x4 patch), g = k 2^-12 with |k| < 2^18 odd.  V is 0 or
    +- the pixel: one piece; U has three.  Needs hh, hm, hl.  Partial sums < 4 x 2^18 units of |pixel| 2^-14: exact.
  * "mid-mid": pixels 1 + k / 256, g = +-(1 + j / 256), j in {1, 3}: V has at most 11 significant bits, U 9: two pieces each, no third.
    Needs mm (and hm, mh, hh).  Partial sums < 38 < 2^6 in units of 2^-18: exact.
In all three the dropped products ml, lm, ll are zero piece by piece, every piece product and every sum is exact, and the fp64
convolution is an fp32 number: the comparison on these inputs is bit equality, on the host and on the GPU.  Dropping hh, hm or mh moves
the result past the fp64 bound as well (terms of relative size >= 2^-9); hl, lh and mm are terms of relative size 2^-16 .. 2^-18 of a
value, at or below the bound of 6e-6 x scale -- only the exact comparison sees them, which is why the constructed inputs exist."""
import ctypes as C

import numpy as np
import pytest
import torch

from flownet2_amd import Fn2Error, _lib, nets, ops
from flownet2_amd._lib import check
from bf16x3_helpers import BIT, F_BF16X3, F_FORCE, forced_variants, host
from test_conv_backward_routes import dev, rand, same_bits, scale_of
from test_conv_forward_routes import DIRECT, FWD, PLANE, SENTINEL, TOL, WINOGRAD, flag_sets, production_layers

SPLIT = WINOGRAD | BIT
F_WINO = 4                                   # FN2_ROUTE_WINO_BF16X3
BOUND = TOL[(False, WINOGRAD)]               # the exact Winograd kernel's own fp64 bound
# (N, Cin, H, W, Cout), all 3x3 / 1 / 1.  The tile variants are 16x16 and 8x32 output pixels.
SHAPES = {
    "threshold": FWD["wino-threshold"][2:7],  # (3, 13, 65, 76, 64): ragged Cin below one k-step, odd height, several tiles both ways
    "small": (1, 40, 6, 8, 128),              # 2.5 k-steps, two 64-channel groups, narrower and shorter than every tile
    "wide": (1, 8, 5, 140, 64),               # wider than every tile, the last tile column ragged (140 = 8 x 16 + 12 = 4 x 32 + 12)
    "deep": (1, 473, 10, 12, 64),             # conv3_1's reduction length: 30 k-steps, the last one ragged
}
EXACT_SHAPE = (2, 12, 17, 28, 64)
KINDS = ["split-v", "split-u", "mid-mid"]
PRODUCTS = ["mm", "lh", "hl", "mh", "hm", "hh"]                  # the kernel's order; first letter: V's piece
DROPPED = ["ml", "lm", "ll"]


def desc_for(shape, N=None):
    n, Cin, H, W, Cout = shape
    return ops.conv_desc(n if N is None else N, Cin, H, W, Cout, 3, 1, 1)


def desc(name, N=None):
    return desc_for(SHAPES[name], N)


def lib_route(d, flags=0):
    return int(_lib.lib().fn2_conv_route(C.byref(d), flags))


def floats(d, route):
    return int(_lib.lib().fn2_conv_packed_weight_floats(C.byref(d), route))


def supported(d):
    return int(_lib.lib().fn2_conv_wino_bf16x3_supported(C.byref(d)))


def fwd_desc(n, N=None):
    _, tr, b, Cin, H, W, Cout, k, s, p = FWD[n]
    return ops.conv_desc(b if N is None else N, Cin, H, W, Cout, k, s, p)


def ref64(x, w, b, relu, slope):
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None if b is None else torch.from_numpy(b).double(),
                                   stride=1, padding=1)
    return (torch.nn.functional.leaky_relu(y, slope) if relu else y).numpy()


def inputs(name, N=None):
    n, Cin, H, W, Cout = SHAPES[name]
    return rand((n if N is None else N, Cin, H, W), 1), rand((Cout, Cin, 3, 3), 2, 0.1), rand((Cout,), 3, 0.1)


_REF = {}


def reference(name, relu, has_b, slope):
    """fp64 reference of a shape's inputs, computed once and shared (read-only) by the host and the GPU test."""
    key = (name, relu, has_b, slope)
    if key not in _REF:
        x, w, b = inputs(name)
        _REF[key] = ref64(x, w, b if has_b else None, relu, slope)
        _REF[key].setflags(write=False)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the arithmetic, emulated: numpy, fp32


def bf16(v):
    """round-to-nearest-even to bf16, as an fp32 array (finite values)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7fff))) & np.uint32(0xffff0000)).view(np.float32)


def split3(v):
    h = bf16(v)
    r = v - h
    m = bf16(r)
    r = r - m
    return {"h": h, "m": m, "l": bf16(r)}


def transform_v(x):
    """[N, C, H, W] -> V [N, tiles y, tiles x, 16, C] in fp32, rows first, conv_wino.hip's operation order."""
    N, Cc, H, W = x.shape
    ty, tx = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((N, Cc, 2 * ty + 2, 2 * tx + 2), np.float32)
    xp[:, :, 1:1 + H, 1:1 + W] = x
    d = [[xp[:, :, i:i + 2 * ty:2, j:j + 2 * tx:2] for j in range(4)] for i in range(4)]
    w_ = [[None] * 4 for _ in range(4)]
    for j in range(4):
        w_[0][j] = d[0][j] - d[2][j]; w_[1][j] = d[1][j] + d[2][j]; w_[2][j] = d[2][j] - d[1][j]; w_[3][j] = d[1][j] - d[3][j]
    v = []
    for i in range(4):
        v += [w_[i][0] - w_[i][2], w_[i][1] + w_[i][2], w_[i][2] - w_[i][1], w_[i][1] - w_[i][3]]
    return np.stack(v, -1).transpose(0, 2, 3, 4, 1).astype(np.float32)          # [N, C, ty, tx, 16] -> [N, ty, tx, 16, C]


def transform_u(w):
    """[Cout, Cin, 3, 3] -> U [16, Cin, Cout] in fp32, conv_wino.hip's wino_u."""
    g = [[w[:, :, a, b] for b in range(3)] for a in range(3)]
    half = np.float32(0.5)
    tmp = [[g[0][k] for k in range(3)], [((g[0][k] + g[1][k]) + g[2][k]) * half for k in range(3)],
           [((g[0][k] - g[1][k]) + g[2][k]) * half for k in range(3)], [g[2][k] for k in range(3)]]
    U = []
    for i in range(4):
        U += [tmp[i][0], ((tmp[i][0] + tmp[i][1]) + tmp[i][2]) * half, ((tmp[i][0] - tmp[i][1]) + tmp[i][2]) * half, tmp[i][2]]
    return np.stack(U, 0).transpose(0, 2, 1).astype(np.float32)                 # [16, Cout, Cin] -> [16, Cin, Cout]


def emulate(x, w, b=None, relu=False, slope=0.1, products=PRODUCTS):
    """The kernel's arithmetic: per position one fp32 accumulator; k-steps of 16 channels ascending; per k-step the piece products in the
    given order, each k-step's product summed over its 16 channels in fp32; A^T . A, bias, ReLU in fp32."""
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    V, U = transform_v(x), transform_u(w)
    ty, tx = V.shape[1:3]
    Vp = {k: a.reshape(N * ty * tx, 16, Cin).transpose(1, 0, 2) for k, a in split3(V).items()}        # [16, tiles, Cin]
    Up = split3(U)                                                                                    # [16, Cin, Cout]
    acc = np.zeros((16, N * ty * tx, Cout), np.float32)
    for c0 in range(0, Cin, 16):
        for pr in products:
            acc = acc + np.matmul(Vp[pr[0]][:, :, c0:c0 + 16], Up[pr[1]][:, c0:c0 + 16, :]).astype(np.float32)
    M = acc.reshape(4, 4, N, ty, tx, Cout)
    t0 = [M[0, k] + M[1, k] + M[2, k] for k in range(4)]
    t1 = [M[1, k] - M[2, k] - M[3, k] for k in range(4)]
    y = np.zeros((N, Cout, 2 * ty, 2 * tx), np.float32)
    for h, t in enumerate((t0, t1)):
        y[:, :, h::2, 0::2] = (t[0] + t[1] + t[2]).transpose(0, 3, 1, 2)
        y[:, :, h::2, 1::2] = (t[1] - t[2] - t[3]).transpose(0, 3, 1, 2)
    y = y[:, :, :H, :W]
    if b is not None:
        y = y + b.astype(np.float32)[None, :, None, None]
    if relu:
        y = np.where(y > 0, y, y * np.float32(slope))
    return np.ascontiguousarray(y, np.float32)


def exact_inputs(kind):
    N, Cin, H, W, Cout = EXACT_SHAPE
    rng = np.random.default_rng(11)
    ci, ta, tb = rng.integers(0, Cin, Cout), rng.integers(0, 3, Cout), rng.integers(0, 3, Cout)
    w = np.zeros((Cout, Cin, 3, 3), np.float32)
    if kind == "split-v":
        x = (rng.integers(-2 ** 17 + 1, 2 ** 17, (N, Cin, H, W)) * 2.0 ** -16).astype(np.float32)
        w[np.arange(Cout), ci, ta, tb] = rng.choice([1.0, -1.0, 0.5, -2.0], Cout)
    elif kind == "split-u":
        x = np.zeros((N, Cin, H, W), np.float32)
        for n in range(N):
            for y in range(n, H, 5):
                for xx in range(2 * n, W, 5):
                    x[n, (3 * y + 5 * xx + n) % Cin, y, xx] = rng.choice([1.0, -1.0, 2.0, -0.5])
        w[np.arange(Cout), ci, ta, tb] = ((2 * rng.integers(2 ** 16, 2 ** 17, Cout) + 1) * rng.choice([1.0, -1.0], Cout) * 2.0 ** -12).astype(np.float32)
    else:
        x = (1.0 + rng.integers(0, 4, (N, Cin, H, W)) / 256.0).astype(np.float32)
        w[np.arange(Cout), ci, ta, tb] = (rng.choice([1.0, -1.0], Cout) * (1.0 + rng.choice([1, 3], Cout) / 256.0)).astype(np.float32)
    return x, w


def exact_reference(kind):
    x, w = exact_inputs(kind)
    ref = ref64(x, w, None, False, 0.1)
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref) and np.abs(ref).max() > 0.5          # the reference is itself an fp32 value
    return x, w, ref32


# ---------------------------------------------------------------------------------------------------------------------------------------
# host


def test_routes_without_the_flag_are_unchanged():
    convs = [n for n in FWD if not FWD[n][1]]
    for flags in (0, F_BF16X3):
        for n in convs:
            want = FWD[n][0]
            if flags and want == DIRECT and FWD[n][7:10] == (5, 2, 2):
                want |= BIT                                   # what FN2_ROUTE_BF16X3 has always done; never a Winograd layer
            assert lib_route(fwd_desc(n), flags) == want, (n, flags)
        for (graph, name, kind, n, ci, h, w, co, k, s, p) in production_layers():
            if kind == "deconv":
                continue
            d = ops.conv_desc(n, ci, h, w, co, k, s, p)
            r = lib_route(d, flags)
            assert r & ~BIT == lib_route(d) and (not r & BIT or (flags and r == (DIRECT | BIT))), (graph, name, flags)
            assert r != SPLIT


def test_flag_changes_the_winograd_layers_the_kernel_takes_only():
    convs = [n for n in FWD if not FWD[n][1]]
    for n in convs:
        d = fwd_desc(n)
        want = SPLIT if (FWD[n][0] == WINOGRAD and supported(d)) else FWD[n][0]
        assert lib_route(d, F_WINO) == want, n
    assert lib_route(fwd_desc("wino-threshold"), F_WINO) == SPLIT == lib_route(fwd_desc("wino-fallthrough"), F_WINO)
    took, wino64 = set(), set()
    for (graph, name, kind, n, ci, h, w, co, k, s, p) in production_layers():
        if kind == "deconv":
            continue
        d = ops.conv_desc(n, ci, h, w, co, k, s, p)
        plain, flagged = lib_route(d), lib_route(d, F_WINO)
        if flagged != plain:
            assert plain == WINOGRAD and flagged == SPLIT and supported(d) and floats(d, SPLIT) > 0, (graph, name)
            took.add((graph, name))
        if plain == WINOGRAD and co % 64 == 0:
            assert (k, s, p) == (3, 1, 1) and w % 4 == 0
            wino64.add((graph, name))
    # every production Winograd layer with Cout % 64 == 0 is taken, and nothing else changes
    assert took == wino64 and {("C@8x448x320", "conv3_1"), ("C@8x448x320", "conv4_1")} <= took


def test_flag_composes_with_force_the_other_flag_and_batch_invariant_mode():
    small = ops.conv_desc(2, 24, 6, 8, 64, 3, 1, 1)          # PLANE by its size, WINOGRAD when forced
    assert lib_route(small) == PLANE == lib_route(small, F_WINO) and lib_route(small, F_FORCE) == WINOGRAD
    assert lib_route(small, F_FORCE | F_WINO) == SPLIT == lib_route(small, F_FORCE | F_WINO | F_BF16X3)
    assert lib_route(small, F_FORCE | F_BF16X3) == WINOGRAD                      # FN2_ROUTE_BF16X3 alone never touches a Winograd layer
    five = fwd_desc("direct-5x5")
    assert lib_route(five, F_WINO) == DIRECT and lib_route(five, F_WINO | F_BF16X3) == (DIRECT | BIT)
    thr = fwd_desc("wino-threshold")
    assert lib_route(thr, F_WINO | F_BF16X3) == SPLIT and lib_route(thr, F_BF16X3) == WINOGRAD
    narrow = ops.conv_desc(3, 13, 65, 76, 96, 3, 1, 1)        # a Winograd layer the split kernel does not take: Cout % 64
    assert lib_route(narrow) == WINOGRAD == lib_route(narrow, F_WINO) == lib_route(narrow, F_WINO | F_FORCE)
    was = ops.get_batch_invariant()
    ops.set_batch_invariant(True)
    try:
        for d1, d8 in ((ops.conv_desc(1, 24, 6, 8, 64, 3, 1, 1), ops.conv_desc(8, 24, 6, 8, 64, 3, 1, 1)), (fwd_desc("wino-threshold", 1), fwd_desc("wino-threshold", 8))):
            assert lib_route(d1, F_WINO) == lib_route(d8, F_WINO) == SPLIT
            assert lib_route(d1) == lib_route(d8) == WINOGRAD
    finally:
        ops.set_batch_invariant(was)
    assert ops.ROUTE_WINO_BF16X3 == F_WINO
    assert ops.conv_forward_route(thr, wino_bf16x3=True) == SPLIT and ops.conv_forward_route(thr) == WINOGRAD
    assert ops.conv_forward_route(small, True, False, True) == SPLIT and ops.conv_forward_route(thr, bf16x3=True) == WINOGRAD
    assert set(ops.CONV_FWD_ROUTES) == set(range(6))          # the arithmetic is a bit beside the route, not a sixth route


def test_operand_sizes():
    L = _lib.lib()
    for s, shape in list(SHAPES.items()) + [("exact", EXACT_SHAPE)]:
        d = desc_for(shape)
        n, Cin, H, W, Cout = shape
        assert supported(d) == 1, s
        # three bf16 planes of [Cout / 32][ceil(Cin / 16) + 1 k-steps][16 positions][64 lanes][8]
        assert floats(d, SPLIT) == (Cout // 32) * ((Cin + 15) // 16 + 1) * 12288, s
        assert floats(d, WINOGRAD) > 0 and floats(d, SPLIT) != floats(d, WINOGRAD), s
        assert floats(d, PLANE | BIT) == 0 and floats(d, DIRECT | BIT) == 0 and floats(d, BIT) == 0, s
        for r in (SPLIT, PLANE | BIT, DIRECT | BIT, BIT):
            assert L.fn2_conv_workspace_bytes(C.byref(d), r) == 0
    for Cin in range(1, 200):          # never the exact operand's length
        d = ops.conv_desc(1, Cin, 8, 8, 64, 3, 1, 1)
        assert floats(d, SPLIT) != floats(d, WINOGRAD) and floats(d, SPLIT) > 0
    refused = {"Win % 4": ops.conv_desc(2, 12, 17, 30, 64, 3, 1, 1), "pad 0": ops.conv_desc(2, 12, 17, 28, 64, 3, 1, 0),
               "Cout 96": ops.conv_desc(2, 12, 17, 28, 96, 3, 1, 1), "Cout 16": ops.conv_desc(2, 12, 17, 28, 16, 3, 1, 1),
               "stride 2": ops.conv_desc(2, 12, 17, 28, 64, 3, 2, 1), "5x5": ops.conv_desc(2, 12, 17, 28, 64, 5, 2, 2)}
    for what, d in refused.items():
        assert supported(d) == 0 and floats(d, SPLIT) == 0 and lib_route(d, F_WINO | F_FORCE) == lib_route(d, F_FORCE), what
    assert supported(ops.conv_desc(1, 1, 1, 4, 64, 3, 1, 1)) == 1 and supported(ops.conv_desc(1, 1000, 7, 4, 512, 3, 1, 1)) == 1      # any Cin, any height
    assert L.fn2_conv_wino_bf16x3_num_variants() >= 2


def test_switch():
    from flownet2_amd import functional as Fn
    others = lambda: (Fn.conv_arithmetic(), Fn.deconv_arithmetic(), Fn.conv_backward_arithmetic(), Fn.correlation_arithmetic())
    before = others()
    assert Fn.get_winograd_arithmetic() == "fp32"
    thr = fwd_desc("wino-threshold")
    try:
        Fn.set_winograd_arithmetic("bf16x3")
        assert Fn.get_winograd_arithmetic() == "bf16x3" and others() == before
        assert Fn.winograd_arithmetic() == Fn.get_winograd_arithmetic() == Fn.arithmetic("wino")          # the regular-named getter, the table's
        for s in Fn.ARITH_SWITCHES:                         # the names the table gives are the module's functions
            assert getattr(Fn, s.getter)() == Fn.arithmetic(s.key) and callable(getattr(Fn, s.setter)), s.key
        assert Fn.conv_forward_route(thr) == SPLIT and Fn.conv_forward_route(fwd_desc("direct-5x5")) == DIRECT
        for bad in ("bf16", "fp16", "", "BF16X3"):
            with pytest.raises(ValueError):
                Fn.set_winograd_arithmetic(bad)
            assert Fn.get_winograd_arithmetic() == "bf16x3"
        Fn.set_conv_arithmetic("bf16x3")
        try:
            assert Fn.conv_forward_route(thr) == SPLIT and Fn.conv_forward_route(fwd_desc("direct-5x5")) == (DIRECT | BIT)
        finally:
            Fn.set_conv_arithmetic("fp32")
    finally:
        Fn.set_winograd_arithmetic("fp32")
    assert Fn.get_winograd_arithmetic() == "fp32" and others() == before and Fn.conv_forward_route(thr) == WINOGRAD
    assert Fn.winograd_arithmetic() == Fn.get_winograd_arithmetic() == Fn.arithmetic("wino")


@pytest.mark.parametrize("name", list(SHAPES))
def test_emulation_meets_the_fp64_bound(name):
    x, w, b = inputs(name)
    for relu, has_b, slope in [(True, True, 0.1), (False, False, 0.1)]:
        ref = reference(name, relu, has_b, slope)
        got = emulate(x, w, b if has_b else None, relu, slope)
        ratio = float(np.abs(got - ref).max()) / (BOUND * scale_of(ref))
        print("emulated bf16x3 fp64 error / bound: %s relu=%d bias=%d: %.3f" % (name, relu, has_b, ratio))
        assert got.shape == ref.shape and ratio <= 1.0, (name, ratio)


def test_emulation_needs_each_of_the_six_products_and_none_of_the_dropped_three():
    moved = {p: 0.0 for p in PRODUCTS}
    for kind in KINDS:
        x, w, ref32 = exact_reference(kind)
        assert same_bits(emulate(x, w) + np.float32(0.0), ref32 + np.float32(0.0)), kind          # (+ 0.0: -0.0 == 0.0)
        Vp, Up = split3(transform_v(x)), split3(transform_u(w))
        for pr in DROPPED:          # zero piece by piece: nothing is owed to the three products the arithmetic leaves out
            v, u = Vp[pr[0]], Up[pr[1]]          # [N, ty, tx, 16, Cin], [16, Cin, Cout]
            assert not (np.abs(v).max(axis=(0, 1, 2))[:, :, None] * np.abs(u)).any(), (kind, pr)
        with_dropped = emulate(x, w, products=DROPPED + PRODUCTS)
        assert same_bits(with_dropped + np.float32(0.0), ref32 + np.float32(0.0)), kind
        for pr in PRODUCTS:
            got = emulate(x, w, products=[q for q in PRODUCTS if q != pr])
            err = float(np.abs(got.astype(np.float64) - ref32).max())
            moved[pr] = max(moved[pr], err / (BOUND * scale_of(ref32)))
            if pr in {"split-v": ("hh", "mh", "lh"), "split-u": ("hh", "hm", "hl"), "mid-mid": ("hh", "hm", "mh", "mm")}[kind]:
                assert not same_bits(got + np.float32(0.0), ref32 + np.float32(0.0)) and err > 0, (kind, pr)
    print("worst move / fp64 bound when a product is dropped: " + ", ".join("%s %.3g" % kv for kv in moved.items()))
    assert all(moved[p] > 0 for p in PRODUCTS)
    assert all(moved[p] > 1.0 for p in ("hh", "hm", "mh"))          # the large terms fail the fp64 bound too


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU


def pack_for(shape, w, route=SPLIT, N=None):
    return ops.conv_pack_weights(dev(w), desc_for(shape, N), route)


def run_for(shape, packed, x_blob, bias, relu, slope, in_c0=0, out_blob=None, out_c0=0, N=None, route=SPLIT):
    o = None if out_blob is None else dev(out_blob)
    y = ops.conv_forward(dev(x_blob), packed, None if bias is None else dev(bias), desc_for(shape, N), route, False, relu, slope, out=o, out_c0=out_c0, in_c0=in_c0)
    torch.cuda.synchronize()
    return host(y)


def pack(name, w, route=SPLIT, N=None):
    return pack_for(SHAPES[name], w, route, N)


def run(name, *a, **k):
    return run_for(SHAPES[name], *a, **k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp64_bound(name):
    """error / bound, worst of the six flag sets, split route / exact Winograd route (measured on an MI355X): small 0.033 / 0.042, wide 0.027 / 0.039, deep 0.102 / 0.132, threshold 0.026 / 0.030"""
    x, w, b = inputs(name)
    packed, packed_exact = pack(name, w), pack(name, w, WINOGRAD)
    worst = {SPLIT: 0.0, WINOGRAD: 0.0}
    for relu, has_b, slope in flag_sets("wino-threshold"):
        bb = b if has_b else None
        ref = reference(name, relu, has_b, slope)
        for route, op in ((SPLIT, packed), (WINOGRAD, packed_exact)):
            got = run(name, op, x, bb, relu, slope, route=route)
            assert got.shape == ref.shape
            ratio = float(np.abs(got - ref).max()) / (BOUND * scale_of(ref))
            worst[route] = max(worst[route], ratio)
            print("fp64 error / bound: %s %s relu=%d bias=%d slope=%g: %.3f" % (name, "bf16x3" if route == SPLIT else "exact ", relu, has_b, slope, ratio))
            assert ratio <= 1.0, (name, route, relu, has_b, slope, ratio)
    print("worst fp64 error / bound: %s bf16x3 %.3f, exact %.3f" % (name, worst[SPLIT], worst[WINOGRAD]))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_exact_values(kind):
    x, w, ref32 = exact_reference(kind)
    got = run_for(EXACT_SHAPE, pack_for(EXACT_SHAPE, w), x, None, False, 0.1)
    assert same_bits(got + np.float32(0.0), ref32 + np.float32(0.0)), (kind, float(np.abs(got - ref32).max()))      # (+ 0.0: -0.0 == 0.0)


@pytest.mark.gpu
def test_blob_forms():
    N, Cin, H, W, Cout = SHAPES["threshold"]
    x, w, b = inputs("threshold")
    packed = pack("threshold", w)
    base = run("threshold", packed, x, b, True, 0.1)
    assert np.isfinite(base).all()
    wide = np.full((N, Cin + 5, H, W), np.nan, np.float32)           # the neighbouring channels hold NaN: a ragged k-step must not meet them
    wide[:, 2:2 + Cin] = x
    for in_slice, out_slice in [(False, True), (True, False), (True, True)]:
        blob = np.full((N, Cout + 7, H, W), SENTINEL) if out_slice else None
        got = run("threshold", packed, wide if in_slice else x, b, True, 0.1, 2 if in_slice else 0, blob, 3 if out_slice else 0)
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
    for i in range(3):
        assert same_bits(run(name, pack(name, w, N=1), x[i:i + 1], b, True, 0.1, N=1), batch[i:i + 1]), i
    ran = 0
    with forced_variants("conv_wino_bf16x3") as (nv, force):
        for v in range(nv):
            force(v)
            assert same_bits(run(name, packed, x, b, True, 0.1, N=3), batch), v
            assert same_bits(run(name, packed, x[:1], b, True, 0.1, N=1), batch[:1]), v
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
    N, Cin, H, W, Cout = EXACT_SHAPE
    d = desc_for(EXACT_SHAPE)
    x = dev(rand((N, Cin + 8, H, W), 4))
    w = rand((Cout, Cin, 3, 3), 2, 0.1)
    split_op, exact_op = pack_for(EXACT_SHAPE, w), pack_for(EXACT_SHAPE, w, WINOGRAD)
    top = torch.full((N, Cout + 8, H, W), float(SENTINEL), device="cuda")
    untouched = lambda: bool((top == float(SENTINEL)).all())
    d96 = ops.conv_desc(N, Cin, H, W, 96, 3, 1, 1)           # an exact Winograd layer the split kernel does not take; the top has room for it
    assert lib_route(d96, F_FORCE) == WINOGRAD and not supported(d96)
    misaligned = split_op.new_empty(split_op.numel() + 1)[1:]
    misaligned.copy_(split_op)
    calls = {
        "Cout 96 descriptor": dict(d=d96), "PLANE | 0x100": dict(route=PLANE | BIT), "DIRECT | 0x100": dict(route=DIRECT | BIT), "0x100 alone": dict(route=BIT),
        "null bottom": dict(null=("bottom",)), "null operand": dict(null=("packed",)), "null top": dict(null=("top",)),
        "bottom slice past its blob": dict(in_ch=Cin + 1, in_c0=2), "top slice past its blob": dict(top_ch=Cout + 2, top_c0=3),
        "negative top slice": dict(top_ch=Cout + 8, top_c0=-1), "misaligned operand": dict(packed=misaligned),
    }
    for what, kw in calls.items():
        a = dict(d=d, route=SPLIT, in_ch=Cin + 8, in_c0=0, top_ch=Cout + 8, top_c0=0, null=(), packed=split_op)
        a.update(kw)
        with pytest.raises(Fn2Error):
            raw_forward(a["d"], a["route"], x, a["in_ch"], a["in_c0"], a["packed"], top, a["top_ch"], a["top_c0"], a["null"])
            pytest.fail("%s was not refused" % what)
        assert untouched(), what
    # an operand packed for the other arithmetic: ops.conv_forward's length check
    xs = x[:, :Cin].contiguous()
    for operand, route in ((exact_op, SPLIT), (split_op, WINOGRAD)):
        with pytest.raises(ValueError):
            ops.conv_forward(xs, operand, None, d, route, False, True, 0.1, out=top)
        assert untouched()
    for r in (PLANE | BIT, DIRECT | BIT, BIT):
        with pytest.raises(ValueError):
            ops.conv_pack_weights(dev(w), d, r)
    with pytest.raises(ValueError):
        ops.conv_pack_weights(dev(rand((96, Cin, 3, 3), 2)), d96, SPLIT)
    with pytest.raises(Fn2Error):
        check(_lib.lib().fn2_conv_pack_weights(C.byref(d96), SPLIT, ops._ptr(dev(w)), ops._ptr(split_op), ops._stream()))
    torch.cuda.synchronize()
    # the by-route backward functions refuse the bit on WINOGRAD: the data gradient stays exact
    L = _lib.lib()
    bw = int(L.fn2_conv_backward_data_route(C.byref(d), 0))
    assert bw != 0 and int(L.fn2_conv_backward_data_packed_weight_floats(C.byref(d), 0, bw)) > 0
    assert int(L.fn2_conv_backward_data_packed_weight_floats(C.byref(d), 0, bw | BIT)) == 0
    assert int(L.fn2_conv_backward_data_computed_channels(C.byref(d), 0, bw | BIT)) == 0
    # ... and the call none of this applies to writes exactly the layer's channels
    raw_forward(d, SPLIT, x, Cin + 8, 0, split_op, top, Cout + 8, 0)
    assert not bool((top[:, :Cout] == float(SENTINEL)).any()) and bool((top[:, Cout:] == float(SENTINEL)).all())


@pytest.mark.gpu
def test_non_finite_inputs_reach_their_own_windows_only():
    N, Cin, H, W, Cout = EXACT_SHAPE
    x, w, b = rand((N, Cin, H, W), 1), rand((Cout, Cin, 3, 3), 2, 0.1), rand((Cout,), 3, 0.1)
    assert (w != 0).all()
    packed = pack_for(EXACT_SHAPE, w)
    clean = run_for(EXACT_SHAPE, packed, x, b, True, 0.1)
    assert np.isfinite(clean).all()
    bad = x.copy()
    spots = [(0, 3, 4, 7, np.inf), (1, 10, 13, 21, np.nan)]          # an even / odd and an odd / odd pixel: a tile's edge column and its inner one
    covered = np.zeros((N, H, W), bool)
    for (n, c, yy, xx, v) in spots:
        bad[n, c, yy, xx] = v
        covered[n, max(0, yy - 1):yy + 2, max(0, xx - 1):xx + 2] = True
    assert covered.sum() == 18
    got = run_for(EXACT_SHAPE, packed, bad, b, True, 0.1)
    mask = np.broadcast_to(covered[:, None], got.shape)
    assert np.array_equal(~np.isfinite(got), mask)
    assert np.array_equal(got.view(np.uint32)[~mask], clean.view(np.uint32)[~mask])


@pytest.mark.gpu
def test_python_layer(monkeypatch):
    from flownet2_amd import functional as Fn
    monkeypatch.delenv("FN2_STRICT", raising=False)          # (what the backward of this layer hands to the library is counted, in either arithmetic)
    N, Cin, H, W, Cout = SHAPES["threshold"]
    d = desc("threshold")
    assert lib_route(d) == WINOGRAD
    w, b = dev(rand((Cout, Cin, 3, 3), 2, 0.1)), dev(rand((Cout,), 3, 0.1))
    wide = dev(rand((N, Cin + 5, H, W), 9))
    x = wide[:, 2:2 + Cin]
    assert not x.is_contiguous()
    want = ops.conv_forward(x.contiguous(), ops.conv_pack_weights(w, d, SPLIT), b, d, SPLIT, False, True, 0.1)
    exact = ops.conv_forward(x.contiguous(), ops.conv_pack_weights(w, d, WINOGRAD), b, d, WINOGRAD, False, True, 0.1)
    assert not torch.equal(want, exact)
    g = dev(rand((N, Cout, H, W), 13))
    lin = {r: ops.conv_forward(x.contiguous(), ops.conv_pack_weights(w, d, r), b, d, r, False, False, 0.1) for r in (SPLIT, WINOGRAD)}

    def grads():
        # without the fused ReLU: the gradients are then functions of g, x and w alone, not of the sign of a forward value that the two
        # arithmetics may round to different sides of zero
        xg, wg, bg = x.detach().clone().requires_grad_(True), torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
        y = Fn.conv_mfma_relu(xg, wg, bg, 1, 1, 0.1, False)
        assert y.requires_grad and y.grad_fn is not None
        (y * g).sum().backward()
        return y.detach(), xg.grad.clone(), wg.grad.clone(), bg.grad.clone()

    assert Fn.get_winograd_arithmetic() == "fp32"
    before = Fn.LIBRARY_FALLBACKS[0]
    y_off, gx_off, gw_off, gb_off = grads()
    assert torch.equal(y_off, lin[WINOGRAD])
    bwd_fallbacks = Fn.LIBRARY_FALLBACKS[0] - before
    before = Fn.LIBRARY_FALLBACKS[0]
    Fn.set_winograd_arithmetic("bf16x3")
    try:
        assert Fn.conv_forward_route(d) == SPLIT and Fn.conv_route_name(x.shape, w, 1, 1) == "wino+bf16x3"
        assert Fn.conv_route_name((N, Cin, H, W), dev(rand((96, Cin, 3, 3), 2)), 1, 1) == "wino"
        assert torch.equal(Fn.conv_mfma_relu(x, w, b, 1, 1, 0.1, True), want)
        blob = torch.full((N, Cout + 7, H, W), float(SENTINEL), device="cuda")
        Fn.conv_mfma_relu(x, w, b, 1, 1, 0.1, True, out=blob, out_c0=3)
        assert torch.equal(blob[:, 3:3 + Cout], want) and bool((blob[:, :3] == float(SENTINEL)).all()) and bool((blob[:, 3 + Cout:] == float(SENTINEL)).all())
        assert Fn.LIBRARY_FALLBACKS[0] == before             # the forward never falls back
        y_on, gx_on, gw_on, gb_on = grads()
        assert torch.equal(y_on, lin[SPLIT]) and not torch.equal(y_on, y_off) and Fn.LIBRARY_FALLBACKS[0] == before + bwd_fallbacks
        # every backward route stays exact fp32: the same bits with the switch on and off
        assert torch.equal(gx_on, gx_off) and torch.equal(gw_on, gw_off) and torch.equal(gb_on, gb_off)
    finally:
        Fn.set_winograd_arithmetic("fp32")
    assert Fn.get_winograd_arithmetic() == "fp32" and Fn.conv_forward_route(d) == WINOGRAD
    assert torch.equal(Fn.conv_mfma_relu(x, w, b, 1, 1, 0.1, True), exact)
    keys = [key for key in Fn._PACKED_T if key[0] == id(w) and key[1][0] == "fwd"]
    assert sorted(key[1][1] for key in keys) == [WINOGRAD, SPLIT]
    assert Fn.LIBRARY_FALLBACKS[0] == before + bwd_fallbacks


@pytest.mark.gpu
def test_flownetc_end_to_end(monkeypatch):
    """Measured on an MI355X at 1 x 128 x 128: 3.201e-07 px between the two exact runs, 3.959e-07 px split against exact (3 layer calls)"""
    from flownet2_amd import functional as Fn
    B, H, W = 1, 128, 128          # the smallest size at which every layer has an own kernel (tests/test_deconv_bf16x3.py)
    calls = []
    fwd = ops.conv_forward

    def recorded(x, packed, bias, desc, route, transposed=False, *a, **k):
        if not transposed:
            calls.append((int(route), desc.Cin, desc.Cout))
        return fwd(x, packed, bias, desc, route, transposed, *a, **k)

    monkeypatch.setattr(ops, "conv_forward", recorded)
    P = {k: v.cuda() for k, v in nets.init_params("C", 0).items()}
    rng = np.random.default_rng(5)
    i0 = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)).cuda()
    i1 = torch.roll(i0, (2, -3), (2, 3)).contiguous()
    assert Fn.get_winograd_arithmetic() == "fp32"
    epd = lambda a, b: float(((a - b) ** 2).sum(1).sqrt().mean())
    with torch.no_grad():
        plain = nets.deploy_forward("C", P, i0, i1, Fn)
        Fn.set_route_force(True)
        try:
            del calls[:]
            forced = nets.deploy_forward("C", P, i0, i1, Fn)
            assert calls and not any(r & BIT for r, _, _ in calls)
            del calls[:]
            Fn.set_winograd_arithmetic("bf16x3")
            try:
                split = nets.deploy_forward("C", P, i0, i1, Fn)
                took = [c for c in calls if c[0] & BIT]
                again = nets.deploy_forward("C", P, i0, i1, Fn)
            finally:
                Fn.set_winograd_arithmetic("fp32")
        finally:
            Fn.set_route_force(False)
    assert took and all(r == SPLIT for r, _, _ in took)
    assert {(473, 256), (512, 512)} <= {(ci, co) for _, ci, co in took}          # the conv3_1 / conv4_1 classes
    assert torch.equal(split, again)
    yard, diff = epd(plain, forced), epd(split, forced)
    print("mean end-point difference: two exact fp32 summation orders (route force off / on) %.3e px; bf16x3 vs exact, force on: %.3e px (%d layer calls in split arithmetic)"
          % (yard, diff, len(took)))
    assert np.isfinite(diff) and yard > 0 and diff <= 3 * yard, (diff, yard)
