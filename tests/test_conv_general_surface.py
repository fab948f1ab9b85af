"""The Python surface of the general-geometry convolution over its three C ABIs (fn2_conv_desc, 14 ints, 19 ints): what a caller of
flownet2_amd.ops / flownet2_amd.functional sees, whichever way the wrappers are written.

CPU tier: the signatures of the public names; the ints conv_geometry and conv_volume build; supported / sizes / out_shape of one square
layer stated three ways; the invalid descriptors refused three ways.  GPU tier: on one tiny layer per family (1 x 2 x 4 x 5 -> 3, 2x2 taps;
the volume family with a depth of 2 and 2x2x2 taps) every wrong call of pack_weights, forward, backward_data and backward_weights is refused
in Python with the text written here in full -- nothing is launched --, a doubly wrong call reports the check that comes first, and one
forward per family writes its channel slice of a wider blob and nothing else."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_general_cases as sq
from flownet2_amd import Fn2Error, ops
from flownet2_amd import functional as Fn

SENTINEL = -7.25
TOL_DIRECT = 4e-6               # the forward bound of tests/test_conv_general.py: 4e-6 x scale

# ------------------------------------------------------------------------------------------------------------------------------ CPU tier
_DESC_TAIL = {
    "supported": "(%s, transposed=False) -> 'bool'",
    "sizes": "(%s, transposed=False)",
    "out_shape": "(%s, transposed=False)",
    "pack_weights": "(weight, %s, transposed=False, backward=False)",
    "forward": "(x, packed, bias, %s, transposed=False, relu=False, negative_slope=0.0, out=None, out_c0=0, in_c0=0)",
    "backward_data": "(top_diff, packed, %s, transposed=False, top_c0=0, out=None, out_c0=0)",
    "backward_weights": "(bottom, top_diff, %s, transposed=False, weight_diff=None, bias_diff=None, bias=True, accumulate=False, "
                        "bottom_c0=0, top_c0=0)",
}
OPS_SIGNATURES = dict(
    [("conv_%s_%s" % (fam, fn), sig % arg) for fam, arg in (("general", "desc"), ("geometry", "geom"), ("volume", "geom"))
     for fn, sig in _DESC_TAIL.items()],
    conv_geometry="(N, Cin, Hin, Win, Cout, kernel, stride=1, pad=0, dilation=1, group=1)",
    conv_volume="(N, Cin, size, Cout, kernel, stride=1, pad=0, dilation=1, group=1)",
    set_conv_general_groups="(groups: 'int' = 0)", _pair="(v, what)", _per_axis="(v, axes, what)")
FN_SIGNATURES = dict(
    lib_conv2d="(x, w, b, stride, pad, dilation=1, groups=1)", lib_conv_transpose2d="(x, w, b, stride, pad, dilation=1, groups=1)",
    lib_conv3d="(x, w, b, stride, pad, dilation=1, groups=1)", lib_conv_transpose3d="(x, w, b, stride, pad, dilation=1, groups=1)",
    set_general_convolution="(name: 'str' = 'library')", general_convolution="() -> 'str'", add_general_convolution_flag="(ap)",
    apply_general_convolution_flag="(args)")


def test_the_public_names_keep_their_signatures():
    assert len(OPS_SIGNATURES) == 26
    for module, table in ((ops, OPS_SIGNATURES), (Fn, FN_SIGNATURES)):
        for name, sig in table.items():
            f = getattr(module, name)
            assert str(inspect.signature(f)) == sig and f.__name__ == name, name
    assert all(getattr(ops, name).__doc__ for name in OPS_SIGNATURES)
    assert isinstance(Fn.LIBRARY_FALLBACKS, list) and len(Fn.LIBRARY_FALLBACKS) == 1 and Fn.general_convolution() in ("library", "own")


def test_the_ints_of_conv_geometry_and_conv_volume():
    # rectangular, grouped, values given as one-element lists
    assert list(ops.conv_geometry(2, 3, 8, 9, 6, (3, 5), (1, 2), (0, 1), (2, 1), 1)) == [2, 3, 8, 9, 6, 3, 5, 1, 2, 0, 1, 2, 1, 1]
    assert list(ops.conv_geometry(1, 4, 6, 6, 8, 3, 2, 1, 1, 2)) == [1, 4, 6, 6, 8, 3, 3, 2, 2, 1, 1, 1, 1, 2]
    assert list(ops.conv_geometry(1, 4, 6, 6, 8, [3], [2], [1], group=4)) == [1, 4, 6, 6, 8, 3, 3, 2, 2, 1, 1, 1, 1, 4]
    # one axis, two axes (rectangular and grouped), three axes, none
    assert list(ops.conv_volume(2, 3, (7,), 5, 3, 2, 1, 1, 1)) == [2, 3, 1, 1, 7, 5, 1, 1, 3, 1, 1, 2, 0, 0, 1, 1, 1, 1, 1]
    assert list(ops.conv_volume(1, 4, (6, 7), 8, (3, 2), (1, 2), (0, 1), 1, 2)) == [1, 4, 1, 6, 7, 8, 1, 3, 2, 1, 1, 2, 0, 0, 1, 1, 1, 1, 2]
    assert list(ops.conv_volume(1, 2, (2, 4, 5), 3, 2)) == [1, 2, 2, 4, 5, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    assert list(ops.conv_volume(1, 2, (2, 4, 5), 3, [2], dilation=(1, 2, 3))) == [1, 2, 2, 4, 5, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0, 1, 2, 3, 1]
    assert list(ops.conv_volume(4, 2, (), 3, 1)) == [4, 2, 1, 1, 1, 3, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    assert ops._pair(3, "kernel") == (3, 3) and ops._pair([4], "kernel") == (4, 4) and ops._pair((1, 2), "kernel") == (1, 2)
    assert ops._per_axis(3, 2, "kernel") == (3, 3) and ops._per_axis([4], 3, "kernel") == (4, 4, 4) and ops._per_axis(5, 0, "kernel") == ()
    for call, text in ((lambda: ops._pair((1, 2, 3), "stride"), "stride: one value or a pair, not (1, 2, 3)"),
                       (lambda: ops.conv_geometry(1, 2, 4, 5, 3, 2, pad=[0, 1, 2]), "pad: one value or a pair, not [0, 1, 2]"),
                       (lambda: ops._per_axis((1, 2), 3, "pad"), "pad: one value or one per spatial axis (3), not (1, 2)"),
                       (lambda: ops.conv_volume(1, 2, (4, 5), 3, (2, 2, 2)), "kernel: one value or one per spatial axis (2), not (2, 2, 2)"),
                       (lambda: ops.conv_volume(1, 2, (2, 2, 4, 5), 3, 2),
                        "conv_volume: 4 spatial axes asked for; convolution over 0 to 3 spatial axes is supported")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


def three_ways(row):
    """(transposed, [(prefix, geometry)]) of a square row of conv_general_cases: descriptor, 14 ints, 19 ints with a trivial depth."""
    tr, N, Cin, H, W, Cout, k, s, p = row
    return tr, [("conv_general", ops.conv_desc(N, Cin, H, W, Cout, k, s, p)), ("conv_geometry", ops.conv_geometry(N, Cin, H, W, Cout, k, s, p)),
                ("conv_volume", ops.conv_volume(N, Cin, (1, H, W), Cout, (1, k, k), (1, s, s), (0, p, p)))]


SHARED = [(False,) + sq.CONV[1], (False,) + sq.CONV[3], (False,) + sq.CONV[5], (True,) + sq.DECONV[0], (True,) + sq.DECONV[3]]


@pytest.mark.parametrize("row", SHARED, ids=sq.row_id)
def test_the_three_abis_agree_on_a_square_layer(row):
    tr, ways = three_ways(row)
    assert [getattr(ops, p + "_supported")(g, tr) for p, g in ways] == [True, True, True]
    sizes = [getattr(ops, p + "_sizes")(g, tr) for p, g in ways]
    assert sizes[0] == sizes[1] == sizes[2] and len(sizes[0]) == 4 and sizes[0][0] > 0 and sizes[0][2] == 0
    shapes = [getattr(ops, p + "_out_shape")(g, tr) for p, g in ways]
    assert shapes[0] == shapes[1] == sq.out_hw(row) and shapes[2] == (1,) + sq.out_hw(row)
    assert all(type(v) is int for s in shapes for v in s)


@pytest.mark.parametrize("row", sq.INVALID, ids=sq.row_id)
def test_an_invalid_layer_is_refused_three_ways(row):
    tr, ways = three_ways(row)
    assert [getattr(ops, p + "_supported")(g, tr) for p, g in ways] == [False, False, False]
    for p, g in ways:
        with pytest.raises(Fn2Error, match="fn2_%s_sizes" % p):
            getattr(ops, p + "_sizes")(g, tr)
    # the descriptor's out shape is Python arithmetic on the descriptor (no refusal); the other two ask the library
    if row[7] > 0:
        assert ops.conv_general_out_shape(ways[0][1], tr) == sq.out_hw(row)
    for p, g in ways[1:]:
        with pytest.raises(Fn2Error, match="fn2_%s_out_shape" % p):
            getattr(ops, p + "_out_shape")(g, tr)


# ------------------------------------------------------------------------------------------------------------------------------ GPU tier
class Family:
    """The tiny layer of one family: N = 1, Cin = 2, 4 x 5 (the volume family: 2 x 4 x 5), Cout = 3, kernel 2, stride 1, pad 0."""

    def __init__(self, name):
        self.name, self.prefix, self.volume = name, "conv_" + name, name == "volume"
        self.g = {"general": lambda: ops.conv_desc(1, 2, 4, 5, 3, 2, 1, 0), "geometry": lambda: ops.conv_geometry(1, 2, 4, 5, 3, 2),
                  "volume": lambda: ops.conv_volume(1, 2, (2, 4, 5), 3, 2)}[name]()
        self.nd = 5 if self.volume else 4
        self.size, self.out, self.taps = ((2, 4, 5), (1, 3, 4), (2, 2, 2)) if self.volume else ((4, 5), (3, 4), (2, 2))
        self.bottom, self.top, self.wshape = (1, 2) + self.size, (1, 3) + self.out, (3, 2) + self.taps

    def fn(self, what):
        return getattr(ops, "%s_%s" % (self.prefix, what))

    def layer(self, channels, size):
        """The layer's extent as the family's blob check prints it."""
        dims = [1, channels] + list(size)
        return str(dims) if self.volume else "[" + ",".join(str(v) for v in dims) + "]"

    def holds(self, what, name, shape, channels, size, c0):
        return "%s_%s: %s blob %s does not hold the layer's %s at channel %d" % (self.prefix, what, name, tuple(shape), self.layer(channels, size), c0)

    def axes(self, name, shape, nd=None):
        return "%s: expected %d axes (NCHW), got shape %s" % (name, self.nd if nd is None else nd, tuple(shape))


FAMILIES = ["general", "geometry", "volume"]
CPU_TENSOR = "%s: expected a CUDA (HIP) tensor; flownet2_amd has no CPU path"


def zeros(*shape):
    return torch.zeros(shape, device="cuda")


def grow(shape, axis=-1):
    s = list(shape)
    s[axis] += 1
    return tuple(s)


def refused(call, text, error=ValueError):
    with pytest.raises(error) as e:
        call()
    assert str(e.value) == text


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_pack_weights_refusals(name):
    f = Family(name)
    pack, g = f.fn("pack_weights"), f.g
    wrong = grow(f.wshape, 0)
    refused(lambda: pack(zeros(*wrong), g), "%s_pack_weights: weight of shape %s is not this layer's" % (f.prefix, wrong))
    refused(lambda: pack(zeros(*f.wshape), g, True), "%s_pack_weights: weight of shape %s is not this layer's" % (f.prefix, f.wshape))
    refused(lambda: pack(zeros(*f.wshape[1:]), g), f.axes("weight", f.wshape[1:]))
    refused(lambda: pack(torch.zeros(f.wshape), g), CPU_TENSOR % "weight")
    refused(lambda: pack(zeros(*f.wshape).double(), g), "weight: expected float32 (Dtype=float), got torch.float64")
    # doubly wrong: a CPU tensor of the wrong axis count; the wrong axis count and so the wrong shape
    refused(lambda: pack(torch.zeros(wrong[1:]), g), CPU_TENSOR % "weight")
    refused(lambda: pack(zeros(*wrong, 1), g), f.axes("weight", wrong + (1,)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_pack_weights_of_a_layer_the_kernels_refuse(name):
    """An empty output (7x7 taps on 4 x 4, pad 1): a right-shaped weight reaches the library's refusal in all three families; with a
    wrong-shaped one the descriptor family reports the shape (it checks it before it asks for the sizes), the other two the layer."""
    g = {"general": lambda: ops.conv_desc(1, 3, 4, 4, 8, 7, 1, 1), "geometry": lambda: ops.conv_geometry(1, 3, 4, 4, 8, 7, 1, 1),
         "volume": lambda: ops.conv_volume(1, 3, (1, 4, 4), 8, (1, 7, 7), 1, (0, 1, 1))}[name]()
    pack, wshape = getattr(ops, "conv_%s_pack_weights" % name), (8, 3, 1, 7, 7) if name == "volume" else (8, 3, 7, 7)
    with pytest.raises(Fn2Error, match="fn2_conv_%s_sizes" % name):
        pack(zeros(*wshape), g)
    if name == "general":
        refused(lambda: pack(zeros(*grow(wshape)), g), "conv_general_pack_weights: weight of shape (8, 3, 7, 8) is not this layer's")
    else:
        with pytest.raises(Fn2Error, match="fn2_conv_%s_sizes" % name):
            pack(zeros(*grow(wshape)), g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_forward_refusals(name):
    f = Family(name)
    fwd, g = f.fn("forward"), f.g
    n = f.fn("sizes")(g)[0]
    x, pw, b = zeros(*f.bottom), zeros(n), zeros(3)
    operand = "%s_forward: the operand has %d floats, not what the forward reads for this layer"
    # a bottom of the wrong extent (spatial, batch), a top of the wrong extent
    for shape in (grow(f.bottom), grow(f.bottom, 0), grow(f.bottom, 2)):
        refused(lambda: fwd(zeros(*shape), pw, b, g), f.holds("forward", "bottom", shape, 2, f.size, 0))
    wide = (1, 5) + f.out
    refused(lambda: fwd(x, pw, b, g, out=zeros(*grow(wide))), f.holds("forward", "top", grow(wide), 3, f.out, 0))
    # a slice that runs past its blob, or starts before it
    refused(lambda: fwd(x, pw, b, g, in_c0=1), f.holds("forward", "bottom", f.bottom, 2, f.size, 1))
    refused(lambda: fwd(zeros(*grow(f.bottom, 1)), pw, b, g, in_c0=2), f.holds("forward", "bottom", grow(f.bottom, 1), 2, f.size, 2))
    refused(lambda: fwd(x, pw, b, g, in_c0=-1), f.holds("forward", "bottom", f.bottom, 2, f.size, -1))
    refused(lambda: fwd(x, pw, b, g, out=zeros(*wide), out_c0=3), f.holds("forward", "top", wide, 3, f.out, 3))
    # a transposed layer of the same geometry has another top
    t_out = tuple(s + 1 for s in f.size)
    refused(lambda: fwd(x, pw, b, g, True, out=zeros(*f.top)), f.holds("forward", "top", f.top, 3, t_out, 0))
    # an operand of the wrong float count
    for k in (n + 1, n - 1, 0):
        refused(lambda: fwd(x, zeros(k), b, g), operand % (f.prefix, k))
    # the wrong axis count
    refused(lambda: fwd(x[0], pw, b, g), f.axes("bottom[0]", f.bottom[1:]))
    refused(lambda: fwd(x, pw, b, g, out=zeros(*f.top)[0]), f.axes("top[0]", f.top[1:]))
    refused(lambda: fwd(x, pw, zeros(3, 1), g), f.axes("bias", (3, 1), 1))
    other = zeros(1, 2, 1, 4, 5) if not f.volume else zeros(1, 2, 8, 5)
    refused(lambda: fwd(other, pw, b, g), f.axes("bottom[0]", other.shape))
    # CPU tensors, another dtype
    refused(lambda: fwd(x.cpu(), pw, b, g), CPU_TENSOR % "bottom[0]")
    refused(lambda: fwd(x, pw.cpu(), b, g), CPU_TENSOR % "packed weight")
    refused(lambda: fwd(x, pw, b.cpu(), g), CPU_TENSOR % "bias")
    refused(lambda: fwd(x, pw, b, g, out=torch.zeros(f.top)), CPU_TENSOR % "top[0]")
    refused(lambda: fwd(x.double(), pw, b, g), "bottom[0]: expected float32 (Dtype=float), got torch.float64")
    # doubly wrong: the order is bottom, top, the blobs' extents, bias, operand
    refused(lambda: fwd(x[0], zeros(n + 1), b, g), f.axes("bottom[0]", f.bottom[1:]))
    refused(lambda: fwd(x[0], pw, b, g, out=torch.zeros(f.top)), f.axes("bottom[0]", f.bottom[1:]))
    refused(lambda: fwd(zeros(*grow(f.bottom)), zeros(n + 1), b.cpu(), g), f.holds("forward", "bottom", grow(f.bottom), 2, f.size, 0))
    refused(lambda: fwd(zeros(*grow(f.bottom)), pw, b, g, out=zeros(*grow(wide))), f.holds("forward", "bottom", grow(f.bottom), 2, f.size, 0))
    refused(lambda: fwd(x, zeros(n + 1), b.cpu(), g), CPU_TENSOR % "bias")
    refused(lambda: fwd(x, zeros(n + 1).cpu(), b, g), CPU_TENSOR % "packed weight")


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_backward_data_refusals(name):
    f = Family(name)
    bwd, g = f.fn("backward_data"), f.g
    n = f.fn("sizes")(g)[1]
    d, pw = zeros(*f.top), zeros(n)
    operand = "%s_backward_data: the operand has %d floats, not what the data gradient reads for this layer"
    for shape in (grow(f.top), grow(f.top, 0)):
        refused(lambda: bwd(zeros(*shape), pw, g), f.holds("backward_data", "top", shape, 3, f.out, 0))
    wide = (1, 4) + f.size
    refused(lambda: bwd(d, pw, g, out=zeros(*grow(wide))), f.holds("backward_data", "bottom", grow(wide), 2, f.size, 0))
    refused(lambda: bwd(d, pw, g, top_c0=1), f.holds("backward_data", "top", f.top, 3, f.out, 1))
    refused(lambda: bwd(d, pw, g, top_c0=-1), f.holds("backward_data", "top", f.top, 3, f.out, -1))
    refused(lambda: bwd(d, pw, g, out=zeros(*wide), out_c0=3), f.holds("backward_data", "bottom", wide, 2, f.size, 3))
    for k in (n + 1, 0):
        refused(lambda: bwd(d, zeros(k), g), operand % (f.prefix, k))
    refused(lambda: bwd(d[0], pw, g), f.axes("top_diff", f.top[1:]))
    refused(lambda: bwd(d, pw, g, out=zeros(*f.bottom)[0]), f.axes("bottom diff", f.bottom[1:]))
    refused(lambda: bwd(d.cpu(), pw, g), CPU_TENSOR % "top_diff")
    refused(lambda: bwd(d, pw.cpu(), g), CPU_TENSOR % "packed weight")
    refused(lambda: bwd(d, pw, g, out=torch.zeros(f.bottom)), CPU_TENSOR % "bottom diff")
    # doubly wrong: the order is top_diff, bottom diff, the blobs' extents (bottom first), operand
    refused(lambda: bwd(d[0], zeros(n + 1), g), f.axes("top_diff", f.top[1:]))
    refused(lambda: bwd(zeros(*grow(f.top)), zeros(n + 1), g), f.holds("backward_data", "top", grow(f.top), 3, f.out, 0))
    refused(lambda: bwd(zeros(*grow(f.top)), pw, g, out=zeros(*grow(wide))), f.holds("backward_data", "bottom", grow(wide), 2, f.size, 0))
    refused(lambda: bwd(d, zeros(n + 1), g, out=zeros(*f.bottom)[0]), f.axes("bottom diff", f.bottom[1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_backward_weights_refusals(name):
    f = Family(name)
    bww, g = f.fn("backward_weights"), f.g
    x, d, dw, db = zeros(*f.bottom), zeros(*f.top), zeros(*f.wshape), zeros(3)
    what = f.prefix + "_backward_weights: "
    refused(lambda: bww(zeros(*grow(f.bottom)), d, g), f.holds("backward_weights", "bottom", grow(f.bottom), 2, f.size, 0))
    refused(lambda: bww(x, zeros(*grow(f.top)), g), f.holds("backward_weights", "top", grow(f.top), 3, f.out, 0))
    refused(lambda: bww(x, d, g, bottom_c0=1), f.holds("backward_weights", "bottom", f.bottom, 2, f.size, 1))
    refused(lambda: bww(x, d, g, top_c0=1), f.holds("backward_weights", "top", f.top, 3, f.out, 1))
    # accumulate without the diffs to add into
    refused(lambda: bww(x, d, g, accumulate=True), what + "accumulate needs the diffs to add into")
    refused(lambda: bww(x, d, g, weight_diff=dw, accumulate=True), what + "accumulate needs the diffs to add into")
    refused(lambda: bww(x, d, g, bias_diff=db, accumulate=True), what + "accumulate needs the diffs to add into")
    refused(lambda: bww(x, d, g, bias=False, accumulate=True), what + "accumulate needs the diffs to add into")
    # wrong-shaped diffs
    refused(lambda: bww(x, d, g, weight_diff=zeros(*grow(f.wshape))), what + "weight diff has the wrong shape")
    d_t = zeros(1, 3, *(s + 1 for s in f.size))                                                          # transposed: [Cin, Cout, ...]
    refused(lambda: bww(x, d_t, g, True, weight_diff=dw), what + "weight diff has the wrong shape")
    refused(lambda: bww(x, d, g, weight_diff=zeros(*grow(f.wshape))[..., :2]), what + "weight diff has the wrong shape")      # not contiguous
    refused(lambda: bww(x, d, g, weight_diff=dw, bias_diff=zeros(4)), what + "bias diff has the wrong shape")
    refused(lambda: bww(x, d, g, bias_diff=zeros(6)[::2]), what + "bias diff has the wrong shape")
    # the wrong axis count
    refused(lambda: bww(x[0], d, g), f.axes("bottom", f.bottom[1:]))
    refused(lambda: bww(x, d[0], g), f.axes("top_diff", f.top[1:]))
    refused(lambda: bww(x, d, g, weight_diff=dw[0]), f.axes("weight diff", f.wshape[1:]))
    refused(lambda: bww(x, d, g, bias_diff=zeros(3, 1)), f.axes("bias diff", (3, 1), 1))
    # CPU tensors
    refused(lambda: bww(x.cpu(), d, g), CPU_TENSOR % "bottom")
    refused(lambda: bww(x, d.cpu(), g), CPU_TENSOR % "top_diff")
    refused(lambda: bww(x, d, g, weight_diff=dw.cpu()), CPU_TENSOR % "weight diff")
    refused(lambda: bww(x, d, g, bias_diff=db.cpu()), CPU_TENSOR % "bias diff")
    # doubly wrong: the order is bottom, top_diff, the blobs' extents, weight diff, bias diff
    refused(lambda: bww(x[0], d, g, weight_diff=zeros(*grow(f.wshape))), f.axes("bottom", f.bottom[1:]))
    refused(lambda: bww(x[0], d.cpu(), g), f.axes("bottom", f.bottom[1:]))
    refused(lambda: bww(zeros(*grow(f.bottom)), d, g, accumulate=True), f.holds("backward_weights", "bottom", grow(f.bottom), 2, f.size, 0))
    refused(lambda: bww(x, d, g, weight_diff=zeros(*grow(f.wshape)), bias_diff=zeros(4)), what + "weight diff has the wrong shape")
    refused(lambda: bww(x, d, g, weight_diff=dw[0], bias_diff=zeros(4)), f.axes("weight diff", f.wshape[1:]))
    refused(lambda: bww(x, d, g, bias_diff=zeros(4), accumulate=True), what + "accumulate needs the diffs to add into")
    # a bias diff that is not wanted is not looked at
    assert bww(x, d, g, weight_diff=dw, bias_diff=zeros(4), bias=False)[1] is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_forward_into_a_channel_slice_writes_only_its_slice(name):
    f = Family(name)
    g = f.g
    x, w, b = (torch.from_numpy(sq.rand(s, seed, scale)).cuda() for s, seed, scale in ((f.bottom, 1, 1.0), (f.wshape, 2, 0.1), ((3,), 3, 1.0)))
    packed = f.fn("pack_weights")(w, g)
    assert packed.numel() == f.fn("sizes")(g)[0]
    alone = f.fn("forward")(x, packed, b, g)
    assert tuple(alone.shape) == f.top
    ref = (F.conv3d if f.volume else F.conv2d)(x.double().cpu(), w.double().cpu(), b.double().cpu()).numpy()
    err = float(np.abs(alone.cpu().numpy() - ref).max())
    print("%s forward: error %.3g, bound %.3g" % (f.prefix, err, TOL_DIRECT * sq.scale_of(ref)))
    assert err <= TOL_DIRECT * sq.scale_of(ref)
    blob = torch.full((1, 5) + f.out, SENTINEL, device="cuda")
    assert f.fn("forward")(x, packed, b, g, out=blob, out_c0=1) is blob
    got = blob.cpu()
    assert torch.equal(got[:, 1:4], alone.cpu())
    assert bool((got[:, 0] == SENTINEL).all()) and bool((got[:, 4] == SENTINEL).all())
    # and reads only its slice of a wider bottom
    wide = torch.full((1, 4) + f.size, float("nan"), device="cuda")
    wide[:, 1:3] = x
    assert torch.equal(f.fn("forward")(wide, packed, b, g, in_c0=1).cpu(), alone.cpu())
