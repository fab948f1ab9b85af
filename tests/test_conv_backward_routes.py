"""Backward by descriptor (csrc/conv_route.cpp): the layer between the autograd mirror / the Caffe adapter's Backward_gpu and the kernels.

Every data-gradient route (WINOGRAD, TCONV, DECONV_PLANE, PLANE, DIRECT; the Deconvolution forms of PLANE and DIRECT) is pinned on its own:
the operand fn2_conv_backward_data_pack_weights builds equals, bit for bit, the oracle's packing of a dense operand built here in numpy from
the weight blob (rotation, channel swap, Cp padding); the result equals, bit for bit, the oracle twin of the kernel the route launches on that
operand, and matches fp64 (torch's convolution_backward); the three output forms (room for the Cp computed channels, the workspace + 2-D copy
into a channel slice of a sentinel-filled blob, a channel slice of top_diff) give the same bits.  Then the masked epilogue (ReLUBackward of
the layer in front folded into the TCONV route), the weight gradients (a / b swap of a Deconvolution, channel slices, accumulate; the stem's
fused weight + bias gradient), the autograd mirror (functional.conv_mfma_relu / deconv_relu with Concat-like blobs and the data-gradient
pack cache across a fused optimizer step), and on the host: the case lists cover every route, every layer of the FlowNetC training
graph at 448x320 batch 8 has an own backward, and so has every layer of the FlowNetS / FlowNet-SD / fusion training graphs but the ones
tests/test_train_parity_family.py allow-lists."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from flownet2_amd import Fn2Error, _lib, nets, ops
from flownet2_amd._lib import check

NONE, WINOGRAD, TCONV, PLANE, DIRECT, DECONV_PLANE = 0, 1, 2, 3, 4, 5        # FN2_BWD_ROUTE_*
SENTINEL = np.float32(-7.25)

# name: (route, transposed, N, Cin, H, W, Cout, kernel, stride, pad) -- the layer's bottom [N, Cin, H, W]; a Deconvolution is {4, 2, 1}
DGRAD = {
    "wino-padded": (WINOGRAD, False, 2, 40, 9, 12, 33, 3, 1, 1),          # Cp 48, ragged reduction quads (33)
    "wino-odd-batch": (WINOGRAD, False, 3, 64, 6, 20, 48, 3, 1, 1),
    "tconv-5x5": (TCONV, False, 2, 64, 16, 24, 96, 5, 2, 2),              # conv2 / conv3 class
    "tconv-5x5-c128": (TCONV, False, 2, 64, 16, 24, 128, 5, 2, 2),        # (the same with a forward kernel: the 96-output one has none)
    "tconv-3x3-odd": (TCONV, False, 2, 128, 17, 32, 64, 3, 2, 1),         # odd bottom height
    "tconv-3x3-9x7": (TCONV, False, 1, 64, 9, 7, 8, 3, 2, 1),             # odd bottom width: the mask read and the store take their scalar tails
    "deconv-plane-10x14": (DECONV_PLANE, False, 2, 64, 10, 14, 128, 3, 2, 1),   # conv5 / conv6 class: top 5x7
    "deconv-plane-6x10": (DECONV_PLANE, False, 2, 64, 6, 10, 128, 3, 2, 1),
    "plane-5x7": (PLANE, False, 2, 40, 5, 7, 64, 3, 1, 1),                # Cp 64
    "plane-3x5": (PLANE, False, 2, 40, 3, 5, 64, 3, 1, 1),
    "plane-deconv": (PLANE, True, 2, 70, 5, 7, 64, 4, 2, 1),              # deconv5 class, Cp 128
    "direct-1x1": (DIRECT, False, 2, 37, 6, 10, 256, 1, 1, 0),            # conv_redir's transpose, Cp 64
    "direct-deconv": (DIRECT, True, 2, 70, 6, 8, 36, 4, 2, 1),            # Cout % 4 == 0, not % 8
}

# fp64 bound of each kernel's own forward test (test_conv_wino / test_conv_mfma / test_conv_plane / test_tconv)
TOL = {WINOGRAD: 6e-6, DIRECT: 4e-6, PLANE: 4e-6, DECONV_PLANE: 4e-6, TCONV: 1e-5}


def rand(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def scale_of(ref):
    return max(1.0, float(np.abs(ref).max()))


def geom(name):
    route, tr, N, Cin, H, W, Cout, k, s, p = DGRAD[name]
    Ht, Wt = (2 * H, 2 * W) if tr else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    return route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt


def desc_of(name):
    _, tr, N, Cin, H, W, Cout, k, s, p = DGRAD[name]
    return ops.conv_desc(N, Cin, H, W, Cout, k, s, p)


def weight_of(name, seed=2):
    _, tr, _, Cin, _, _, Cout, k, _, _ = DGRAD[name]
    return rand((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), seed, 0.1)


def computed_channels(name):
    route, tr = DGRAD[name][:2]
    return _lib.lib().fn2_conv_backward_data_computed_channels(C.byref(desc_of(name)), int(tr), route)


def dense_packed(name, w):
    """The operand the route's kernel must read, built from the weight blob in numpy and packed by the oracle -- independent of the strided
    view machinery of fn2_conv_mfma_pack_weights_view / rot180_swap."""
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    Cp = computed_channels(name)
    if route == DECONV_PLANE:     # the transposed 3x3 / 2 / 1 convolution IS the Deconvolution{4, 2, 1} [in = Cout][out = Cin] with zero 4th taps
        w4 = np.zeros((Cout, Cin, 4, 4), np.float32)
        w4[:, :, :3, :3] = w
        return oracle.deconv_plane_pack_weights(w4)
    if route == TCONV:            # the transposed-convolution kernel's operand: the [Cin][Cout] view of the blob, no rotation
        return oracle.conv_mfma_pack_weights(np.ascontiguousarray(w.transpose(1, 0, 2, 3)))
    if tr:                        # a Deconvolution's gradient is the 4x4 / 2 / 1 convolution with the blob as it is ([out = Cin][in = Cout])
        t = w
    elif k == 1:
        t = w.transpose(1, 0, 2, 3)
    else:                         # 3x3 / 1 / 1: rotated by 180 degrees, channel axes swapped
        t = w.transpose(1, 0, 2, 3)[..., ::-1, ::-1]
    dense = np.zeros((Cp,) + t.shape[1:], np.float32)
    dense[:Cin] = t
    return oracle.conv_wino_pack_weights(dense) if route == WINOGRAD else oracle.conv_mfma_pack_weights(dense)


def twin(name, top, packed, w):
    """CPU twin of the kernel the route launches, on the packed operand: the Cp computed channels (TCONV / DECONV_PLANE: Cin)."""
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    Cp = computed_channels(name)
    if route == WINOGRAD:
        return oracle.conv_wino_forward(top, packed, None, Cp, 1, relu=False)
    if route == TCONV:
        return oracle.tconv_forward(top, w, None, k, p, out_hw=(H, W))
    if route == DECONV_PLANE:
        return oracle.deconv_plane_forward(top, packed, None, Cin, ops.deconv_plane_ksplit(N, Cout, Ht, Wt, Cin), relu=False)
    if route == PLANE and tr:
        return oracle.conv_plane_forward(top, packed, None, Cp, 2, 1, ops.conv_plane_k_ksplit(N, Cout, Ht, Wt, Cp, 4, 2, 1), relu=False, kernel=4)
    if route == PLANE:
        return oracle.conv_plane_forward(top, packed, None, Cp, 1, 1, ops.conv_plane_ksplit(N, Cout, Ht, Wt, Cp, 1, 1), relu=False)
    if tr:
        return oracle.conv_mfma_forward(top, packed, None, Cp, 4, 2, 1, relu=False)
    return oracle.conv_mfma_forward(top, packed, None, Cp, 1, 1, 0, relu=False)


def dgrad64(name, top, w):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    x = torch.zeros((N, Cin, H, W), dtype=torch.float64)
    return torch.ops.aten.convolution_backward(torch.from_numpy(top).double(), x, torch.from_numpy(w).double(), None, [s, s], [p, p], [1, 1], tr,
                                               [0, 0], 1, [True, False, False])[0].numpy()


def top_of(name, seed=1):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    return rand((N, Cout, Ht, Wt), seed)


# ---------------------------------------------------------------------------------------------------------------------------------------
# host: routing, coverage, the decomposition itself


@pytest.mark.parametrize("name", list(DGRAD))
def test_every_case_takes_its_route(name):
    route, tr = DGRAD[name][:2]
    d = desc_of(name)
    assert ops.conv_backward_data_route(d, tr) == route, name
    Cp = computed_channels(name)
    Cin = DGRAD[name][3]
    assert Cp >= Cin and (Cp == Cin or route not in (TCONV, DECONV_PLANE))
    assert ops.conv_backward_data_masked_supported(d, tr, route) == (route == TCONV)


def test_case_lists_cover_every_route_and_form():
    forms = {(DGRAD[n][0], DGRAD[n][1]) for n in DGRAD if ops.conv_backward_data_route(desc_of(n), DGRAD[n][1]) == DGRAD[n][0]}
    assert {r for r, _ in forms} == {WINOGRAD, TCONV, PLANE, DIRECT, DECONV_PLANE}
    assert {(PLANE, False), (PLANE, True), (DIRECT, False), (DIRECT, True)} <= forms
    assert any(ops.conv_backward_data_masked_supported(desc_of(n), DGRAD[n][1], DGRAD[n][0]) for n in DGRAD)
    # the geometry a dispatcher refuses: no route, no packing, no computed channels
    d = ops.conv_desc(2, 40, 9, 12, 33, 3, 2, 2)
    assert ops.conv_backward_data_route(d, False) == NONE and computed_channels_of(d, False, NONE) == 0


def test_forward_routes_refuse_geometries_without_a_tile_variant():
    """fn2_conv_mfma_supported answers for the tile variants too: only the 1x1 tiles block Cout by 32, so a Convolution{5, 2, 2} with 96
    outputs has no direct kernel (it used to be routed DIRECT and to fail at launch); it takes the counted last resort."""
    assert not ops.conv_mfma_supported(64, 16, 24, 96, 5, 2, 2) and ops.conv_route(2, 64, 16, 24, 96, 5, 2, 2) is None
    for k, s, p in [(3, 1, 1), (3, 2, 1), (4, 2, 1), (5, 2, 2), (7, 2, 3)]:
        assert not ops.conv_mfma_supported(64, 16, 24, 32, k, s, p) and ops.conv_mfma_supported(64, 16, 24, 64, k, s, p)
    assert ops.conv_mfma_supported(64, 16, 24, 32, 1, 1, 0) and ops.conv_mfma_supported(37, 6, 10, 96, 1, 1, 0)


def computed_channels_of(d, tr, route):
    return _lib.lib().fn2_conv_backward_data_computed_channels(C.byref(d), int(tr), route)


def flownetc_training_layers(B=8, H=320, W=448):
    """(name, kind, N, Cin, Hb, Wb, Cout, k, s, p) of every Convolution / Deconvolution of the FlowNetC training graph, derived from
    nets.layer_table: the siamese layers conv1-3 run on both towers (2B samples); a convolution takes the current map and scales it by its
    stride, a deconvolution takes the current map, and the decoder convolution after it runs at twice the resolution."""
    out, r, after_deconv = [], 1, False
    for (name, kind, ci, co, k, s, p) in nets.layer_table("C"):
        n = 2 * B if name in ("conv1", "conv2", "conv3") else B
        if kind == "conv":
            if after_deconv:
                r, after_deconv = r // 2, False
            out.append((name, kind, n, ci, H // r, W // r, co, k, s, p))
            r *= s
        else:
            out.append((name, kind, n, ci, H // r, W // r, co, k, s, p))
            after_deconv = True
    return out


def test_flownetc_training_graph_has_an_own_backward_for_every_layer():
    layers = flownetc_training_layers()
    # the derivation reproduces the layer sizes nets.conv_flops counts with
    flops = 0.0
    for (name, kind, n, ci, h, w, co, k, s, p) in layers:
        if kind == "conv":
            flops += 2.0 * n * ((h + 2 * p - k) // s + 1) * ((w + 2 * p - k) // s + 1) * co * ci * k * k
        else:
            flops += 2.0 * n * h * w * ci * co * k * k
    assert flops == 8 * nets.conv_flops("C", 320, 448)
    L = _lib.lib()
    for (name, kind, n, ci, h, w, co, k, s, p) in layers:
        d = ops.conv_desc(n, ci, h, w, co, k, s, p)
        tr = kind == "deconv"
        if tr and ci == 2 and co == 2:           # upsample_flow*: the 2-channel head kernel (fn2_upsample_flow_deconv_backward)
            assert L.fn2_deconv_route(C.byref(d), 0) == 3, name
            continue
        if not tr and co == 2:                   # predict_flow*: the flow-head backward kernel (fn2_predict_flow_conv_backward)
            assert L.fn2_predict_flow_conv_backward_supported(n, ci, h, w) == 1, name
            continue
        if name != "conv1":                      # conv1's bottom is the image: no data gradient
            assert ops.conv_backward_data_route(d, tr) != NONE, name
        assert ops.conv_backward_weights_supported(d, tr), name
    assert ops.conv_backward_weights_bias_fused(ops.conv_desc(*layers[0][2:]), False)


def family_training_layers(case, B, H=320, W=448):
    """(name, kind, N, Cin, Hb, Wb, Cout, k, s, p) of every Convolution / Deconvolution of the FlowNetS ("S6", "S12"), FlowNet-SD ("SD") and
    fusion ("fusion") training graphs (tests/test_train_parity_family.py): FlowNetS from nets.layer_table like FlowNetC (one tower); SD and
    fusion from their tables and the OUTPUT resolution divisor of every layer (nets._SD_RES / _FUSE_RES): a convolution's bottom is at
    divisor / stride, a deconvolution's at twice its divisor."""
    if case in ("S6", "S12"):
        out, r, after_deconv = [], 1, False
        for (name, kind, ci, co, k, s, p) in nets.layer_table("S", 6 if case == "S6" else 12):
            if kind == "conv" and after_deconv:
                r, after_deconv = r // 2, False
            out.append((name, kind, B, ci, H // r, W // r, co, k, s, p))
            if kind == "conv":
                r *= s
            else:
                after_deconv = True
        return out
    table, res = (nets._SD_TABLE, nets._SD_RES) if case == "SD" else (nets._FUSE_TABLE, nets._FUSE_RES)
    return [(name, kind, B, ci, H // (res[name] // s if kind == "conv" else 2 * res[name]), W // (res[name] // s if kind == "conv" else 2 * res[name]),
             co, k, s, p) for (name, kind, ci, co, k, s, p) in table]


def library_parts(layers):
    """{layer: parts of its training step that no own kernel computes} by descriptor: "forward" (the library's autograd then computes both
    gradients of the layer), else "data" (every layer but the first: its bottom is the input blob) and / or "weight"."""
    from flownet2_amd import functional as Fn
    L = _lib.lib()
    gaps = {}
    for i, (name, kind, n, ci, h, w, co, k, s, p) in enumerate(layers):
        d = ops.conv_desc(n, ci, h, w, co, k, s, p)
        tr = kind == "deconv"
        if tr and ci == 2 and co == 2:           # upsample_flow*: the 2-channel head kernel, forward and backward (fn2_upsample_flow_deconv_*)
            assert L.fn2_deconv_route(C.byref(d), 0) == 3, name
            continue
        if not tr and co == 2:                   # predict_flow*: the flow-head kernels (fn2_predict_flow_conv_*)
            assert L.fn2_conv_route(C.byref(d), 0) == 5 and L.fn2_predict_flow_conv_backward_supported(n, ci, h, w) == 1, name
            continue
        # the forward a training graph runs: functional.conv_mfma_relu (stem / Winograd / small-map / direct) or, for a Deconvolution,
        # deconv_relu (GEMM + col2im, or the small-map kernel) -- the library's route minus what those two decline
        if (Fn.deconv_forward_route(d) if tr else Fn.conv_forward_route(d)) != NONE:
            parts = tuple(part for part, ok in (("data", i == 0 or ops.conv_backward_data_route(d, tr) != NONE),
                                                ("weight", ops.conv_backward_weights_supported(d, tr))) if not ok)
        else:
            parts = ("forward",)
        if parts:
            gaps[name] = parts
    return gaps


def test_family_training_graphs_have_an_own_backward_for_every_layer_but_the_allow_listed():
    """FlowNetS (6 and 12 input channels), FlowNet-SD and the fusion net at the sizes of tests/test_train_parity_family.py: every layer has an
    own forward, data-gradient (all but the first) and weight-gradient route, except the layers that file lists -- exactly those."""
    from test_train_parity_family import CASES, LIBRARY_LAYERS
    flops_of = {"S6": lambda H, W: nets.conv_flops("S", H, W, 6), "S12": lambda H, W: nets.conv_flops("S", H, W, 12),
                "SD": lambda H, W: nets._table_flops(nets._SD_TABLE, nets._SD_RES, H, W),
                "fusion": lambda H, W: nets._table_flops(nets._FUSE_TABLE, nets._FUSE_RES, H, W)}
    found = {}
    for case, (B, H, W) in CASES.items():
        layers = family_training_layers(case, B, H, W)
        flops = 0.0         # the derivation reproduces the layer sizes the FLOP model counts with
        for (name, kind, n, ci, h, w, co, k, s, p) in layers:
            if kind == "conv":
                flops += 2.0 * n * ((h + 2 * p - k) // s + 1) * ((w + 2 * p - k) // s + 1) * co * ci * k * k
            else:
                flops += 2.0 * n * h * w * ci * co * k * k
        assert flops == B * flops_of[case](H, W), case
        found.update({(case, name): parts for name, parts in library_parts(layers).items()})
    assert found == {key: parts for key, (parts, _why) in LIBRARY_LAYERS.items()}


def test_forward_routes_python_declines_although_the_library_has_one():
    """functional.conv_forward_route / deconv_forward_route = the library's route minus a fixed list of layers (the graphs send those to
    the flow-head entry points or to the counted library call): pinned here, independently of library_parts, which asks the same functions."""
    from flownet2_amd import functional as Fn
    L = _lib.lib()
    dec = ops.conv_desc(2, 64, 10, 14, 32, 4, 2, 1)
    assert L.fn2_deconv_route(C.byref(dec), 0) == 1 and Fn.deconv_forward_route(dec) == 1
    assert Fn.deconv_forward_route(dec, act=False) == NONE                                   # a Deconvolution without ReLU
    small = ops.conv_desc(2, 32, 10, 14, 32, 4, 2, 1)
    assert L.fn2_deconv_route(C.byref(small), 0) == 1 and Fn.deconv_forward_route(small) == NONE        # fewer than 64 input channels
    up = ops.conv_desc(2, 2, 10, 14, 2, 4, 2, 1)
    assert L.fn2_deconv_route(C.byref(up), 0) == 3 and Fn.deconv_forward_route(up, act=False) == NONE == Fn.deconv_forward_route(up)      # HEAD
    stem = ops.conv_desc(2, 3, 64, 128, 64, 7, 2, 3)
    assert L.fn2_conv_route(C.byref(stem), 0) == 4 and Fn.conv_forward_route(stem) == 4
    assert Fn.conv_forward_route(stem, act=False) == NONE and Fn.conv_forward_route(stem, whole_blobs=False) == NONE      # the stem: ReLU, whole blobs
    head = ops.conv_desc(2, 194, 20, 28, 2, 3, 1, 1)
    assert L.fn2_conv_route(C.byref(head), 0) == 5 and Fn.conv_forward_route(head) == NONE and Fn.conv_forward_route(head, act=False) == NONE
    k4 = ops.conv_desc(2, 64, 16, 24, 64, 4, 2, 1)                                            # the direct kernel on 4x4 taps, 7x7 off channel quads
    assert L.fn2_conv_route(C.byref(k4), 0) == 1 and Fn.conv_forward_route(k4) == NONE
    k7 = ops.conv_desc(2, 3, 64, 100, 64, 7, 2, 3)
    assert L.fn2_conv_route(C.byref(k7), 0) == 1 and Fn.conv_forward_route(k7) == NONE
    quad = ops.conv_desc(2, 12, 64, 128, 64, 7, 2, 3)
    assert L.fn2_conv_route(C.byref(quad), 0) == 1 and Fn.conv_forward_route(quad) == 1 and Fn.conv_forward_route(quad, act=False) == 1
    assert Fn.conv_route_name((2, 3, 64, 128), torch.empty(64, 3, 7, 7), 2, 3) == "stem"


def test_weight_gradient_support_needs_16_channels_on_both_sides():
    for (N, Cin, H, W, Cout, k, s, p, tr) in [(2, 24, 7, 12, 48, 3, 1, 1, False), (2, 32, 9, 16, 64, 3, 2, 1, False),
                                              (2, 40, 6, 10, 32, 1, 1, 0, False), (2, 48, 5, 8, 32, 4, 2, 1, True)]:
        assert ops.conv_backward_weights_supported(ops.conv_desc(N, Cin, H, W, Cout, k, s, p), tr)
        assert not ops.conv_backward_weights_supported(ops.conv_desc(N, 8, H, W, Cout, k, s, p), tr)
        assert not ops.conv_backward_weights_supported(ops.conv_desc(N, Cin, H, W, 8, k, s, p), tr)


@pytest.mark.parametrize("name", list(DGRAD))
def test_oracle_decomposition_matches_fp64(name):
    """The route's decomposition itself (operand built in numpy, the twin of the launched kernel) against fp64, on the host."""
    route = DGRAD[name][0]
    Cin = DGRAD[name][3]
    w, top = weight_of(name), top_of(name)
    got = twin(name, top, dense_packed(name, w), w)
    ref = dgrad64(name, top, w)
    assert np.abs(got[:, :Cin] - ref).max() <= TOL[route] * scale_of(ref)
    assert not got[:, Cin:].any()                # the surplus channels are zeros


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: data gradient by descriptor


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_bwd_data(name, packed, top_blob, top_c0, out_blob, bottom_c0, room):
    """fn2_conv_backward_data on host blobs (copied to the device); returns the whole output blob."""
    route, tr = DGRAD[name][:2]
    d = desc_of(name)
    L = _lib.lib()
    need = int(L.fn2_conv_backward_data_workspace_bytes_with_room(C.byref(d), int(tr), route, room))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
    t, o = dev(top_blob), dev(out_blob)
    check(L.fn2_conv_backward_data(C.byref(d), int(tr), route, ops._ptr(t), t.shape[1], top_c0, ops._ptr(packed), ops._ptr(o), o.shape[1], bottom_c0,
                                   room, ops._ptr(ws), need, ops._stream()))
    torch.cuda.synchronize()
    return o.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DGRAD))
def test_data_gradient_route(name):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    d = desc_of(name)
    assert ops.conv_backward_data_route(d, tr) == route
    Cp = computed_channels(name)
    w, top = weight_of(name), top_of(name)
    # (a) the packed operand
    packed = ops.conv_backward_data_pack_weights(dev(w), d, tr, route)
    want_packed = dense_packed(name, w)
    assert same_bits(packed.cpu().numpy(), want_packed), "packed operand"
    # (b) room for the Cp computed channels (the Python wrapper's form): the twin's bits, surplus channels included
    want = twin(name, top, want_packed, w)
    room = run_bwd_data(name, packed, top, 0, np.full((N, Cp, H, W), SENTINEL), 0, Cp)
    assert same_bits(room[:, :want.shape[1]], want), float(np.abs(room[:, :want.shape[1]] - want).max())
    # (c) fp64
    ref = dgrad64(name, top, w)
    assert np.abs(room[:, :Cin] - ref).max() <= TOL[route] * scale_of(ref)
    # (d) no room for the surplus: through the workspace into channels [3, 3 + Cin) of a wider blob; the neighbours keep their sentinel
    padded = run_bwd_data(name, packed, top, 0, np.full((N, Cin + 7, H, W), SENTINEL), 3, Cin)
    assert same_bits(padded[:, 3:3 + Cin], room[:, :Cin])
    assert (padded[:, :3] == SENTINEL).all() and (padded[:, 3 + Cin:] == SENTINEL).all()
    #     top_diff as channels [5, 5 + Cout) of a wider blob
    wide = rand((N, Cout + 8, Ht, Wt), 9)
    wide[:, 5:5 + Cout] = top
    sliced = run_bwd_data(name, packed, wide, 5, np.full((N, Cp, H, W), SENTINEL), 0, Cp)
    assert same_bits(sliced, room)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the masked data gradient (ReLUBackward of the layer in front folded into the TCONV route)

MASKED = [n for n in DGRAD if DGRAD[n][0] == TCONV]


def bottom_data_of(name, seed=5):
    """The layer's bottom = the activated output of the layer in front, as channels [4, 4 + Cin) of a wider blob: +x, -x, 0.0 and -0.0."""
    route, tr, N, Cin, H, W = DGRAD[name][:6]
    y = rand((N, Cin + 6, H, W), seed)
    flat = y.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return y


def run_masked(name, packed, top_blob, top_c0, y_blob, data_c0, out_blob, bottom_c0, slope, misalign=False):
    route, tr = DGRAD[name][:2]
    d = desc_of(name)
    t, o = dev(top_blob), dev(out_blob)
    yd = torch.empty(y_blob.size + 4, dtype=torch.float32, device="cuda")
    off = 1 if misalign else 0                   # 1 float: 4 bytes off the 16-byte alignment of the allocation
    yd[off:off + y_blob.size] = dev(y_blob.reshape(-1))
    try:
        check(_lib.lib().fn2_conv_backward_data_masked(C.byref(d), int(tr), route, ops._ptr(t), t.shape[1], top_c0, ops._ptr(packed), ops._ptr(o),
                                                       o.shape[1], bottom_c0, C.c_void_p(yd.data_ptr() + 4 * off), y_blob.shape[1], data_c0,
                                                       C.c_float(slope), ops._stream()))
    finally:
        torch.cuda.synchronize()
        out_blob[...] = o.cpu().numpy()
    return out_blob


@pytest.mark.gpu
@pytest.mark.parametrize("name", MASKED)
def test_masked_data_gradient(name):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    d = desc_of(name)
    assert ops.conv_backward_data_masked_supported(d, tr, route) and computed_channels(name) == Cin
    w, top, y = weight_of(name), top_of(name), bottom_data_of(name)
    packed = ops.conv_backward_data_pack_weights(dev(w), d, tr, route)
    slope = 0.1
    wide = rand((N, Cout + 8, Ht, Wt), 9)
    wide[:, 5:5 + Cout] = top
    got = run_masked(name, packed, wide, 5, y, 4, np.full((N, Cin + 5, H, W), SENTINEL), 2, slope)
    assert (got[:, :2] == SENTINEL).all() and (got[:, 2 + Cin:] == SENTINEL).all()
    plain = run_bwd_data(name, packed, top, 0, np.full((N, Cin, H, W), SENTINEL), 0, Cin)
    yv = y[:, 4:4 + Cin]
    want = plain * np.where(yv > 0, np.float32(1.0), np.float32(slope))          # bias_leaky_relu_bwd's expression, fp32
    assert same_bits(got[:, 2:2 + Cin], want)
    ref = dgrad64(name, top, w) * np.where(yv > 0, 1.0, slope)
    assert np.abs(got[:, 2:2 + Cin] - ref).max() <= TOL[route] * scale_of(ref)
    # the zeros of either sign take the slope: those units must carry a gradient for that to be seen
    z = yv == 0
    assert z.any() and np.signbit(yv[z]).any() and np.abs(plain[z]).max() > 0


@pytest.mark.gpu
def test_masked_data_gradient_refuses_other_routes_and_misaligned_masks():
    for name in DGRAD:
        route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
        if route == TCONV:
            continue
        assert not ops.conv_backward_data_masked_supported(desc_of(name), tr, route), name
        w = weight_of(name)
        packed = ops.conv_backward_data_pack_weights(dev(w), desc_of(name), tr, route)
        out = np.full((N, Cin, H, W), SENTINEL)
        with pytest.raises(Fn2Error):
            run_masked(name, packed, top_of(name), 0, rand((N, Cin, H, W), 5), 0, out, 0, 0.1)
        assert (out == SENTINEL).all(), name
    name = MASKED[0]
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    packed = ops.conv_backward_data_pack_weights(dev(weight_of(name)), desc_of(name), tr, route)
    out = np.full((N, Cin, H, W), SENTINEL)
    with pytest.raises(Fn2Error, match="aligned"):
        run_masked(name, packed, top_of(name), 0, bottom_data_of(name), 4, out, 0, 0.1, misalign=True)
    assert (out == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: weight gradients by descriptor

# (N, Cin, H, W, Cout, kernel, stride, pad, transposed); bottom and top_diff are channel slices of wider blobs
WGRAD = [(2, 40, 6, 10, 32, 1, 1, 0, False), (2, 24, 7, 12, 48, 3, 1, 1, False), (2, 32, 9, 16, 64, 3, 2, 1, False),
         (1, 64, 16, 24, 32, 5, 2, 2, False), (2, 48, 5, 8, 32, 4, 2, 1, True)]


def guarded(a):
    """a on the device at the start of an allocation four times its size larger: a kernel that takes one blob's geometry for the other's
    (the a / b roles of a Deconvolution swapped) then reads wrong values instead of reading past the allocation."""
    buf = torch.zeros(5 * a.size, device="cuda")
    buf[:a.size] = dev(a.reshape(-1))
    return buf[:a.size].view(a.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", WGRAD)
def test_weight_gradient(case):
    N, Cin, H, W, Cout, k, s, p, tr = case
    d = ops.conv_desc(N, Cin, H, W, Cout, k, s, p)
    assert ops.conv_backward_weights_supported(d, tr)
    Ho, Wo = (2 * H, 2 * W) if tr else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    xb, gb = rand((N, Cin + 5, H, W), 1), rand((N, Cout + 6, Ho, Wo), 2)         # bottom: channels [3, 3 + Cin); top_diff: [4, 4 + Cout)
    xd, gd = guarded(xb), guarded(gb)
    got = ops.conv_backward_weights(xd, gd, d, tr, bottom_c0=3, top_c0=4).cpu().numpy()
    start = rand(got.shape, 3)
    acc = ops.conv_backward_weights(xd, gd, d, tr, out=dev(start), accumulate=True, bottom_c0=3, top_c0=4).cpu().numpy()
    assert same_bits(acc, start + got)
    # the twin on the pair the header documents: Convolution a = top_diff, b = bottom; Deconvolution a = bottom, b = top_diff
    if tr:
        a, a0, Ca, b, b0, Cb, Ha, Wa, Hb, Wb = xb, 3, Cin, gb, 4, Cout, H, W, Ho, Wo
    else:
        a, a0, Ca, b, b0, Cb, Ha, Wa, Hb, Wb = gb, 4, Cout, xb, 3, Cin, Ho, Wo, H, W
    ks = ops.conv_wgrad_ksplit(N, Ca, Ha, Wa, Cb, Hb, Wb, k, s, p)
    assert same_bits(got, oracle.conv_wgrad(a, b, k, s, p, ks, a_c0=a0, Ca=Ca, b_c0=b0, Cb=Cb))
    x64, g64 = torch.from_numpy(xb[:, 3:3 + Cin]).double(), torch.from_numpy(gb[:, 4:4 + Cout]).double()
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    ref = torch.ops.aten.convolution_backward(g64, x64, torch.zeros(wshape, dtype=torch.float64), None, [s, s], [p, p], [1, 1], tr, [0, 0], 1,
                                              [False, True, False])[1].numpy()
    assert np.abs(got - ref).max() <= 2e-6 * scale_of(ref) * np.sqrt(N * Ha * Wa)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2, 3, 17, 32), (1, 6, 11, 40), (1, 12, 9, 16)])      # N, Cin, H (odd), W
def test_stem_fused_weight_and_bias_gradient(case):
    N, Cin, H, W = case
    d = ops.conv_desc(N, Cin, H, W, 64, 7, 2, 3)
    assert ops.conv_backward_weights_bias_fused(d, False)
    x, g = rand((N, Cin, H, W), 1), rand((N, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1), 2)
    xd, gd = dev(x), dev(g)
    L = _lib.lib()
    need = int(L.fn2_conv_backward_weights_workspace_bytes(C.byref(d), 0))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")

    def fused(dw, db, accumulate):
        check(L.fn2_conv_backward_weights_bias(C.byref(d), 0, ops._ptr(xd), ops._ptr(gd), ops._ptr(dw), ops._ptr(db), int(accumulate), ops._ptr(ws),
                                               need, ops._stream()))
        torch.cuda.synchronize()
        return dw.cpu().numpy(), db.cpu().numpy()

    dw, db = fused(torch.empty((64, Cin, 7, 7), device="cuda"), torch.empty(64, device="cuda"), False)
    assert same_bits(dw, ops.conv_backward_weights(xd, gd, d, False).cpu().numpy())
    ref_b = g.astype(np.float64).sum((0, 2, 3))
    assert np.abs(db - ref_b).max() <= 2e-6 * scale_of(ref_b)
    sw, sb = rand(dw.shape, 3), rand(db.shape, 4)
    aw, ab = fused(dev(sw), dev(sb), True)
    assert same_bits(aw, sw + dw) and same_bits(ab, sb + db)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: through autograd (functional.conv_mfma_relu / deconv_relu), output into a Concat-like blob, upstream gradient a channel slice

AUTOGRAD = ["wino-odd-batch", "tconv-5x5-c128", "deconv-plane-10x14", "plane-5x7", "direct-1x1", "plane-deconv", "direct-deconv"]


def own_forward(name, x, w, b, blob, c0):
    from flownet2_amd import functional as Fn
    route, tr, N, Cin, H, W, Cout, k, s, p = DGRAD[name]
    if tr:
        return Fn.deconv_relu(x, w, b, 0.1, True, out=blob, out_c0=c0)
    return Fn.conv_mfma_relu(x, w, b, s, p, 0.1, True, out=blob, out_c0=c0)


def autograd_step(name, x, w, b, G):
    """Own forward into channels [3, 3 + Cout) of a blob, backward with the gradient of channels [4, 4 + Cout) of G; returns the output."""
    from flownet2_amd import functional as Fn
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    blob = torch.zeros((N, Cout + 7, Ht, Wt), device="cuda")
    y = own_forward(name, x, w, b, blob, 3)
    assert y is not None, name
    torch.autograd.backward(y, G[:, 4:4 + Cout])
    Fn.join_side_streams()
    torch.cuda.synchronize()
    return y.detach()


def grads64(name, x, w, b, y32, g):
    """fp64 gradients on the fp32 run's ReLU branch (the mask is the sign of the fp32 output, as fp64_graph.record_relu_branches takes it)."""
    route, tr, N, Cin, H, W, Cout, k, s, p = DGRAD[name]
    x64, w64, b64 = (t.detach().cpu().double().requires_grad_(True) for t in (x, w, b))
    z = (torch.nn.functional.conv_transpose2d(x64, w64, b64, stride=2, padding=1) if tr
         else torch.nn.functional.conv2d(x64, w64, b64, stride=s, padding=p))
    gz = g.detach().cpu().double() * torch.where(y32.cpu() > 0, 1.0, 0.1).double()
    return torch.autograd.grad(z, (x64, w64, b64), gz)


def check_grads(name, x, w, b, y32, g):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    gx, gw, gb = grads64(name, x, w, b, y32, g)
    assert float((x.grad.cpu().double() - gx).abs().max()) <= TOL[route] * max(1.0, float(gx.abs().max())), "x.grad"
    Ha, Wa = (H, W) if tr else (Ht, Wt)                    # the map at the convolution's output resolution (conv_wgrad.hip's `a`)
    assert float((w.grad.cpu().double() - gw).abs().max()) <= 2e-6 * max(1.0, float(gw.abs().max())) * np.sqrt(N * Ha * Wa), "w.grad"
    assert float((b.grad.cpu().double() - gb).abs().max()) <= 2e-6 * max(1.0, float(gb.abs().max())) * np.sqrt(N * Ht * Wt), "b.grad"


def leaves(name, seed):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    x = dev(rand((N, Cin, H, W), seed)).requires_grad_(True)
    w = torch.nn.Parameter(dev(weight_of(name, seed + 1)))
    b = torch.nn.Parameter(dev(rand((Cout,), seed + 2, 0.1)))
    G = dev(rand((N, Cout + 9, Ht, Wt), seed + 3))
    return x, w, b, G


@pytest.mark.gpu
@pytest.mark.parametrize("name", AUTOGRAD)
def test_autograd_through_the_routes(name, monkeypatch):
    from flownet2_amd import functional as Fn
    monkeypatch.setenv("FN2_STRICT", "1")
    before = Fn.LIBRARY_FALLBACKS[0]
    Cout = DGRAD[name][6]
    x, w, b, G = leaves(name, 21)
    y = autograd_step(name, x, w, b, G)
    assert Fn.LIBRARY_FALLBACKS[0] == before
    check_grads(name, x, w, b, y, G[:, 4:4 + Cout])


@pytest.mark.gpu
def test_forward_without_a_tile_variant_is_left_to_the_caller():
    from flownet2_amd import functional as Fn
    x, w = dev(rand((2, 64, 16, 24), 1)), dev(rand((96, 64, 5, 5), 2, 0.1))
    assert Fn.conv_mfma_relu(x, w, None, 2, 2) is None


@pytest.mark.gpu
def test_data_gradient_pack_cache_follows_a_fused_optimizer_step(monkeypatch):
    from flownet2_amd import functional as Fn
    monkeypatch.setenv("FN2_STRICT", "1")
    before = Fn.LIBRARY_FALLBACKS[0]
    name = "wino-odd-batch"
    Cout = DGRAD[name][6]
    x, w, b, G = leaves(name, 31)
    autograd_step(name, x, w, b, G)
    first = x.grad.clone()
    opt = torch.optim.Adam([w, b], lr=0.05, fused=True)
    opt.step()
    for t in (x, w, b):
        t.grad = None
    y = autograd_step(name, x, w, b, G)
    assert float((x.grad - first).abs().max()) > 0.05 * float(first.abs().max())      # the step moved the data gradient
    check_grads(name, x, w, b, y, G[:, 4:4 + Cout])                                  # ... to the new weights' gradient
    assert Fn.LIBRARY_FALLBACKS[0] == before
