"""Forward by descriptor (csrc/conv_route.cpp): fn2_conv_route / fn2_deconv_route -> fn2_conv_pack_weights / fn2_deconv_pack_weights ->
fn2_conv_workspace_bytes / fn2_deconv_workspace_bytes -> fn2_conv_forward / fn2_deconv_forward, the call sequence every Convolution and
Deconvolution of every FlowNet graph makes, from functional.conv_mfma_relu / deconv_relu and from the Caffe adapter alike.

Every forward route (Convolution: DIRECT at 5x5 / 2, 3x3 / 2, 7x7 / 2 and 1x1, WINOGRAD by the occupancy threshold and by the fallthrough,
PLANE through both entry points, STEM, HEAD; Deconvolution{4, 2, 1}: GEMM, PLANE, HEAD) is pinned on its own, through ops.conv_pack_weights
and ops.conv_forward only: the packed operand equals, bit for bit, the oracle's packing of the operand built here in numpy from the weight
blob; the result equals the oracle twin of the kernel the route launches on that operand (bit for bit where the kernel's own test claims
bit identity, at that test's bound otherwise) and matches fp64 (torch's conv2d / conv_transpose2d + leaky ReLU on the CPU) at the bound of
the kernel's own forward test; the flags (ReLU, bias, negative_slope) and the four blob forms (fresh top, top a channel slice of a
sentinel-filled blob, bottom a channel slice of a wider blob, both) give the same bits.  Then what the dispatchers refuse on the host,
batch-invariant mode and FN2_ROUTE_FORCE, the Python layer (slice views, out= / out_c0=, autograd, the forward operand cache) and, on the
host, every Convolution / Deconvolution of the deploy graphs at the benchmark sizes: each has a forward route of a class this file runs."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from flownet2_amd import Fn2Error, _lib, nets, ops
from flownet2_amd._lib import check
from test_conv_backward_routes import dev, family_training_layers, flownetc_training_layers, rand, same_bits, scale_of

NONE, DIRECT, WINOGRAD, PLANE, STEM, HEAD = range(6)            # FN2_CONV_ROUTE_*
D_NONE, D_GEMM, D_PLANE, D_HEAD = range(4)                      # FN2_DECONV_ROUTE_*
SENTINEL = np.float32(-7.25)

# name: (route, transposed, N, Cin, H, W, Cout, kernel, stride, pad) -- the layer's bottom [N, Cin, H, W]; a Deconvolution is {4, 2, 1}
FWD = {
    "direct-5x5": (DIRECT, False, 2, 12, 17, 28, 64, 5, 2, 2),              # conv2 / conv3 class; whole channel quads, not whole octets
    "direct-3x3s2": (DIRECT, False, 2, 20, 17, 28, 64, 3, 2, 1),            # SD / fusion conv1 class
    "direct-7x7": (DIRECT, False, 2, 12, 21, 48, 64, 7, 2, 3),              # the 12-channel stems of the stacked nets
    "direct-1x1": (DIRECT, False, 3, 37, 7, 12, 96, 1, 1, 0),               # conv_redir class; Cout % 32 == 0, not % 64; ragged Cin
    "wino-threshold": (WINOGRAD, False, 3, 13, 65, 76, 64, 3, 1, 1),        # 3 * 9 * 10 * 4 = 1080 accumulator blocks >= 1000; ragged Cin
    "wino-fallthrough": (WINOGRAD, False, 1, 24, 95, 100, 64, 3, 1, 1),     # a small-map geometry but 9500 > 8000 pixels; 624 blocks < 1000
    "plane-3x3s1": (PLANE, False, 2, 24, 5, 7, 64, 3, 1, 1),                # conv5_1 / conv6_1 class
    "plane-3x3s2": (PLANE, False, 3, 24, 11, 13, 64, 3, 2, 1),              # conv5 / conv6 class
    "plane-5x5": (PLANE, False, 1, 24, 17, 28, 64, 5, 2, 2),                # conv3 with one sample: fn2_conv_plane_k_forward
    "stem-3": (STEM, False, 2, 3, 17, 32, 64, 7, 2, 3),
    "stem-6": (STEM, False, 1, 6, 11, 40, 64, 7, 2, 3),
    "head": (HEAD, False, 2, 37, 9, 11, 2, 3, 1, 1),                        # predict_flow*
    "deconv-gemm": (D_GEMM, True, 3, 70, 5, 8, 34, 4, 2, 1),                # M = 16 * 34 = 544: % 32 == 0, Cout itself is not
    "deconv-plane": (D_PLANE, True, 2, 70, 5, 7, 64, 4, 2, 1),              # deconv5 class: H W % 4 != 0
    "deconv-head": (D_HEAD, True, 3, 2, 5, 7, 2, 4, 2, 1),                  # upsample_flow*
}
# (the Winograd kernel takes pad 1 only -- fn2_conv_wino_supported: pad == 1, Win % 4 == 0 -- so there is no second pad to run; the small-map
# kernel takes whole channel octets, the direct kernel whole output-channel blocks of 64 (1x1: 32) on widths that are multiples of 4)
CONV_CASES = [n for n in FWD if not FWD[n][1]]

# fp64 bound of each kernel's own forward test, x max(1, |ref|max):
#   DIRECT 4e-6: test_conv_mfma.py::test_conv_mfma_at_flownet_shapes;  WINOGRAD 6e-6: test_conv_wino.py::test_winograd_at_flownet_shapes;
#   PLANE 4e-6: test_conv_plane.py::test_conv_plane_at_flownet_shapes;  STEM 5e-6: test_gpu_parity.py::test_stem_conv_k7s2_relu;
#   HEAD 3e-6: test_gpu_parity.py::test_predict_flow_conv;  Deconvolution GEMM 3e-6: test_gpu_parity.py::test_deconv_via_gemm_and_col2im;
#   Deconvolution PLANE 4e-6: test_conv_plane.py::test_deconv_plane_at_flownet_shapes;  Deconvolution HEAD 1e-6: test_gpu_parity.py::test_upsample_flow_deconv
TOL = {(False, DIRECT): 4e-6, (False, WINOGRAD): 6e-6, (False, PLANE): 4e-6, (False, STEM): 5e-6, (False, HEAD): 3e-6,
       (True, D_GEMM): 3e-6, (True, D_PLANE): 4e-6, (True, D_HEAD): 1e-6}
# against the twin: None = bit for bit (test_conv_mfma / test_conv_wino / test_conv_plane: "equals_oracle_bitwise_in_every_variant"; col2im and
# bias + ReLU: test_gpu_parity.py::test_deconv_via_gemm_and_col2im / test_bias_leaky_relu_inplace); the three kernels whose twins sum in another
# order have the bound of their own test against the twin: test_stem_conv_k7s2_relu 5e-6, test_predict_flow_conv 3e-6, test_upsample_flow_deconv 1e-6
TWIN_TOL = {(False, STEM): 5e-6, (False, HEAD): 3e-6, (True, D_HEAD): 1e-6}
# the whole-size runs: test_conv_mfma.py::test_conv_mfma_at_flownet_shapes (MIOpen fp32 everywhere, fp64 on sample 0)
LIB_TOL, FP64_TOL = 1e-5, 4e-6


def geom(name):
    route, tr, N, Cin, H, W, Cout, k, s, p = FWD[name]
    Ht, Wt = (2 * H, 2 * W) if tr else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    return route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt


def desc_of(name, N=None):
    _, tr, n, Cin, H, W, Cout, k, s, p = FWD[name]
    return ops.conv_desc(n if N is None else N, Cin, H, W, Cout, k, s, p)


def lib_route(d, tr, flags=0):
    L = _lib.lib()
    return int((L.fn2_deconv_route if tr else L.fn2_conv_route)(C.byref(d), flags))


def entry_of(tr, route, k):
    """The entry point the dispatcher calls: PLANE has two (fn2_conv_plane_forward for 3x3, fn2_conv_plane_k_forward for 5x5 / 2)."""
    if tr:
        return {D_GEMM: "deconv_gemm", D_PLANE: "deconv_plane", D_HEAD: "upsample_flow"}[route]
    if route == PLANE:
        return "conv_plane" if k == 3 else "conv_plane_k"
    return {DIRECT: "conv_mfma", WINOGRAD: "conv_wino", STEM: "conv_k7s2", HEAD: "predict_flow"}[route]


def class_of(tr, route, k, s):
    return (bool(tr), route, k, s, entry_of(tr, route, k))


def weight_of(name, seed=2):
    _, tr, _, Cin, _, _, Cout, k, _, _ = FWD[name]
    return rand((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), seed, 0.1)


def bottom_of(name, seed=1, N=None):
    _, tr, n, Cin, H, W = FWD[name][:6]
    return rand((n if N is None else N, Cin, H, W), seed)


def bias_of(name, seed=3):
    return rand((FWD[name][6],), seed, 0.1)


def dense_packed(name, w):
    """The operand the route's kernel must read, built from the weight blob in numpy and packed by the oracle -- independent of
    fn2_conv_pack_weights / fn2_deconv_pack_weights and of the strided view the GEMM operand goes through."""
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    if tr and route == D_GEMM:        # weight^T: the dense [M = 16 Cout][Cin] matrix, row (co, ky, kx), as a 1x1 convolution's blob
        dense = np.ascontiguousarray(w.reshape(Cin, Cout * 16).T).reshape(Cout * 16, Cin, 1, 1)
        return oracle.conv_mfma_pack_weights(dense)
    if tr and route == D_PLANE:
        return oracle.deconv_plane_pack_weights(w)
    if route in (STEM, HEAD) or (tr and route == D_HEAD):
        return np.ascontiguousarray(w).reshape(-1)      # these kernels read the blob as it is
    if route == WINOGRAD:
        return oracle.conv_wino_pack_weights(w)
    return oracle.conv_mfma_pack_weights(w)             # DIRECT, PLANE


def plane_ksplit(name, N=None):
    route, tr, n, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    n = n if N is None else N
    if tr:
        return ops.deconv_plane_ksplit(n, Cin, H, W, Cout)
    return ops.conv_plane_ksplit(n, Cin, H, W, Cout, s, p) if k == 3 else ops.conv_plane_k_ksplit(n, Cin, H, W, Cout, k, s, p)


def twin(name, x, packed, w, b, relu, slope):
    """CPU twin of what the route launches, on the packed operand (STEM / the heads: on the blob)."""
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    if tr and route == D_GEMM:
        col = oracle.conv_mfma_forward(x, packed, None, Cout * 16, 1, 1, 0, relu=False)              # [N, 16 Cout, H, W]: the column matrix
        return oracle.col2im_bias_relu_forward(col.reshape(N, Cout * 16, H * W), b, N, Cout, Ht, Wt, 4, 1, 2, relu, slope)
    if tr and route == D_PLANE:
        return oracle.deconv_plane_forward(x, packed, b, Cout, plane_ksplit(name), relu, slope)
    if tr:
        assert not relu
        return oracle.upsample_flow_deconv_forward(x, w, b)
    if route == DIRECT:
        return oracle.conv_mfma_forward(x, packed, b, Cout, k, s, p, relu, slope)
    if route == WINOGRAD:
        return oracle.conv_wino_forward(x, packed, b, Cout, p, relu, slope)
    if route == PLANE:
        return oracle.conv_plane_forward(x, packed, b, Cout, s, p, plane_ksplit(name), relu, slope, kernel=k)
    if route == STEM:                 # the kernel always applies t > 0 ? t : t * slope; without a ReLU the dispatcher hands it slope 1
        return oracle.conv_k7s2_relu_forward(x, w, b, slope if relu else 1.0)
    y = oracle.predict_flow_conv_forward(x, w, b)
    return oracle.bias_leaky_relu_forward(y, None, slope) if relu else y


def ref64(name, x, w, b, relu, slope):
    tr, s, p = FWD[name][1], FWD[name][8], FWD[name][9]
    x64, w64 = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    b64 = None if b is None else torch.from_numpy(b).double()
    y = torch.nn.functional.conv_transpose2d(x64, w64, b64, stride=2, padding=1) if tr else torch.nn.functional.conv2d(x64, w64, b64, stride=s, padding=p)
    return (torch.nn.functional.leaky_relu(y, slope) if relu else y).numpy()


def flag_sets(name):
    """(relu, bias present, negative_slope): what the route accepts (the 2-channel Deconvolution head has no fused ReLU)."""
    if FWD[name][1] and FWD[name][0] == D_HEAD:
        return [(False, True, 0.1), (False, False, 0.1)]
    return [(True, True, 0.1), (True, True, 0.0), (True, False, 0.1), (True, False, 0.0), (False, True, 0.1), (False, False, 0.1)]


def slices_of(name):
    """(bottom a slice, top a slice) forms the route accepts besides the fresh one."""
    route, tr = FWD[name][:2]
    if not tr and route in (STEM, HEAD):
        return []
    if tr and route == D_HEAD:
        return [(False, True)]
    return [(False, True), (True, False), (True, True)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# host: routing, coverage, the decomposition itself


@pytest.mark.parametrize("name", list(FWD))
def test_every_case_takes_its_route(name):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    d = desc_of(name)
    assert lib_route(d, tr) == route, name
    assert ops.get_batch_invariant() is False
    L = _lib.lib()
    floats = int((L.fn2_deconv_packed_weight_floats if tr else L.fn2_conv_packed_weight_floats)(C.byref(d), route))
    assert floats == dense_packed(name, weight_of(name)).size
    # the stated reason of the two Winograd cases and of the single-sample 5x5 case
    blocks = N * ((Ht + 7) // 8) * ((Wt + 7) // 8) * (Cout // 16)
    if name == "wino-threshold":
        assert blocks >= 1000
    if name == "wino-fallthrough":
        assert blocks < 1000 and Ht * Wt > 8000 and ops.conv_plane_supported(N, Cin, H, W, Cout, s, p)
    if name == "plane-5x5":
        assert N == 1 and entry_of(tr, route, k) == "conv_plane_k"


def test_case_table_covers_every_route_and_both_plane_entry_points():
    took = {n: lib_route(desc_of(n), FWD[n][1]) for n in FWD}
    assert all(took[n] == FWD[n][0] for n in FWD)
    assert {took[n] for n in FWD if not FWD[n][1]} == {DIRECT, WINOGRAD, PLANE, STEM, HEAD} == set(ops.CONV_FWD_ROUTES) - {NONE}
    assert {took[n] for n in FWD if FWD[n][1]} == {D_GEMM, D_PLANE, D_HEAD} == set(ops.DECONV_FWD_ROUTES) - {D_NONE}
    entries = {entry_of(FWD[n][1], FWD[n][0], FWD[n][7]) for n in FWD}
    assert {"conv_plane", "conv_plane_k"} <= entries
    assert {(FWD[n][7], FWD[n][8]) for n in FWD if FWD[n][0] == DIRECT and not FWD[n][1]} == {(5, 2), (3, 2), (7, 2), (1, 1)}
    assert {(FWD[n][7], FWD[n][8]) for n in FWD if FWD[n][0] == PLANE and not FWD[n][1]} == {(3, 1), (3, 2), (5, 2)}
    assert {FWD[n][3] for n in FWD if FWD[n][0] == STEM} == {3, 6}
    assert not any(ops.conv_wino_supported(13, 65, 76, 64, pad) for pad in (0, 2, 3)) and ops.conv_wino_supported(13, 65, 76, 64, 1)
    assert {FWD[n][2] for n in FWD} == {1, 2, 3}
    # the geometries the dispatchers have nothing for: no route, no operand
    L = _lib.lib()
    d = ops.conv_desc(2, 64, 16, 24, 96, 5, 2, 2)
    assert lib_route(d, False) == NONE and L.fn2_conv_packed_weight_floats(C.byref(d), NONE) == 0
    d = ops.conv_desc(2, 64, 5, 7, 48, 4, 2, 1)
    assert lib_route(d, True) == D_NONE and L.fn2_deconv_packed_weight_floats(C.byref(d), D_NONE) == 0
    assert lib_route(ops.conv_desc(2, 64, 5, 8, 64, 3, 2, 1), True) == D_NONE          # not a Deconvolution{4, 2, 1}


@pytest.mark.parametrize("name", list(FWD))
def test_oracle_decomposition_matches_fp64(name):
    """The route's decomposition itself (operand built in numpy, the twin of what the route launches) against fp64, on the host."""
    route, tr = FWD[name][:2]
    w, x, b = weight_of(name), bottom_of(name), bias_of(name)
    packed = dense_packed(name, w)
    for relu, has_b, slope in flag_sets(name)[:1] + flag_sets(name)[-1:]:
        got = twin(name, x, packed, w, b if has_b else None, relu, slope)
        ref = ref64(name, x, w, b if has_b else None, relu, slope)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= TOL[(tr, route)] * scale_of(ref), (name, relu, has_b, slope)


def invariant(on):
    was = ops.get_batch_invariant()
    ops.set_batch_invariant(on)
    return was


SMALL_WINO = (24, 6, 8, 64, 3, 1, 1)            # a small map the Winograd kernel takes too: PLANE, WINOGRAD when forced or batch-invariant
BATCH_DEPENDENT = (24, 65, 76, 64, 3, 1, 1)     # 360 accumulator blocks per sample: PLANE for one sample, WINOGRAD by the threshold from three on
LARGE_S2 = (1, 24, 181, 200, 64, 3, 2, 1)       # a 3x3 / 2 layer with 91 x 100 > 8000 output pixels: DIRECT, PLANE when forced


def test_batch_invariant_routes_do_not_depend_on_the_batch():
    assert lib_route(ops.conv_desc(1, *BATCH_DEPENDENT), False) == PLANE and lib_route(ops.conv_desc(3, *BATCH_DEPENDENT), False) == WINOGRAD
    was = invariant(True)
    try:
        for name in FWD:
            tr = FWD[name][1]
            one, eight = lib_route(desc_of(name, N=1), tr), lib_route(desc_of(name, N=8), tr)
            assert one == eight != NONE, name
        # decided as for one sample, Winograd first
        assert [lib_route(ops.conv_desc(n, *BATCH_DEPENDENT), False) for n in (1, 3, 8)] == [WINOGRAD] * 3
        assert [lib_route(ops.conv_desc(n, *SMALL_WINO), False) for n in (1, 8)] == [WINOGRAD] * 2
    finally:
        ops.set_batch_invariant(was)
    assert lib_route(ops.conv_desc(1, *BATCH_DEPENDENT), False) == PLANE and lib_route(ops.conv_desc(2, *SMALL_WINO), False) == PLANE


def test_route_force_changes_winograd_and_plane_eligibility():
    """FN2_ROUTE_FORCE (fn2_conv_route's flag 1): Winograd wherever it applies (no occupancy threshold), the small-map kernel whatever the
    map size (no 8000-pixel limit); nothing else moves."""
    small = ops.conv_desc(2, *SMALL_WINO)
    assert lib_route(small, False) == PLANE and lib_route(small, False, 1) == WINOGRAD
    large = ops.conv_desc(*LARGE_S2)
    assert lib_route(large, False) == DIRECT and lib_route(large, False, 1) == PLANE and ops.conv_plane_supported(*LARGE_S2[:5], 2, 1)
    for name in FWD:
        assert lib_route(desc_of(name), FWD[name][1], 1) == FWD[name][0], name
    assert ops.conv_route(2, *SMALL_WINO, force=True) == "wino" and ops.conv_route(2, *SMALL_WINO) == "plane"


# ---------------------------------------------------------------------------------------------------------------------------------------
# host: every Convolution / Deconvolution of the deploy graphs has a forward route of a class the case table runs

PRODUCTION = [("C", 1, 448, 1024), ("S6", 1, 448, 1024), ("S12", 1, 448, 1024), ("SD", 1, 448, 1024), ("fusion", 1, 448, 1024),
              ("C", 4, 384, 768), ("S6", 4, 384, 768), ("S12", 4, 384, 768), ("SD", 4, 384, 768), ("fusion", 4, 384, 768),
              ("C", 8, 320, 448)]          # (graph, batch, H, W); the last one: FlowNetC training


def production_layers():
    """(graph, name, kind, N, Cin, H, W, Cout, k, s, p) of every Convolution / Deconvolution, from nets.layer_table / _SD_TABLE / _FUSE_TABLE."""
    out = []
    for (case, B, H, W) in PRODUCTION:
        layers = flownetc_training_layers(B, H, W) if case == "C" else family_training_layers(case, B, H, W)
        out += [("%s@%dx%dx%d" % (case, B, W, H),) + tuple(layer) for layer in layers]
    return out


def test_deploy_graphs_take_routes_of_classes_the_case_table_runs():
    from flownet2_amd import functional as Fn
    table = {class_of(FWD[n][1], FWD[n][0], FWD[n][7], FWD[n][8]) for n in FWD}
    layers = production_layers()
    assert len(layers) == 252 and {l[0].split("@")[0] for l in layers} == {"C", "S6", "S12", "SD", "fusion"}
    seen = set()
    for (graph, name, kind, n, ci, h, w, co, k, s, p) in layers:
        d = ops.conv_desc(n, ci, h, w, co, k, s, p)
        tr = kind == "deconv"
        route = lib_route(d, tr)
        assert route != NONE, (graph, name)
        served = (Fn.deconv_forward_route(d) if tr else Fn.conv_forward_route(d)) != NONE
        heads = route == (D_HEAD if tr else HEAD)
        # functional.conv_mfma_relu / deconv_relu serve every layer but the 2-channel heads, by name: Convolution* / predict_flow* and
        # upsample_flow* go to functional.predict_flow_conv / upsample_flow_deconv (entry points and autograd functions of their own)
        assert served != heads and heads == name.startswith(("upsample_flow",) if tr else ("Convolution", "predict_flow")), (graph, name)
        cls = class_of(tr, route, k, s)
        assert cls in table, (graph, name, cls)
        seen.add(cls)
    largest = largest_of_each_class()
    assert seen == table == {cls for cls, _ in largest.values()} and sorted(AT_SIZE) == sorted(largest)


def largest_of_each_class():
    """{class name: (class, the production layer of that class with the most multiply-adds)}."""
    best = {}
    for (graph, name, kind, n, ci, h, w, co, k, s, p) in production_layers():
        tr = kind == "deconv"
        cls = class_of(tr, lib_route(ops.conv_desc(n, ci, h, w, co, k, s, p), tr), k, s)
        macs = n * h * w * ci * co * k * k if tr else n * ((h + 2 * p - k) // s + 1) * ((w + 2 * p - k) // s + 1) * ci * co * k * k
        key = "%s-%dx%ds%d" % (cls[4], k, k, s)
        if key not in best or macs > best[key][2]:
            best[key] = (cls, (graph, name, tr, n, ci, h, w, co, k, s, p), macs)
    return {key: v[:2] for key, v in best.items()}


# the classes test_each_class_at_its_largest_production_shape is parametrised with (static, so that collection needs no library); the host
# test above pins the list to what the graphs derive
AT_SIZE = ["conv_mfma-5x5s2", "conv_mfma-3x3s2", "conv_mfma-7x7s2", "conv_mfma-1x1s1", "conv_wino-3x3s1", "conv_plane-3x3s1", "conv_plane-3x3s2",
           "conv_plane_k-5x5s2", "conv_k7s2-7x7s2", "predict_flow-3x3s1", "deconv_gemm-4x4s2", "deconv_plane-4x4s2", "upsample_flow-4x4s2"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: every route through ops.conv_pack_weights / ops.conv_forward


def host(t):
    return t.detach().cpu().numpy()


def run_fwd(name, packed, x_blob, in_c0, bias, relu, slope, out_blob=None, out_c0=0, N=None, route=None):
    """ops.conv_forward on host blobs (copied to the device); returns the whole top blob."""
    tr = FWD[name][1]
    o = None if out_blob is None else dev(out_blob)
    y = ops.conv_forward(dev(x_blob), packed, None if bias is None else dev(bias), desc_of(name, N), FWD[name][0] if route is None else route, tr,
                         relu, slope, out=o, out_c0=out_c0, in_c0=in_c0)
    torch.cuda.synchronize()
    return host(y)


def close_to_twin(name, got, want):
    route, tr = FWD[name][:2]
    bound = TWIN_TOL.get((tr, route))
    if bound is None:
        return same_bits(got, want)
    return got.shape == want.shape and float(np.abs(got - want).max()) <= bound * scale_of(want)


WORST = {}          # route name -> worst error / bound against fp64 (printed: the figures of the commit message)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FWD))
def test_forward_route(name):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    d = desc_of(name)
    assert lib_route(d, tr) == route
    w, x, b = weight_of(name), bottom_of(name), bias_of(name)
    # (a) the packed operand
    packed = ops.conv_pack_weights(dev(w), d, route, tr)
    want_packed = dense_packed(name, w)
    assert same_bits(host(packed), want_packed), "packed operand"
    # (b) the twin's bits (bound), (c) fp64 -- under every flag combination the route accepts, on a fresh top
    fresh = {}
    for relu, has_b, slope in flag_sets(name):
        bb = b if has_b else None
        got = run_fwd(name, packed, x, 0, bb, relu, slope)
        fresh[(relu, has_b, slope)] = got
        want = twin(name, x, want_packed, w, bb, relu, slope)
        assert close_to_twin(name, got, want), ("twin", relu, has_b, slope, float(np.abs(got - want).max()))
        ref = ref64(name, x, w, bb, relu, slope)
        ratio = float(np.abs(got - ref).max()) / (TOL[(tr, route)] * scale_of(ref))
        key = ("deconv " if tr else "conv ") + (ops.DECONV_FWD_ROUTES if tr else ops.CONV_FWD_ROUTES)[route]
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        print("fp64 error / bound: %s %s relu=%d bias=%d slope=%g: %.3f" % (name, key, relu, has_b, slope, ratio))
        assert ratio <= 1.0, ("fp64", relu, has_b, slope, ratio)
    if not (tr and route == D_HEAD):
        # the flags are seen: the ReLU changes the negative half, the bias every value, the slope the negative half again
        assert (fresh[(True, True, 0.1)] != fresh[(False, True, 0.1)]).any() and (fresh[(True, True, 0.1)] != fresh[(True, True, 0.0)]).any()
        assert (fresh[(False, True, 0.1)] < 0).any() and not (fresh[(True, True, 0.0)] < 0).any()
    assert (fresh[flag_sets(name)[0]] != fresh[(flag_sets(name)[0][0], False, 0.1)]).any()
    # (d) the blob forms: top a channel slice at 3 of a sentinel-filled blob, bottom a channel slice at 2 of a wider blob, both
    relu, has_b, slope = flag_sets(name)[0]
    base = fresh[(relu, has_b, slope)]
    wide = rand((N, Cin + 5, H, W), 9)
    wide[:, 2:2 + Cin] = x
    for in_slice, out_slice in slices_of(name):
        blob = np.full((N, Cout + 7, Ht, Wt), SENTINEL) if out_slice else None
        got = run_fwd(name, packed, wide if in_slice else x, 2 if in_slice else 0, b, relu, slope, blob, 3 if out_slice else 0)
        if out_slice:
            assert (got[:, :3] == SENTINEL).all() and (got[:, 3 + Cout:] == SENTINEL).all(), (in_slice, out_slice)
            got = got[:, 3:3 + Cout]
        assert same_bits(got, base), (in_slice, out_slice)


@pytest.mark.gpu
def test_stem_without_relu_is_the_linear_result_and_keeps_special_values():
    """The stem kernel always applies t > 0 ? t : t * slope; for a layer without a fused ReLU the dispatcher hands it slope 1 -- whatever
    negative_slope says.  On small integers (x, bias) and small integer multiples of 1/8 (w) every partial sum is exact in fp32, so the
    kernel, its fp64-accumulating twin and fp64 agree to the bit; among them - 0.0, NaN and the infinities (every weight is nonzero)."""
    for name in ("stem-3", "stem-6"):
        route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
        rng = np.random.default_rng(17)
        w = (rng.integers(1, 8, (Cout, Cin, 7, 7)) * rng.choice([-1, 1], (Cout, Cin, 7, 7)) / 8.0).astype(np.float32)
        b = rng.integers(-4, 5, (Cout,)).astype(np.float32)
        x = rng.integers(-8, 9, (N, Cin, H, W)).astype(np.float32)
        packed = ops.conv_pack_weights(dev(w), desc_of(name), route)
        # finite input: without ReLU the result IS the linear fp64 result (exact), for slope 0.1 and slope 0 alike
        lin = ref64(name, x, w, b, False, 0.0).astype(np.float32)
        assert (lin < 0).any()
        for slope in (0.1, 0.0):
            assert same_bits(run_fwd(name, packed, x, 0, b, False, slope), lin), slope
        assert same_bits(run_fwd(name, packed, x, 0, b, True, 0.1), twin(name, x, packed, w, b, True, 0.1))
        # special values
        x.reshape(-1)[::5] = -0.0
        x[0, 0, 2, 3], x[0, 1, H - 5, 20], x[N - 1, 2, H // 2, 28] = np.nan, np.inf, -np.inf          # no window holds two of them
        for relu, slope in ((False, 0.1), (True, 0.1), (True, 0.0)):
            got = run_fwd(name, packed, x, 0, b, relu, slope)
            want = twin(name, x, packed, w, b, relu, slope)
            nan = np.isnan(want)
            assert nan.any() and np.isinf(want).any() and (~nan & ~np.isinf(want)).any()
            assert np.array_equal(np.isnan(got), nan), (name, relu, slope)
            assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), (name, relu, slope)       # (a NaN's payload is the hardware's)


@pytest.mark.gpu
def test_head_relu_runs_the_second_launch():
    """HEAD = fn2_predict_flow_conv_forward, then (ReLU) fn2_bias_leaky_relu_forward in place: the second launch's bits are those of the
    bias + ReLU twin on the first launch's result."""
    name = "head"
    w, x, b = weight_of(name), bottom_of(name), bias_of(name)
    packed = ops.conv_pack_weights(dev(w), desc_of(name), HEAD)
    plain = run_fwd(name, packed, x, 0, b, False, 0.1)
    assert (plain < 0).any()
    for slope in (0.1, 0.0):
        assert same_bits(run_fwd(name, packed, x, 0, b, True, slope), oracle.bias_leaky_relu_forward(plain, None, slope)), slope


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: refusals -- decided on the host, nothing launched (every blob keeps its sentinel)


def raw_forward(name, route, x, in_ch, in_c0, packed, top, top_ch, top_c0, relu=1, ws=None, ws_bytes=None, null=()):
    """fn2_conv_forward / fn2_deconv_forward past the Python checks.  Every blob is as large as its stated geometry needs, or larger."""
    tr = FWD[name][1]
    d = desc_of(name)
    L = _lib.lib()
    need = int((L.fn2_deconv_workspace_bytes if tr else L.fn2_conv_workspace_bytes)(C.byref(d), FWD[name][0]))
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    ptr = {"bottom": ops._ptr(x), "packed": ops._ptr(packed), "top": ops._ptr(top)}
    for n in null:
        ptr[n] = None
    try:
        check((L.fn2_deconv_forward if tr else L.fn2_conv_forward)(
            C.byref(d), int(route), ptr["bottom"], in_ch, in_c0, ptr["packed"], None, ptr["top"], top_ch, top_c0, relu, C.c_float(0.1),
            None if ws is False else ops._ptr(ws), need if ws_bytes is None else ws_bytes, ops._stream()))
    finally:
        torch.cuda.synchronize()


def refusal_blobs(name):
    """Bottom, operand and a sentinel-filled top with 8 channels of room on either side of what the layer reads and writes."""
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    x = dev(rand((N, Cin + 8, H, W), 4))
    top = torch.full((N, Cout + 8, Ht, Wt), float(SENTINEL), device="cuda")
    packed = ops.conv_pack_weights(dev(weight_of(name)), desc_of(name), route, tr)
    return x, packed, top


def family_takes(name, r):
    """Does the kernel family route r names take this layer's geometry (whether or not the library would choose it)?"""
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    if tr:
        return {D_GEMM: (16 * Cout) % 32 == 0 and (H * W) % 4 == 0 and ops.conv_mfma_supported(Cin, H, W, 16 * Cout, 1, 1, 0),
                D_PLANE: ops.deconv_plane_supported(N, Cin, H, W, Cout), D_HEAD: Cin == 2 and Cout == 2}[r]
    return {DIRECT: ops.conv_mfma_supported(Cin, H, W, Cout, k, s, p), WINOGRAD: k == 3 and s == 1 and ops.conv_wino_supported(Cin, H, W, Cout, p),
            PLANE: (k == 3 and ops.conv_plane_supported(N, Cin, H, W, Cout, s, p)) or ((k, s, p) == (5, 2, 2) and ops.conv_plane_k_supported(N, Cin, H, W, Cout, 5, 2, 2)),
            STEM: (k, s, p) == (7, 2, 3) and ops.conv_k7s2_relu_supported(Cin, H, W, Cout), HEAD: (k, s, p) == (3, 1, 1) and Cout == 2}[r]


def untouched(top):
    return bool((top == float(SENTINEL)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FWD))
def test_dispatchers_refuse_on_the_host(name):
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    x, packed, top = refusal_blobs(name)
    whole = (not tr and route in (STEM, HEAD))
    relu = 0 if (tr and route == D_HEAD) else 1
    # the stated geometry is inside the allocations in every call below; the dispatcher must refuse on what it is TOLD
    calls = {
        "route NONE": dict(route=0),
        "null bottom": dict(null=("bottom",)), "null operand": dict(null=("packed",)), "null top": dict(null=("top",)),
        "bottom slice past its blob": dict(in_ch=Cin + 1, in_c0=2), "top slice past its blob": dict(top_ch=Cout + 2, top_c0=3),
        "negative bottom slice": dict(in_ch=Cin + 8, in_c0=-1), "negative top slice": dict(top_ch=Cout + 8, top_c0=-1),
    }
    for r in ((D_GEMM, D_PLANE, D_HEAD) if tr else (DIRECT, WINOGRAD, PLANE, STEM, HEAD)):
        if r != route and not family_takes(name, r):          # a route that is not the layer's: the family it names has no kernel for this geometry
            calls["route %d" % r] = dict(route=r)
    assert sum(1 for what in calls if what.startswith("route ")) >= 3
    if whole:
        calls.update({"bottom slice": dict(in_ch=Cin + 8, in_c0=2), "top slice": dict(top_ch=Cout + 8, top_c0=3)})
    if tr and route == D_HEAD:
        calls.update({"ReLU": dict(relu=1), "bottom slice": dict(in_ch=Cin + 8, in_c0=2)})
    L = _lib.lib()
    need = int((L.fn2_deconv_workspace_bytes if tr else L.fn2_conv_workspace_bytes)(C.byref(desc_of(name)), route))
    if (tr and route in (D_GEMM, D_PLANE)) or (not tr and route in (PLANE, HEAD)):
        assert need > 0, name
        calls.update({"short workspace": dict(ws_bytes=need - 4), "null workspace": dict(ws=False)})
    for what, kw in calls.items():
        args = dict(route=route, in_ch=Cin, in_c0=0, top_ch=Cout, top_c0=0, relu=relu)
        args.update(kw)
        with pytest.raises(Fn2Error):
            raw_forward(name, args["route"], x, args["in_ch"], args["in_c0"], packed, top, args["top_ch"], args["top_c0"], args["relu"],
                        ws=kw.get("ws"), ws_bytes=kw.get("ws_bytes"), null=kw.get("null", ()))
            pytest.fail("%s: %s was not refused" % (name, what))
        assert untouched(top), (name, what)
    # an operand of the wrong length: ops.conv_forward's own check
    with pytest.raises(ValueError):
        ops.conv_forward(x[:, :Cin].contiguous(), packed[:-4], None, desc_of(name), route, tr, bool(relu), 0.1)
    with pytest.raises(ValueError):
        ops.conv_forward(x[:, :Cin].contiguous(), torch.cat([packed, packed[:4]]), None, desc_of(name), route, tr, bool(relu), 0.1)
    with pytest.raises(ValueError):
        ops.conv_pack_weights(dev(weight_of(name)), desc_of(name), 0, tr)
    # ... and the call none of this applies to writes exactly the layer's channels
    if not whole:
        raw_forward(name, route, x, Cin + 8, 0, packed, top, Cout + 8, 0, relu) if not (tr and route == D_HEAD) else \
            raw_forward(name, route, x[:, :2].contiguous(), 2, 0, packed, top, Cout + 8, 0, relu)
        assert not bool((top[:, :Cout] == float(SENTINEL)).any()) and untouched(top[:, Cout:])


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: batch-invariant mode

INVARIANT = ["direct-5x5", "direct-1x1", "wino-threshold", "plane-3x3s1", "plane-3x3s2", "plane-5x5", "stem-3", "head", "deconv-gemm",
             "deconv-plane", "deconv-head"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", INVARIANT)
def test_batch_invariant_sample_has_the_bits_of_that_sample_alone(name):
    tr = FWD[name][1]
    w, b, x = weight_of(name), bias_of(name), bottom_of(name, N=3)
    relu = not (tr and FWD[name][0] == D_HEAD)
    was = invariant(True)
    try:
        r3, r1 = lib_route(desc_of(name, N=3), tr), lib_route(desc_of(name, N=1), tr)
        assert r3 == r1 == FWD[name][0]
        p3 = ops.conv_pack_weights(dev(w), desc_of(name, N=3), r3, tr)
        p1 = ops.conv_pack_weights(dev(w), desc_of(name, N=1), r1, tr)
        assert torch.equal(p3, p1)
        batch = run_fwd(name, p3, x, 0, b, relu, 0.1, N=3, route=r3)
        alone = run_fwd(name, p1, x[:1], 0, b, relu, 0.1, N=1, route=r1)
        assert same_bits(batch[:1], alone)
        ref = ref64(name, x, w, b, relu, 0.1)
        assert np.abs(batch - ref).max() <= TOL[(tr, r3)] * scale_of(ref)
    finally:
        ops.set_batch_invariant(was)
    assert ops.get_batch_invariant() == was


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the Python layer (functional.conv_mfma_relu / deconv_relu)

PYTHON = ["direct-5x5", "direct-3x3s2", "direct-7x7", "direct-1x1", "wino-threshold", "plane-3x3s1", "plane-3x3s2", "plane-5x5", "deconv-gemm",
          "deconv-plane"]


def fn_forward(name, x, w, b, out=None, out_c0=0):
    from flownet2_amd import functional as Fn
    route, tr, N, Cin, H, W, Cout, k, s, p = FWD[name]
    if tr:
        return Fn.deconv_relu(x, w, b, 0.1, True, out=out, out_c0=out_c0)
    return Fn.conv_mfma_relu(x, w, b, s, p, 0.1, True, out=out, out_c0=out_c0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PYTHON + ["stem-3"])
def test_python_layer_has_the_bits_of_the_descriptor_call(name, monkeypatch):
    from flownet2_amd import functional as Fn
    monkeypatch.setenv("FN2_STRICT", "1")
    route, tr, N, Cin, H, W, Cout, k, s, p, Ht, Wt = geom(name)
    d = desc_of(name)
    assert (Fn.deconv_forward_route(d) if tr else Fn.conv_forward_route(d)) == route
    w, b = dev(weight_of(name)), dev(bias_of(name))
    wide = dev(rand((N, Cin + 5, H, W), 9))
    x = wide[:, 2:2 + Cin]                       # a non-contiguous channel-slice view: read in place
    assert N == 1 or not x.is_contiguous()        # (one sample: the slice IS contiguous, and read as a blob of its own)
    want = ops.conv_forward(x.contiguous(), ops.conv_pack_weights(w, d, route, tr), b, d, route, tr, True, 0.1)
    before = Fn.LIBRARY_FALLBACKS[0]
    assert torch.equal(fn_forward(name, x, w, b), want)
    if route != STEM:                            # (the stem writes whole blobs: conv_mfma_relu declines out=)
        blob = torch.full((N, Cout + 7, Ht, Wt), float(SENTINEL), device="cuda")
        y = fn_forward(name, x, w, b, out=blob, out_c0=3)
        assert torch.equal(blob[:, 3:3 + Cout], want) and untouched(blob[:, :3]) and untouched(blob[:, 3 + Cout:])
        assert y.data_ptr() == blob.data_ptr() or torch.equal(y, want)
    else:
        assert fn_forward(name, x, w, b, out=torch.empty((N, Cout, Ht, Wt), device="cuda")) is None
    # under autograd: _OwnForwardConv runs the same forward
    xg, wg, bg = x.detach().clone().requires_grad_(True), torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
    y = fn_forward(name, xg, wg, bg)
    assert y.requires_grad and y.grad_fn is not None and torch.equal(y.detach(), want)
    if route != STEM:
        blob = torch.full((N, Cout + 7, Ht, Wt), float(SENTINEL), device="cuda")
        y = fn_forward(name, wide.detach().clone().requires_grad_(True)[:, 2:2 + Cin], wg, bg, out=blob, out_c0=3)
        assert y.requires_grad and torch.equal(y.detach(), want) and torch.equal(blob[:, 3:3 + Cout], want) and untouched(blob[:, :3])
    assert Fn.LIBRARY_FALLBACKS[0] == before


def counted_packs(monkeypatch):
    packs, pack = [], ops.conv_pack_weights
    monkeypatch.setattr(ops, "conv_pack_weights", lambda w, desc, route, *a, **k: packs.append((w.clone(), int(route))) or pack(w, desc, route, *a, **k))
    return packs


def lib_act(x, w, b, s, p):
    return torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p), 0.1)


def assert_fp64(y, ref, bound):
    assert float((y.double() - ref).abs().max()) <= bound * max(1.0, float(ref.abs().max()))


@pytest.mark.gpu
def test_forward_operand_cache_is_per_weight_and_route(monkeypatch):
    """functional._PACKED_T: one pack per (weight, route) -- reused at another map size of the same route, a second pack where the same weight
    takes another route (WINOGRAD on a large map, PLANE on a small one), rebuilt after an in-place write and after a fused optimizer step."""
    from flownet2_amd import functional as Fn
    packs = counted_packs(monkeypatch)
    w = torch.nn.Parameter(dev(rand((64, 24, 3, 3), 40, 0.1)))
    b = dev(rand((64,), 41, 0.1))
    sizes = {"wino-a": (3, 24, 65, 76), "wino-b": (1, 24, 95, 100), "plane": (2, 24, 6, 8)}
    xs = {k: dev(rand(v, 42)) for k, v in sizes.items()}
    routes = {k: Fn.conv_forward_route(ops.conv_desc(*v, 64, 3, 1, 1)) for k, v in sizes.items()}
    assert routes == {"wino-a": WINOGRAD, "wino-b": WINOGRAD, "plane": PLANE}
    bound = {WINOGRAD: TOL[(False, WINOGRAD)], PLANE: TOL[(False, PLANE)]}

    def forward_all(expect_packs):
        with torch.no_grad():
            for k in ("wino-a", "wino-b", "plane", "wino-a", "plane"):
                y = Fn.conv_mfma_relu(xs[k], w, b, 1, 1, 0.1, True)
                assert_fp64(y, lib_act(xs[k], w.detach(), b, 1, 1), bound[routes[k]])
        assert [r for _, r in packs] == expect_packs

    forward_all([WINOGRAD, PLANE])                           # one pack per route; the second Winograd size reuses the first's
    forward_all([WINOGRAD, PLANE])                           # nothing repacked
    with torch.no_grad():
        w.mul_(2.0)
    forward_all([WINOGRAD, PLANE] * 2)                       # rebuilt from the written tensor, both routes
    assert torch.equal(packs[2][0], w.detach()) and torch.equal(packs[3][0], w.detach())
    w.grad = torch.ones_like(w)
    torch.optim.Adam([w], lr=0.05, fused=True).step()        # writes w without touching _version
    forward_all([WINOGRAD, PLANE] * 3)
    assert torch.equal(packs[4][0], w.detach()) and not torch.equal(packs[4][0], packs[2][0])
    # the key carries the route: the two operands live side by side
    keys = [key for key in Fn._PACKED_T if key[0] == id(w) and key[1][0] == "fwd"]
    assert sorted(key[1][1] for key in keys) == sorted([WINOGRAD, PLANE])


@pytest.mark.gpu
def test_stem_route_caches_nothing(monkeypatch):
    from flownet2_amd import functional as Fn
    packs = counted_packs(monkeypatch)
    name = "stem-3"
    w, b, x = dev(weight_of(name)), dev(bias_of(name)), dev(bottom_of(name))
    y = Fn.conv_mfma_relu(x, w, b, 2, 3, 0.1, True)
    assert_fp64(y, lib_act(x, w, b, 2, 3), TOL[(False, STEM)])
    assert packs == [] and not [key for key in Fn._PACKED_T if key[0] == id(w)]
    w.mul_(2.0)
    assert_fp64(Fn.conv_mfma_relu(x, w, b, 2, 3, 0.1, True), lib_act(x, w, b, 2, 3), TOL[(False, STEM)])
    assert packs == []


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the largest production layer of each class, by descriptor


@pytest.mark.gpu
@pytest.mark.parametrize("key", AT_SIZE)
def test_each_class_at_its_largest_production_shape(key):
    """Against MIOpen fp32 everywhere and fp64 on sample 0, at the bounds of test_conv_mfma.py::test_conv_mfma_at_flownet_shapes."""
    F = torch.nn.functional
    cls, (graph, lname, tr, N, Cin, H, W, Cout, k, s, p) = largest_of_each_class()[key]
    d = ops.conv_desc(N, Cin, H, W, Cout, k, s, p)
    route = lib_route(d, tr)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, Cin, H, W, device="cuda", generator=g)
    w = torch.randn((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), device="cuda", generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    b = torch.randn(Cout, device="cuda", generator=g) * 0.1
    relu = not (tr and route == D_HEAD)
    got = ops.conv_forward(x, ops.conv_pack_weights(w, d, route, tr), b, d, route, tr, relu, 0.1)
    conv = (lambda xx, ww, bb: F.conv_transpose2d(xx, ww, bb, stride=2, padding=1)) if tr else (lambda xx, ww, bb: F.conv2d(xx, ww, bb, stride=s, padding=p))
    act = (lambda t: F.leaky_relu(t, 0.1)) if relu else (lambda t: t)
    lib = act(conv(x, w, b))
    scale = max(1.0, float(lib.abs().max()))
    e_lib = float((got - lib).abs().max())
    e_64 = float((got[:1].double() - act(conv(x[:1].double(), w.double(), b.double()))).abs().max())
    print("%s %s %s: vs MIOpen %.2e, vs fp64 %.2e (x scale %.2f)" % (key, graph, lname, e_lib / scale, e_64 / scale, scale))
    assert e_lib <= LIB_TOL * scale and e_64 <= FP64_TOL * scale
