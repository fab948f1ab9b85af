// Convolution / Deconvolution behind ONE geometry descriptor: the library picks its own kernel.
//
// The reference has one ConvolutionLayer / DeconvolutionLayer for every geometry (im2col + GEMM per sample: conv_layer.cu:8-23,
// deconv_layer.cu:8-26, base_conv_layer.cpp:255-396); this library has a kernel family per geometry class (direct 5x5/2 .. 7x7/2 and 1x1,
// Winograd F(2x2,3x3), the small-map kernel with its deterministic K split, the Deconvolution as GEMM + col2im or as parity classes).
// Which one serves a layer is decided HERE, from the descriptor alone -- the Python mirror (flownet2_amd/functional.py: conv_mfma_relu,
// deconv_relu, conv_backward) and the Caffe adapter (csrc/caffe_adapter) make the same call sequence, forward and backward: route -> pack
// (once per weight version) -> workspace -> one dispatch call.  Python holds no routing rule and no per-family dispatch of its own, so a
// Caffe user of libflownet2_hip.so gets the routing, the operands and the kernels the tests and the benchmarks ran with.
//
// DECISIONS are code: fn2_conv_route, fn2_deconv_route, bwd_geom, fn2_conv_backward_data_route_flags.  Their thresholds are measurements
// (profiles/r02_conv_bench_*.txt, r04_conv_plane_bench_flownetc.txt, scripts/probes/small_layer_routes.py; the split-bf16 flags:
// profiles/deconv_bf16x3_bench.md, dgrad_bf16x3_bench.md, wino_bf16x3_bench.md) and their order matters.  FN2_ROUTE_BF16X3 asks for the
// split-bf16 arithmetic where a kernel of it takes the layer, as a bit (FN2_CONV_ARITH_BF16X3) beside the route; FN2_ROUTE_WINO_BF16X3 is a
// flag of its own for the Winograd layers; without a flag every answer is the exact fp32 one.
// FAMILIES are data: three tables, one row per route value (arithmetic bit included), a family's facts stated once in its row --
//     kConvRows    7  DIRECT, DIRECT | BF16X3, WINOGRAD, WINOGRAD | BF16X3, PLANE, STEM, HEAD
//     kDeconvRows  4  GEMM, GEMM | BF16X3, PLANE, HEAD
//     kBwdRows     6  WINOGRAD, TCONV, TCONV | BF16X3, PLANE, DIRECT, DECONV_PLANE            (the data gradient)
// Every by-route entry point is a lookup (find / bwd_plan), the checks all families share, and one call through the row.  The weight
// gradient has two arithmetics and no route: one body (wgrad_workspace / wgrad_run) behind the plain and the _arith entry points.
// ADDING A ROUTE: one row in its table (what it takes, its operand, its scratch, its launch) and the line of the decision function that
// returns it.  Nothing else names a family.
// What the entry points do that one would not guess, kept as it was (tests/test_conv_route_table.py pins all of it):
//   - the forward size queries and pack calls answer for a BASE route whether or not its family takes the layer (Winograd floats for a
//     5x5 layer, the flow head's scratch for any layer); a route with the arithmetic bit answers only where its kernel takes the layer.
//     fn2_*_forward refuses both alike.  The data-gradient queries answer 0 for every route but the layer's own.
//   - fn2_*_forward checks: route not the layer's, NULL blob, slice outside its blob, whole-blob family given a slice, then the family's
//     own (workspace, alignment).  fn2_conv_backward_data and its pack call look at NULL blobs BEFORE the route.
//   - the Deconvolution's flow head reads a whole bottom blob but writes a slice of top, and refuses a fused ReLU; the Convolution's stem
//     gets slope 1 for a layer without ReLU; the Convolution's flow head runs bias + ReLU as a second launch.
#include "conv_internal.hpp"
#include "fn2_common.hpp"

namespace {

struct Out { int H, W; };
inline Out conv_out(const fn2_conv_desc* d) {
  return {(d->Hin + 2 * d->pad - d->kernel) / d->stride + 1, (d->Win + 2 * d->pad - d->kernel) / d->stride + 1};
}

bool valid(const fn2_conv_desc* d) {
  return d && d->N >= 1 && d->Cin >= 1 && d->Cout >= 1 && d->Hin >= 1 && d->Win >= 1 && d->kernel >= 1 && d->stride >= 1 && d->pad >= 0 &&
         d->Hin + 2 * d->pad >= d->kernel && d->Win + 2 * d->pad >= d->kernel;
}

// the layers of the GEMM route: weight^T x bottom on the 1x1 form of the direct kernel
bool deconv_gemm_ok(const fn2_conv_desc* d) {
  return (d->Cout * 16) % 32 == 0 && (d->Hin * d->Win) % 4 == 0 && fn2_conv_mfma_supported(d->Cin, d->Hin, d->Win, d->Cout * 16, 1, 1, 0) != 0;
}
inline bool deconv_421(const fn2_conv_desc* d) { return d->kernel == 4 && d->stride == 2 && d->pad == 1; }

// ---- the forward families ----
using Desc = const fn2_conv_desc*;
struct FwdCall {
  const float* bottom; int bottom_channels, bottom_c0; const float* packed; const float* bias; float* top; int top_channels, top_c0;
  int relu; float slope; void* workspace; size_t workspace_bytes; void* stream;
};
struct FwdRow {
  int route;                                                               // the value callers pass, arithmetic bit included
  bool (*takes)(Desc);                                                     // does the family's kernel take this geometry?
  size_t (*packed_floats)(Desc);
  int (*pack)(Desc, const float* weight, float* packed, void* stream);     // NULL: the kernel reads the blob as it is
  size_t (*workspace_bytes)(Desc);                                         // NULL: none
  const char* whole;                                                       // the kernel's name where it reads whole blobs only, else NULL
  int (*run)(Desc, const FwdCall&);
};
// a row's entries are captureless lambdas over the descriptor d (pack: weight, packed, stream; run: the call c); their heads, spelled once
#define TAKES(...) [](Desc d) -> bool { return __VA_ARGS__; }
#define SIZE(...) [](Desc d) -> size_t { return __VA_ARGS__; }
#define PACK(...) [](Desc d, const float* weight, float* packed, void* stream) -> int { return __VA_ARGS__; }
#define RUN(...) [](Desc d, const FwdCall& c) -> int { return __VA_ARGS__; }
// ... and what every forward kernel takes first: the four blobs, the bottom's geometry and slice, the top's slice
#define BLOBS c.bottom, c.packed, c.bias, c.top, d->N, d->Cin, d->Hin, d->Win, c.bottom_channels, c.bottom_c0, d->Cout, c.top_channels, c.top_c0
#define GEOM d->N, d->Cin, d->Hin, d->Win, d->Cout

size_t blob_floats(Desc d) { return (size_t)d->Cout * d->Cin * d->kernel * d->kernel; }
size_t mfma_floats(Desc d) { return fn2_conv_mfma_packed_floats(d->Cout, d->Cin, d->kernel); }
int mfma_pack(Desc d, const float* weight, float* packed, void* stream) { return fn2_conv_mfma_pack_weights(weight, packed, d->Cout, d->Cin, d->kernel, stream); }
int head_run(Desc d, const FwdCall& c) {       // predict_flow*: bias + ReLU is a second launch, in place
  const int rc = fn2_predict_flow_conv_forward(c.bottom, c.packed, c.bias, c.top, d->N, d->Cin, d->Hin, d->Win, c.workspace, c.workspace_bytes, c.stream);
  return (rc != FN2_OK || !c.relu) ? rc : fn2_bias_leaky_relu_forward(c.top, nullptr, d->N, d->Cout, d->Hin, d->Win, c.slope, c.stream);
}

const FwdRow kConvRows[] = {
    {FN2_CONV_ROUTE_DIRECT, TAKES(fn2_conv_mfma_supported(d->Cin, d->Hin, d->Win, d->Cout, d->kernel, d->stride, d->pad) != 0), mfma_floats, mfma_pack, nullptr,
     nullptr, RUN(fn2_conv_mfma_forward(BLOBS, d->kernel, d->stride, d->pad, c.relu, c.slope, c.stream))},
    {FN2_CONV_ROUTE_DIRECT | FN2_CONV_ARITH_BF16X3, TAKES(fn2_conv_bf16x3_supported(d) != 0),                 // csrc/conv_bf16x3.hip
     SIZE(fn2::conv_bf16x3_packed_floats(d->Cout, d->Cin, d->kernel)), PACK(fn2::conv_bf16x3_pack_weights(weight, packed, d->Cout, d->Cin, d->kernel, stream)),
     nullptr, nullptr, RUN(fn2::conv_bf16x3_forward(BLOBS, d->kernel, d->stride, d->pad, c.relu, c.slope, c.stream))},
    // (Winograd and the flow head take no kernel / stride argument: `takes` is all that keeps another geometry out of them)
    {FN2_CONV_ROUTE_WINOGRAD, TAKES(d->kernel == 3 && d->stride == 1 && fn2_conv_wino_supported(d->Cin, d->Hin, d->Win, d->Cout, d->pad) != 0),
     SIZE(fn2_conv_wino_packed_floats(d->Cout, d->Cin)), PACK(fn2_conv_wino_pack_weights(weight, packed, d->Cout, d->Cin, stream)), nullptr, nullptr,
     RUN(fn2_conv_wino_forward(BLOBS, d->pad, c.relu, c.slope, c.stream))},
    {FN2_CONV_ROUTE_WINOGRAD | FN2_CONV_ARITH_BF16X3, TAKES(fn2_conv_wino_bf16x3_supported(d) != 0),          // csrc/conv_wino_bf16x3.hip
     SIZE(fn2::conv_wino_bf16x3_packed_floats(d->Cout, d->Cin)), PACK(fn2::conv_wino_bf16x3_pack_weights(weight, packed, d->Cout, d->Cin, stream)), nullptr,
     nullptr, RUN(fn2::conv_wino_bf16x3_forward(BLOBS, d->kernel, d->stride, d->pad, c.relu, c.slope, c.stream))},
    {FN2_CONV_ROUTE_PLANE,                                                                                    // two entry points: 3x3 / 1 or 2, and 5x5 / 2 / 2
     TAKES(d->kernel == 3 ? fn2_conv_plane_supported(GEOM, d->stride, d->pad) != 0
                          : (d->kernel == 5 && d->stride == 2 && d->pad == 2 && fn2_conv_plane_k_supported(GEOM, 5, 2, 2) != 0)),
     mfma_floats, mfma_pack,
     SIZE(d->kernel == 3 ? fn2_conv_plane_workspace_bytes(GEOM, d->stride, d->pad) : fn2_conv_plane_k_workspace_bytes(GEOM, d->kernel, d->stride, d->pad)), nullptr,
     RUN(d->kernel == 3 ? fn2_conv_plane_forward(BLOBS, d->stride, d->pad, c.relu, c.slope, c.workspace, c.workspace_bytes, c.stream)
                        : fn2_conv_plane_k_forward(BLOBS, d->kernel, d->stride, d->pad, c.relu, c.slope, c.workspace, c.workspace_bytes, c.stream))},
    // the stem kernel always applies t > 0 ? t : t * slope: slope 1 is the identity (exactly: t * 1.0f == t) for a layer without a fused ReLU
    {FN2_CONV_ROUTE_STEM, TAKES(d->kernel == 7 && d->stride == 2 && d->pad == 3 && fn2_conv_k7s2_relu_supported(d->Cin, d->Hin, d->Win, d->Cout) != 0), blob_floats,
     nullptr, nullptr, "stem", RUN(fn2_conv_k7s2_relu_forward(c.bottom, c.packed, c.bias, c.top, GEOM, c.relu ? c.slope : 1.0f, c.stream))},
    {FN2_CONV_ROUTE_HEAD, TAKES(d->kernel == 3 && d->stride == 1 && d->pad == 1 && d->Cout == 2), blob_floats, nullptr,
     SIZE(fn2_predict_flow_conv_workspace_bytes(d->N, d->Cin, d->Hin, d->Win)), "flow-head", head_run},
};

// Deconvolution{4, 2, 1}: Cin = bottom channels, Cout = top channels, top is [N, Cout, 2 Hin, 2 Win]; weight blob [Cin][Cout][4][4].
// GEMM and GEMM | BF16X3 are one route in two arithmetics: the same column matrix [N][16 Cout][Hin Win] in the workspace and the same
// col2im + bias + ReLU second pass (deconv_gemm_col2im); only the GEMM that fills the column matrix differs.
size_t deconv_col_bytes(Desc d) { return sizeof(float) * (size_t)d->N * d->Cout * 16 * d->Hin * d->Win; }
int deconv_gemm_col2im(Desc d, const FwdCall& c, int (*gemm)(Desc, const FwdCall&, float* col)) {
  const size_t need = deconv_col_bytes(d);
  if (!c.workspace || c.workspace_bytes < need) return fn2::fail(FN2_ERR_INVALID_ARG, "deconv_forward: workspace of %zu bytes needed for the column matrix", need);
  float* col = static_cast<float*>(c.workspace);
  if (const int rc = gemm(d, c, col)) return rc;
  return fn2_col2im_bias_relu_forward_into(col, c.bias, c.top, d->N, d->Cout, 2 * d->Hin, 2 * d->Win, 4, 1, 2, c.relu, c.slope, c.top_channels, c.top_c0, c.stream);
}
#define GEMM(...) RUN(deconv_gemm_col2im(d, c, [](Desc d, const FwdCall& c, float* col) -> int { return __VA_ARGS__; }))

const FwdRow kDeconvRows[] = {
    // GEMM operand [M = Cout 16][Cin] straight from the [Cin][Cout][4][4] blob through the strided view (base_conv_layer.cpp:375-384's weight^T)
    {FN2_DECONV_ROUTE_GEMM, TAKES(deconv_421(d) && deconv_gemm_ok(d)), SIZE(fn2_conv_mfma_packed_floats(d->Cout * 16, d->Cin, 1)),
     PACK(fn2_conv_mfma_pack_weights_view(weight, packed, d->Cout * 16, d->Cin, 1, d->Cout * 16, d->Cin, 1, d->Cout * 16, 0, stream)), deconv_col_bytes, nullptr,
     GEMM(fn2_conv_mfma_forward(c.bottom, c.packed, nullptr, col, d->N, d->Cin, d->Hin, d->Win, c.bottom_channels, c.bottom_c0, d->Cout * 16, d->Cout * 16, 0, 1, 1, 0,
                                0, 0.f, c.stream))},
    {FN2_DECONV_ROUTE_GEMM | FN2_CONV_ARITH_BF16X3, TAKES(deconv_421(d) && deconv_gemm_ok(d) && fn2_deconv_bf16x3_supported(d) != 0),      // csrc/deconv_bf16x3.hip
     SIZE(fn2::deconv_bf16x3_packed_floats(d->Cin, d->Cout)), PACK(fn2::deconv_bf16x3_pack_weights(weight, packed, d->Cin, d->Cout, stream)), deconv_col_bytes, nullptr,
     GEMM(fn2::deconv_bf16x3_gemm(c.bottom, c.packed, col, d->N, d->Cin, d->Hin, d->Win, c.bottom_channels, c.bottom_c0, d->Cout, c.stream))},
    {FN2_DECONV_ROUTE_PLANE, TAKES(deconv_421(d) && fn2_deconv_plane_supported(GEOM) != 0), SIZE(fn2_deconv_plane_packed_floats(d->Cin, d->Cout)),
     PACK(fn2_deconv_plane_pack_weights(weight, packed, d->Cin, d->Cout, stream)), SIZE(fn2_deconv_plane_workspace_bytes(GEOM)), nullptr,
     RUN(fn2_deconv_plane_forward(BLOBS, c.relu, c.slope, c.workspace, c.workspace_bytes, c.stream))},
    // upsample_flow*: the 2-channel kernel (csrc/flow_head.hip) reads a whole blob, writes a slice of top, and has no fused ReLU
    {FN2_DECONV_ROUTE_HEAD, TAKES(deconv_421(d) && d->Cin == 2 && d->Cout == 2), SIZE((size_t)d->Cin * d->Cout * 16), nullptr, nullptr, "flow-head",
     RUN(c.relu ? fn2::fail(FN2_ERR_UNSUPPORTED, "deconv_forward: the 2-channel flow-head kernel has no fused ReLU (the FlowNet graphs have none there)")
                : fn2_upsample_flow_deconv_forward_into(c.bottom, c.packed, c.bias, c.top, d->N, d->Hin, d->Win, c.top_channels, c.top_c0, c.stream))},
};
#undef TAKES
#undef SIZE
#undef PACK
#undef RUN
#undef GEMM
#undef BLOBS
#undef GEOM

// name: how the error texts begin; whole_top: a whole-blob family writes a whole top blob too (the Deconvolution's flow head writes a slice)
struct FwdTable { const char* name; const char* layer; const FwdRow* rows; int n; bool whole_top; };
const FwdTable kConv = {"conv", "Convolution", kConvRows, (int)(sizeof(kConvRows) / sizeof(kConvRows[0])), true};
const FwdTable kDeconv = {"deconv", "Deconvolution", kDeconvRows, (int)(sizeof(kDeconvRows) / sizeof(kDeconvRows[0])), false};

// The row `route` names, where its family takes the layer.  Not "is it the route fn2_conv_route returns": that depends on the flags and on
// batch-invariant mode, and a caller may pack for one answer and run after the mode changed.  `sized`: for the operand and scratch queries
// and the pack calls, which answer for a base route whatever the layer (kept: callers read these numbers); the arithmetic bit on a layer
// its kernel does not take names no kernel there either.
const FwdRow* find(const FwdTable& t, Desc d, int route, bool sized = false) {
  for (int i = 0; i < t.n; ++i)
    if (t.rows[i].route == route) return ((sized && !(route & FN2_CONV_ARITH_BF16X3)) || t.rows[i].takes(d)) ? &t.rows[i] : nullptr;
  return nullptr;
}

size_t fwd_packed_floats(const FwdTable& t, Desc d, int route) {
  const FwdRow* r = valid(d) ? find(t, d, route, true) : nullptr;
  return r ? r->packed_floats(d) : 0;
}
size_t fwd_workspace_bytes(const FwdTable& t, Desc d, int route) {
  const FwdRow* r = valid(d) ? find(t, d, route, true) : nullptr;
  return r && r->workspace_bytes ? r->workspace_bytes(d) : 0;
}
int fwd_pack_weights(const FwdTable& t, Desc d, int route, const float* weight, float* packed, void* stream) {
  if (!valid(d) || !weight || !packed) return fn2::fail(FN2_ERR_INVALID_ARG, "%s_pack_weights: bad descriptor or NULL blob", t.name);
  const FwdRow* r = find(t, d, route, true);
  if (!r) return fn2::fail(FN2_ERR_UNSUPPORTED, "%s_pack_weights: no own kernel for this layer (route %d)", t.name, route);
  if (r->pack) return r->pack(d, weight, packed, stream);
  // the kernel reads the blob as it is: the operand is a copy of it (or the blob itself)
  if (weight != packed && hipMemcpyAsync(packed, weight, sizeof(float) * r->packed_floats(d), hipMemcpyDeviceToDevice, fn2::as_stream(stream)) != hipSuccess)
    return fn2::fail(FN2_ERR_LAUNCH, "%s_pack_weights: device copy of the weight blob failed", t.name);
  return FN2_OK;
}

int fwd_forward(const FwdTable& t, Desc d, int route, const FwdCall& c) {
  if (!valid(d)) return fn2::fail(FN2_ERR_INVALID_ARG, "%s_forward: bad descriptor", t.name);
  const FwdRow* r = find(t, d, route);
  if (!r)
    return fn2::fail(FN2_ERR_UNSUPPORTED, "%s_forward: no own kernel for %s{kernel %d, stride %d, pad %d} %d -> %d on %d x %d (route %d)", t.name, t.layer,
                     d->kernel, d->stride, d->pad, d->Cin, d->Cout, d->Hin, d->Win, route);
  if (!c.bottom || !c.packed || !c.top) return fn2::fail(FN2_ERR_INVALID_ARG, "%s_forward: NULL blob", t.name);
  if (c.bottom_c0 < 0 || c.bottom_c0 + d->Cin > c.bottom_channels || c.top_c0 < 0 || c.top_c0 + d->Cout > c.top_channels)
    return fn2::fail(FN2_ERR_INVALID_ARG, "%s_forward: channel slice outside its blob", t.name);
  if (r->whole && (c.bottom_channels != d->Cin || c.bottom_c0 != 0 || (t.whole_top && (c.top_channels != d->Cout || c.top_c0 != 0))))
    return t.whole_top ? fn2::fail(FN2_ERR_UNSUPPORTED, "%s_forward: the %s kernel reads and writes whole blobs, not channel slices", t.name, r->whole)
                       : fn2::fail(FN2_ERR_UNSUPPORTED, "%s_forward: the %s kernel reads a whole %d-channel blob", t.name, r->whole, d->Cin);
  return r->run(d, c);
}

}  // namespace

FN2_API int fn2_conv_route(const fn2_conv_desc* d, int flags) {
  if (!valid(d)) return FN2_CONV_ROUTE_NONE;
  const bool force = (flags & FN2_ROUTE_FORCE) != 0;
  const int k = d->kernel, s = d->stride, p = d->pad, Cin = d->Cin, Cout = d->Cout, H = d->Hin, W = d->Win;
  // batch-invariant mode (fn2_set_batch_invariant): the route -- and with it the arithmetic -- must not depend on the batch: decide as for
  // one sample, and require the small-map kernel's plan for one sample AND for the real batch
  const bool inv = fn2_get_batch_invariant() != 0;
  const int N = inv ? 1 : d->N;
  const bool wino_first = force || inv;
  const Out o = conv_out(d);
  // the two geometry classes with kernels of their own (round 6: reachable by descriptor, so that the Caffe adapter's Convolution plug-in
  // serves EVERY layer of the FlowNet graphs): the 7x7 / 2 stem on 3 / 6 / 12 input channels, and the 2-channel predict_flow heads
  // (the 12-channel stems of FlowNet2's stacked nets are whole channel quads: the direct kernel does them in one pass -- 174 us against 277 for
  // the register-resident stem kernel's two passes at batch 4 @768x384 -- so the stem route is for the channel counts the direct kernel does not take)
  if (k == 7 && s == 2 && p == 3 && !(Cin % 4 == 0 && fn2_conv_mfma_supported(Cin, H, W, Cout, k, s, p)) && fn2_conv_k7s2_relu_supported(Cin, H, W, Cout))
    return FN2_CONV_ROUTE_STEM;
  if (k == 3 && s == 1 && p == 1 && Cout == 2) return FN2_CONV_ROUTE_HEAD;
  const bool wino_ok = k == 3 && s == 1 && fn2_conv_wino_supported(Cin, H, W, Cout, p) != 0;
  // FN2_ROUTE_WINO_BF16X3: the same layers, in split-bf16 arithmetic where that kernel takes them
  const int wino = ((flags & FN2_ROUTE_WINO_BF16X3) && fn2_conv_wino_bf16x3_supported(d)) ? (FN2_CONV_ROUTE_WINOGRAD | FN2_CONV_ARITH_BF16X3) : FN2_CONV_ROUTE_WINOGRAD;
  // accumulator blocks of the Winograd kernel (16 channels x an 8x8-pixel block of tiles): from ~1000 on the launch fills the 1024 SIMDs and
  // it is the fastest kernel of a 3x3 / 1 layer (20x28 maps win by 1.6x, 12x24 maps lose)
  if (wino_ok && (wino_first || (long long)N * ((o.H + 7) / 8) * ((o.W + 7) / 8) * (Cout / 16) >= 1000)) return wino;
  const int maxpix = 8000;
  if (k == 3 && (force || o.H * o.W <= maxpix) && fn2_conv_plane_supported(N, Cin, H, W, Cout, s, p) &&
      (N == d->N || fn2_conv_plane_supported(d->N, Cin, H, W, Cout, s, p)))
    return FN2_CONV_ROUTE_PLANE;       // the encoder layers from 1/16 resolution down: whole planes in LDS, pixels of several samples per tile, split K
  if (k == 5 && s == 2 && p == 2 && (long long)N * ((o.H + 3) / 4) * ((o.W + 3) / 4) * (Cout / 16) < 64 * 256 && o.H * o.W <= maxpix &&
      fn2_conv_plane_k_supported(d->N, Cin, H, W, Cout, 5, 2, 2) && (N == d->N || fn2_conv_plane_k_supported(N, Cin, H, W, Cout, 5, 2, 2)))
    return FN2_CONV_ROUTE_PLANE;       // conv3 of the encoders when one sample is the whole batch: the direct kernel has no K split to fill the chip with
  if (wino_ok) return wino;      // too large for the small-map kernel, too small to fill the chip: still 2.25x fewer multiplies
  if (fn2_conv_mfma_supported(Cin, H, W, Cout, k, s, p))      // FN2_ROUTE_BF16X3: the same layers, in split-bf16 arithmetic where that kernel takes them
    return ((flags & FN2_ROUTE_BF16X3) && fn2_conv_bf16x3_supported(d)) ? (FN2_CONV_ROUTE_DIRECT | FN2_CONV_ARITH_BF16X3) : FN2_CONV_ROUTE_DIRECT;
  return FN2_CONV_ROUTE_NONE;
}

FN2_API size_t fn2_conv_packed_weight_floats(const fn2_conv_desc* d, int route) { return fwd_packed_floats(kConv, d, route); }
FN2_API size_t fn2_conv_workspace_bytes(const fn2_conv_desc* d, int route) { return fwd_workspace_bytes(kConv, d, route); }
FN2_API int fn2_conv_pack_weights(const fn2_conv_desc* d, int route, const float* weight, float* packed, void* stream) {
  return fwd_pack_weights(kConv, d, route, weight, packed, stream);
}
FN2_API int fn2_conv_forward(const fn2_conv_desc* d, int route, const float* bottom, int bottom_channels, int bottom_c0,
                             const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                             int relu, float negative_slope, void* workspace, size_t workspace_bytes, void* stream) {
  return fwd_forward(kConv, d, route,
                     {bottom, bottom_channels, bottom_c0, packed_weight, bias, top, top_channels, top_c0, relu, negative_slope, workspace, workspace_bytes, stream});
}

// ---- Deconvolution{4, 2, 1}: Cin = bottom channels, Cout = top channels, top is [N, Cout, 2 Hin, 2 Win]; weight blob [Cin][Cout][4][4] ----
FN2_API int fn2_deconv_route(const fn2_conv_desc* d, int flags) {
  if (!valid(d) || d->kernel != 4 || d->stride != 2 || d->pad != 1) return FN2_DECONV_ROUTE_NONE;
  if (d->Cin == 2 && d->Cout == 2) return FN2_DECONV_ROUTE_HEAD;       // upsample_flow*: the 2-channel kernel (csrc/flow_head.hip)
  // weight^T x bottom as the 1x1 / GEMM form of the direct kernel + our col2im / bias / ReLU pass: 5-25 % faster than the parity-class kernel
  // on every FlowNet map it takes (profiles/r02_deconv_bench_flownetc.txt); planes whose size is no multiple of 4 (deconv5: 5x7) are not its.
  // FN2_ROUTE_BF16X3: the same layers with the GEMM in split-bf16 arithmetic where that kernel takes them (profiles/deconv_bf16x3_bench.md)
  if (deconv_gemm_ok(d))
    return ((flags & FN2_ROUTE_BF16X3) && fn2_deconv_bf16x3_supported(d)) ? (FN2_DECONV_ROUTE_GEMM | FN2_CONV_ARITH_BF16X3) : FN2_DECONV_ROUTE_GEMM;
  if (fn2_deconv_plane_supported(d->N, d->Cin, d->Hin, d->Win, d->Cout)) return FN2_DECONV_ROUTE_PLANE;
  return FN2_DECONV_ROUTE_NONE;
}

FN2_API size_t fn2_deconv_packed_weight_floats(const fn2_conv_desc* d, int route) { return fwd_packed_floats(kDeconv, d, route); }
FN2_API size_t fn2_deconv_workspace_bytes(const fn2_conv_desc* d, int route) { return fwd_workspace_bytes(kDeconv, d, route); }
FN2_API int fn2_deconv_pack_weights(const fn2_conv_desc* d, int route, const float* weight, float* packed, void* stream) {
  return fwd_pack_weights(kDeconv, d, route, weight, packed, stream);
}
FN2_API int fn2_deconv_forward(const fn2_conv_desc* d, int route, const float* bottom, int bottom_channels, int bottom_c0,
                               const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                               int relu, float negative_slope, void* workspace, size_t workspace_bytes, void* stream) {
  return fwd_forward(kDeconv, d, route,
                     {bottom, bottom_channels, bottom_c0, packed_weight, bias, top, top_channels, top_c0, relu, negative_slope, workspace, workspace_bytes, stream});
}

// =====================================================================================================================================
// Backward by descriptor (declarations and reference citations: include/flownet2_hip.h).  The same decisions flownet2_amd/functional.py
// made in Python through round 4 -- now one function for the autograd mirror and the Caffe adapter's Backward_gpu.
namespace {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Geometry of a data gradient: top_diff [N, Ct, Ht, Wt] -> bottom_diff [N, Cb, Hb, Wb]; the kernels compute Cp >= Cb channels.
struct Bwd { int route, Ct, Ht, Wt, Cb, Hb, Wb, Cp; };

Bwd bwd_geom(const fn2_conv_desc* d, int transposed) {
  Bwd g{FN2_BWD_ROUTE_NONE, 0, 0, 0, 0, 0, 0, 0};
  if (!valid(d)) return g;
  const int k = d->kernel, s = d->stride, p = d->pad, N = d->N;
  g.Cb = d->Cin; g.Hb = d->Hin; g.Wb = d->Win; g.Ct = d->Cout; g.Cp = d->Cin;
  if (transposed) {
    // Deconvolution{4, 2, 1}: the gradient is the 4x4 / 2 / 1 CONVOLUTION of top_diff with the blob as it is ([Cin][Cout][4][4] = [out][in][k][k])
    if (k != 4 || s != 2 || p != 1 || d->Cout % 4 != 0) return g;
    g.Ht = 2 * d->Hin; g.Wt = 2 * d->Win; g.Cp = round_up(d->Cin, 64);
    if (fn2_conv_mfma_supported(g.Ct, g.Ht, g.Wt, g.Cp, 4, 2, 1)) g.route = FN2_BWD_ROUTE_DIRECT;
    else if (d->Cout % 8 == 0 && fn2_conv_plane_k_supported(N, g.Ct, g.Ht, g.Wt, g.Cp, 4, 2, 1)) g.route = FN2_BWD_ROUTE_PLANE;   // deconv5: 10x14 -> 5x7
    return g;
  }
  const Out o = conv_out(d);
  g.Ht = o.H; g.Wt = o.W;
  if (s == 2 && ((k == 5 && p == 2) || (k == 3 && p == 1)) && d->Cin % 64 == 0) {
    if (fn2_tconv_supported(g.Ct, g.Ht, g.Wt, g.Cb, g.Hb, g.Wb, k, p)) { g.route = FN2_BWD_ROUTE_TCONV; return g; }
    // maps whose width is no multiple of 4 (conv5, conv6: top_diff 10x14 / 5x7): the transposed 3x3 / 2 / 1 convolution IS the Deconvolution{4, 2, 1}
    // whose fourth tap row and column are zero (Y = 2 y - 1 + ky in both)
    if (k == 3 && g.Hb == 2 * g.Ht && g.Wb == 2 * g.Wt && fn2_deconv_plane_supported(N, g.Ct, g.Ht, g.Wt, g.Cb)) { g.route = FN2_BWD_ROUTE_DECONV_PLANE; return g; }
  }
  if (k == 1 && s == 1 && p == 0) {
    g.Cp = round_up(d->Cin, 32);
    if (fn2_conv_mfma_supported(g.Ct, g.Ht, g.Wt, g.Cp, 1, 1, 0)) g.route = FN2_BWD_ROUTE_DIRECT;
    return g;
  }
  if (k == 3 && s == 1 && p == 1) {
    g.Cp = round_up(d->Cin, 16);
    if (fn2_conv_wino_supported(g.Ct, g.Ht, g.Wt, g.Cp, 1)) { g.route = FN2_BWD_ROUTE_WINOGRAD; return g; }
    g.Cp = round_up(d->Cin, 64);       // 10x14, 5x7 (conv5_1, conv6_1): the small-map kernel on the same rotated weights
    if (d->Cout % 8 == 0 && fn2_conv_plane_supported(N, g.Ct, g.Ht, g.Wt, g.Cp, 1, 1)) g.route = FN2_BWD_ROUTE_PLANE;
  }
  return g;
}

// [Cout][Cin][3][3] -> [Cp][Cout][3][3]: rotated by 180 degrees, channel axes swapped, rows beyond Cin zero (the blob the Winograd packing reads)
__global__ void __launch_bounds__(256) rot180_swap(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin, int Cp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)Cp * Cout * 9;
  if (i >= total) return;
  const int t = (int)(i % 9);
  const long long r = i / 9;
  const int co = (int)(r % Cout), ci = (int)(r / Cout);
  out[i] = ci < Cin ? w[((size_t)co * Cin + ci) * 9 + (8 - t)] : 0.f;
}

// ---- the data-gradient families: every one runs a forward kernel on top_diff [N, Ct, Ht, Wt] into `out` ----
struct BwdRow;
struct BwdPlan { Bwd g; const BwdRow* row; Desc d; int transposed; };      // row NULL: the route is not this layer's
struct BwdCall {
  const float* top_diff; int top_channels, top_c0; const float* packed;
  float* out; int out_channels, out_c0;                                  // bottom_diff, or the padded result in the workspace
  void* workspace; size_t workspace_bytes;                               // the kernel's own scratch
  const float* mask; int mask_channels, mask_c0; float mask_slope;       // the masked run; the plain one: NULL, 0, 0, 1
  void* stream;
};
struct BwdRow {
  int route;                                     // the value callers pass, arithmetic bit included
  bool (*takes)(Desc, int transposed);           // NULL: every layer bwd_geom gives the base route to
  size_t (*packed_floats)(const BwdPlan&);
  size_t (*pack_scratch)(const BwdPlan&);        // NULL: none
  int (*pack)(const BwdPlan&, const float* weight, float* packed, void* workspace, size_t workspace_bytes, void* stream);
  size_t (*scratch)(const BwdPlan&);             // the kernel's own; NULL: none
  int (*run)(const BwdPlan&, const BwdCall&);
  int (*masked)(const BwdPlan&, const BwdCall&); // with the ReLU derivative of the layer in front folded in; NULL: none
};
#define SIZE(...) [](const BwdPlan& p) -> size_t { return __VA_ARGS__; }
#define PACK(...) [](const BwdPlan& p, const float* weight, float* packed, void*, size_t, void* stream) -> int { return __VA_ARGS__; }
#define RUN(...) [](const BwdPlan& p, const BwdCall& c) -> int { return __VA_ARGS__; }
// what every kernel takes first: top_diff as its bottom, no bias, its geometry and slice (then: the output channels and the output's slice)
#define DIFF c.top_diff, c.packed, nullptr, c.out, p.d->N, p.g.Ct, p.g.Ht, p.g.Wt, c.top_channels, c.top_c0

size_t bwd_mfma_floats(const BwdPlan& p) { return fn2_conv_mfma_packed_floats(p.g.Cp, p.g.Ct, p.d->kernel); }
// operand [Cp][Ct][k][k] of a gradient that runs as a convolution of top_diff: a Convolution's blob [Cout][Cin][k][k] with its channel axes
// swapped (and, `flip`, rotated by 180 degrees), a Deconvolution's [Cin][Cout][4][4] as it is ([out][in][k][k] already)
int bwd_pack_view(const BwdPlan& p, const float* weight, float* packed, int flip, void* stream) {
  const int Cin = p.d->Cin, Cout = p.d->Cout, k = p.d->kernel, kk = k * k;
  return fn2_conv_mfma_pack_weights_view(weight, packed, p.g.Cp, Cout, k, Cin, Cout, p.transposed ? (long long)Cout * kk : kk,
                                         p.transposed ? kk : (long long)Cin * kk, flip, stream);
}
// [Cout][Cin][3][3] -> the rotated, channel-swapped blob in the scratch -> the Winograd packing of that
int bwd_pack_rotated(const BwdPlan& p, const float* weight, float* packed, void* workspace, size_t workspace_bytes, void* stream) {
  const size_t need = p.row->pack_scratch(p);
  if (!workspace || workspace_bytes < need) return fn2::fail(FN2_ERR_WORKSPACE, "conv_backward_data_pack_weights: %zu bytes of scratch needed for the rotated blob", need);
  const long long total = (long long)p.g.Cp * p.d->Cout * 9;
  hipLaunchKernelGGL(rot180_swap, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, fn2::as_stream(stream), weight, static_cast<float*>(workspace), p.d->Cout,
                     p.d->Cin, p.g.Cp);
  if (const int rc = fn2::check_launch("conv_backward_data_pack_weights (rotate)")) return rc;
  return fn2_conv_wino_pack_weights(static_cast<const float*>(workspace), packed, p.g.Cp, p.d->Cout, stream);
}
// the exact and the split-bf16 transposed convolution: the plain run is the masked one without a mask
int tconv_run(const BwdPlan& p, const BwdCall& c) {
  return fn2::tconv_forward_masked(DIFF, p.g.Cb, p.g.Hb, p.g.Wb, c.out_channels, c.out_c0, p.d->kernel, p.d->pad, 0, 0.f, c.mask, c.mask_channels, c.mask_c0, c.mask_slope, c.stream);
}
int tconv_bf16x3_run(const BwdPlan& p, const BwdCall& c) {
  return fn2::tconv_bf16x3_masked(c.top_diff, c.packed, c.out, p.d->N, p.g.Ct, p.g.Ht, p.g.Wt, c.top_channels, c.top_c0, p.g.Cb, p.g.Hb, p.g.Wb, c.out_channels, c.out_c0, p.d->kernel,
                                  p.d->pad, c.mask, c.mask_channels, c.mask_c0, c.mask_slope, c.stream);
}

const BwdRow kBwdRows[] = {
    // 3x3 / 1 / 1: the forward Winograd kernel on the rotated, channel-swapped weights
    {FN2_BWD_ROUTE_WINOGRAD, nullptr, SIZE(fn2_conv_wino_packed_floats(p.g.Cp, p.g.Ct)), SIZE(sizeof(float) * (size_t)p.g.Cp * p.g.Ct * 9), bwd_pack_rotated, nullptr,
     RUN(fn2_conv_wino_forward(DIFF, p.g.Cp, c.out_channels, c.out_c0, 1, 0, 0.f, c.stream)), nullptr},
    // stride 2: operand [Cin][Cout][k][k], the Convolution's own blob with its channel axes swapped (Cp == Cin)
    {FN2_BWD_ROUTE_TCONV, nullptr, bwd_mfma_floats, nullptr, PACK(bwd_pack_view(p, weight, packed, 0, stream)), nullptr, tconv_run, tconv_run},
    {FN2_BWD_ROUTE_TCONV | FN2_CONV_ARITH_BF16X3, [](Desc d, int transposed) { return fn2_tconv_bf16x3_supported(d, transposed) != 0; },      // csrc/tconv_bf16x3.hip
     SIZE(fn2::tconv_bf16x3_packed_floats(p.g.Cb, p.g.Ct, p.d->kernel, p.d->pad)), nullptr,
     PACK(fn2::tconv_bf16x3_pack_weights(weight, packed, p.g.Cb, p.g.Ct, p.d->kernel, p.d->pad, stream)), nullptr, tconv_bf16x3_run, tconv_bf16x3_run},
    // the small-map kernel: 3x3 / 1 / 1 on the rotated weights (10x14, 5x7), or a Deconvolution's 4x4 / 2 / 1
    {FN2_BWD_ROUTE_PLANE, nullptr, bwd_mfma_floats, nullptr, PACK(bwd_pack_view(p, weight, packed, !p.transposed, stream)),
     SIZE(p.transposed ? fn2_conv_plane_k_workspace_bytes(p.d->N, p.g.Ct, p.g.Ht, p.g.Wt, p.g.Cp, 4, 2, 1)
                       : fn2_conv_plane_workspace_bytes(p.d->N, p.g.Ct, p.g.Ht, p.g.Wt, p.g.Cp, 1, 1)),
     RUN(p.transposed ? fn2_conv_plane_k_forward(DIFF, p.g.Cp, c.out_channels, c.out_c0, 4, 2, 1, 0, 0.f, c.workspace, c.workspace_bytes, c.stream)
                      : fn2_conv_plane_forward(DIFF, p.g.Cp, c.out_channels, c.out_c0, 1, 1, 0, 0.f, c.workspace, c.workspace_bytes, c.stream)),
     nullptr},
    // the direct kernel at the layer's own geometry: 1x1 / 1 / 0, or a Deconvolution's 4x4 / 2 / 1
    {FN2_BWD_ROUTE_DIRECT, nullptr, bwd_mfma_floats, nullptr, PACK(bwd_pack_view(p, weight, packed, 0, stream)), nullptr,
     RUN(fn2_conv_mfma_forward(DIFF, p.g.Cp, c.out_channels, c.out_c0, p.d->kernel, p.d->stride, p.d->pad, 0, 0.f, c.stream)), nullptr},
    // 3x3 / 2 / 1 on maps the TCONV kernel does not take: the [Cout][Cin][3][3] blob read as a Deconvolution blob [in = Cout][out = Cin] with zero taps
    {FN2_BWD_ROUTE_DECONV_PLANE, nullptr, SIZE(fn2_deconv_plane_packed_floats(p.g.Ct, p.g.Cb)), nullptr,
     PACK(fn2_deconv_plane_pack_weights_k(weight, packed, p.d->Cout, p.d->Cin, 3, stream)),
     SIZE(fn2_deconv_plane_workspace_bytes(p.d->N, p.g.Ct, p.g.Ht, p.g.Wt, p.g.Cb)),
     RUN(fn2_deconv_plane_forward(DIFF, p.g.Cb, c.out_channels, c.out_c0, 0, 0.f, c.workspace, c.workspace_bytes, c.stream)), nullptr},
};
#undef SIZE
#undef PACK
#undef RUN
#undef DIFF

// The layer's geometry and the row `route_arith` names -- where that is the layer's own route (bwd_geom's), in an arithmetic whose kernel
// takes the layer.  The arithmetic bit on any other base route, on any other layer, or alone names no kernel: sizes 0, calls refused.
BwdPlan bwd_plan(Desc d, int transposed, int route_arith) {
  BwdPlan p{bwd_geom(d, transposed), nullptr, d, transposed};
  if (p.g.route != FN2_BWD_ROUTE_NONE && (route_arith & ~FN2_CONV_ARITH_BF16X3) == p.g.route)
    for (const BwdRow& r : kBwdRows)
      if (r.route == route_arith && (!r.takes || r.takes(d, transposed))) p.row = &r;
  return p;
}

size_t bwd_scratch(const BwdPlan& p) { return p.row->scratch ? p.row->scratch(p) : 0; }
// ... and the padded result, copied into bottom_diff afterwards, where the kernel computes more channels than the layer has
size_t bwd_scratch_and_result(const BwdPlan& p) { return align256(bwd_scratch(p)) + (p.g.Cp != p.g.Cb ? sizeof(float) * (size_t)p.d->N * p.g.Cp * p.g.Hb * p.g.Wb : 0); }
bool bwd_masks(const BwdPlan& p) { return p.row && p.row->masked && p.g.Cp == p.g.Cb; }

}  // namespace

FN2_API int fn2_conv_backward_data_route(const fn2_conv_desc* d, int transposed) { return bwd_geom(d, transposed).route; }

// FN2_ROUTE_BF16X3: the TCONV layers the split-bf16 kernel takes (5x5 / 2 / 2), in that arithmetic; everything else as without the flag
FN2_API int fn2_conv_backward_data_route_flags(const fn2_conv_desc* d, int transposed, int flags) {
  const int route = bwd_geom(d, transposed).route;
  if ((flags & FN2_ROUTE_BF16X3) && route == FN2_BWD_ROUTE_TCONV && fn2_tconv_bf16x3_supported(d, transposed)) return route | FN2_CONV_ARITH_BF16X3;
  return route;
}

FN2_API size_t fn2_conv_backward_data_packed_weight_floats(const fn2_conv_desc* d, int transposed, int route_arith) {
  const BwdPlan p = bwd_plan(d, transposed, route_arith);
  return p.row ? p.row->packed_floats(p) : 0;
}
FN2_API size_t fn2_conv_backward_data_pack_workspace_bytes(const fn2_conv_desc* d, int transposed, int route_arith) {
  const BwdPlan p = bwd_plan(d, transposed, route_arith);
  return p.row && p.row->pack_scratch ? p.row->pack_scratch(p) : 0;
}

FN2_API int fn2_conv_backward_data_pack_weights(const fn2_conv_desc* d, int transposed, int route_arith, const float* weight, float* packed,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  const BwdPlan p = bwd_plan(d, transposed, route_arith);
  if (!weight || !packed) return fn2::fail(FN2_ERR_INVALID_ARG, "conv_backward_data_pack_weights: NULL blob");
  if (!p.row) return fn2::fail(FN2_ERR_UNSUPPORTED, "conv_backward_data_pack_weights: route %d is not this layer's (%d)", route_arith, p.g.route);
  return p.row->pack(p, weight, packed, workspace, workspace_bytes, stream);
}

FN2_API size_t fn2_conv_backward_data_workspace_bytes(const fn2_conv_desc* d, int transposed, int route_arith) {
  const BwdPlan p = bwd_plan(d, transposed, route_arith);
  return p.row ? bwd_scratch_and_result(p) : 0;
}

// the same for a caller whose bottom_diff blob has room for `bottom_room` channels: with room for the computed channels
// (fn2_conv_backward_data_computed_channels) only the kernel's own scratch is needed -- no padded copy
FN2_API size_t fn2_conv_backward_data_workspace_bytes_with_room(const fn2_conv_desc* d, int transposed, int route_arith, int bottom_room) {
  const BwdPlan p = bwd_plan(d, transposed, route_arith);
  return !p.row ? 0 : bottom_room >= p.g.Cp ? bwd_scratch(p) : bwd_scratch_and_result(p);
}
FN2_API int fn2_conv_backward_data_computed_channels(const fn2_conv_desc* d, int transposed, int route_arith) {
  const BwdPlan p = bwd_plan(d, transposed, route_arith);
  return p.row ? p.g.Cp : 0;
}
FN2_API int fn2_conv_backward_data_masked_supported(const fn2_conv_desc* d, int transposed, int route_arith) { return bwd_masks(bwd_plan(d, transposed, route_arith)); }

FN2_API int fn2_conv_backward_data_masked(const fn2_conv_desc* d, int transposed, int route_arith, const float* top_diff, int top_channels, int top_c0,
                                          const float* packed, float* bottom_diff, int bottom_channels, int bottom_c0,
                                          const float* bottom_data, int data_channels, int data_c0, float negative_slope, void* stream) {
  const BwdPlan p = bwd_plan(d, transposed, route_arith);
  if (!bwd_masks(p))
    return fn2::fail(FN2_ERR_UNSUPPORTED, "conv_backward_data_masked: only the transposed-convolution route folds the ReLU derivative of the layer in front");
  if (!top_diff || !packed || !bottom_diff || !bottom_data) return fn2::fail(FN2_ERR_INVALID_ARG, "conv_backward_data_masked: NULL blob");
  if (top_c0 < 0 || top_c0 + p.g.Ct > top_channels || bottom_c0 < 0 || bottom_c0 + p.g.Cb > bottom_channels)
    return fn2::fail(FN2_ERR_INVALID_ARG, "conv_backward_data_masked: channel slice outside its blob");
  return p.row->masked(p, {top_diff, top_channels, top_c0, packed, bottom_diff, bottom_channels, bottom_c0, nullptr, 0, bottom_data, data_channels, data_c0,
                           negative_slope, stream});
}

FN2_API int fn2_conv_backward_data(const fn2_conv_desc* d, int transposed, int route_arith, const float* top_diff, int top_channels, int top_c0,
                                   const float* packed, float* bottom_diff, int bottom_channels, int bottom_c0, int bottom_room,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  const BwdPlan p = bwd_plan(d, transposed, route_arith);
  const Bwd& g = p.g;
  if (!top_diff || !packed || !bottom_diff) return fn2::fail(FN2_ERR_INVALID_ARG, "conv_backward_data: NULL blob");
  if (!p.row)
    return fn2::fail(FN2_ERR_UNSUPPORTED, "conv_backward_data: no own kernel for %s{kernel %d, stride %d, pad %d} %d -> %d on %d x %d (route %d)",
                     transposed ? "Deconvolution" : "Convolution", d ? d->kernel : 0, d ? d->stride : 0, d ? d->pad : 0, d ? d->Cin : 0, d ? d->Cout : 0,
                     d ? d->Hin : 0, d ? d->Win : 0, route_arith);
  if (top_c0 < 0 || top_c0 + g.Ct > top_channels || bottom_c0 < 0 || bottom_room < g.Cb || bottom_c0 + bottom_room > bottom_channels)
    return fn2::fail(FN2_ERR_INVALID_ARG, "conv_backward_data: channel slice outside its blob");
  const size_t kws = bwd_scratch(p);
  const bool padded = g.Cp > bottom_room;               // no room for the surplus channels: through the workspace
  const size_t need = padded ? bwd_scratch_and_result(p) : kws;
  if (need && (!workspace || workspace_bytes < need)) return fn2::fail(FN2_ERR_WORKSPACE, "conv_backward_data: workspace too small (%zu < %zu)", workspace_bytes, need);
  float* out = padded ? reinterpret_cast<float*>(static_cast<char*>(workspace) + align256(kws)) : bottom_diff;
  const int rc = p.row->run(p, {top_diff, top_channels, top_c0, packed, out, padded ? g.Cp : bottom_channels, padded ? 0 : bottom_c0, workspace, kws,
                                nullptr, 0, 0, 1.f, stream});
  if (rc || !padded) return rc;
  // the first Cb of the Cp computed channels of every sample -> the layer's slice of bottom_diff (one strided copy)
  const size_t plane = sizeof(float) * (size_t)g.Hb * g.Wb;
  if (hipMemcpy2DAsync(bottom_diff + (size_t)bottom_c0 * g.Hb * g.Wb, (size_t)bottom_channels * plane, out, (size_t)g.Cp * plane, (size_t)g.Cb * plane, (size_t)d->N,
                       hipMemcpyDeviceToDevice, fn2::as_stream(stream)) != hipSuccess) {
    (void)hipGetLastError();
    return fn2::fail(FN2_ERR_LAUNCH, "conv_backward_data: copy of the padded result failed");
  }
  return FN2_OK;
}

// ---- weight gradient: no route, two arithmetics.  0: the exact kernel (csrc/conv_wgrad.hip), or the stem's; FN2_CONV_ARITH_BF16X3: the
// split-bf16 kernel (csrc/conv_wgrad_bf16x3.hip) on the layers it takes (Convolution{5, 2, 2}).  The plain entry points are arithmetic 0.
namespace {
bool stem_class(const fn2_conv_desc* d, int transposed) {
  return !transposed && d->kernel == 7 && d->stride == 2 && d->pad == 3 && fn2_conv_k7s2_wgrad_supported(d->N, d->Cin, d->Hin, d->Win, d->Cout) != 0;
}
struct WG { int Ca, Ha, Wa, Cb, Hb, Wb; };
WG wg_geom(const fn2_conv_desc* d, int transposed) {          // `a`: the map at the convolution's OUTPUT resolution (conv_wgrad.hip)
  if (transposed) return {d->Cin, d->Hin, d->Win, d->Cout, 2 * d->Hin, 2 * d->Win};
  const Out o = conv_out(d);
  return {d->Cout, o.H, o.W, d->Cin, d->Hin, d->Win};
}

size_t wgrad_workspace(Desc d, int transposed, int arith) {
  if (arith == FN2_CONV_ARITH_BF16X3)
    return fn2_conv_backward_weights_arith(d, transposed, FN2_ROUTE_BF16X3) ? fn2::conv_wgrad_bf16x3_workspace_bytes(d, transposed) : 0;
  if (arith != 0 || !fn2_conv_backward_weights_supported(d, transposed)) return 0;
  if (stem_class(d, transposed)) return fn2_conv_k7s2_wgrad_workspace_bytes(d->N, d->Cin, d->Hin, d->Win, d->Cout);
  const WG w = wg_geom(d, transposed);
  return fn2_conv_wgrad_workspace_bytes(d->N, w.Ca, w.Ha, w.Wa, w.Cb, w.Hb, w.Wb, d->kernel, d->stride, d->pad);
}

int wgrad_run(Desc d, int transposed, int arith, const float* bottom, int bottom_channels, int bottom_c0, const float* top_diff, int top_channels, int top_c0,
              float* weight_diff, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (arith == FN2_CONV_ARITH_BF16X3) {
    if (!fn2_conv_backward_weights_arith(d, transposed, FN2_ROUTE_BF16X3))
      return fn2::fail(FN2_ERR_UNSUPPORTED, "conv_backward_weights_arith_run: the split-bf16 weight gradient does not take this layer");
    return fn2::conv_wgrad_bf16x3(d, transposed, bottom, bottom_channels, bottom_c0, top_diff, top_channels, top_c0, weight_diff, accumulate, workspace,
                                  workspace_bytes, stream);
  }
  if (arith != 0) return fn2::fail(FN2_ERR_UNSUPPORTED, "conv_backward_weights_arith_run: unknown arithmetic 0x%x", arith);
  if (!fn2_conv_backward_weights_supported(d, transposed)) return fn2::fail(FN2_ERR_UNSUPPORTED, "conv_backward_weights: no own kernel for this layer");
  if (!bottom || !top_diff || !weight_diff) return fn2::fail(FN2_ERR_INVALID_ARG, "conv_backward_weights: NULL blob");
  if (stem_class(d, transposed)) {
    if (bottom_channels != d->Cin || bottom_c0 != 0 || top_channels != d->Cout || top_c0 != 0)
      return fn2::fail(FN2_ERR_UNSUPPORTED, "conv_backward_weights: the stem kernel reads whole blobs, not channel slices");
    return fn2_conv_k7s2_wgrad(top_diff, bottom, weight_diff, d->N, d->Cin, d->Hin, d->Win, d->Cout, accumulate, workspace, workspace_bytes, stream);
  }
  const WG w = wg_geom(d, transposed);
  const float* a = transposed ? bottom : top_diff;
  const float* b = transposed ? top_diff : bottom;
  const int ac = transposed ? bottom_channels : top_channels, a0 = transposed ? bottom_c0 : top_c0;
  const int bc = transposed ? top_channels : bottom_channels, b0 = transposed ? top_c0 : bottom_c0;
  return fn2_conv_wgrad(a, b, weight_diff, d->N, w.Ca, w.Ha, w.Wa, ac, a0, w.Cb, w.Hb, w.Wb, bc, b0, d->kernel, d->stride, d->pad, accumulate,
                        workspace, workspace_bytes, stream);
}
}  // namespace

FN2_API int fn2_conv_backward_weights_supported(const fn2_conv_desc* d, int transposed) {
  if (!valid(d)) return 0;
  if (transposed && (d->kernel != 4 || d->stride != 2 || d->pad != 1)) return 0;
  if (stem_class(d, transposed)) return 1;
  const WG w = wg_geom(d, transposed);
  if (w.Ca < 16 || w.Cb < 16) return 0;       // the 2-channel flow heads have kernels of their own (fn2_predict_flow_conv_backward, fn2_upsample_flow_deconv_backward)
  return fn2_conv_wgrad_supported(d->N, w.Ca, w.Ha, w.Wa, w.Cb, w.Hb, w.Wb, d->kernel, d->stride, d->pad) != 0;
}

// FN2_ROUTE_BF16X3: FN2_CONV_ARITH_BF16X3 for the layers the split kernel takes (Convolution{5, 2, 2}), 0 = the exact kernel everywhere else
FN2_API int fn2_conv_backward_weights_arith(const fn2_conv_desc* d, int transposed, int flags) {
  if (!(flags & FN2_ROUTE_BF16X3) || !valid(d)) return 0;
  return fn2_conv_backward_weights_supported(d, transposed) && fn2_conv_wgrad_bf16x3_supported(d, transposed) ? FN2_CONV_ARITH_BF16X3 : 0;
}

FN2_API size_t fn2_conv_backward_weights_workspace_bytes(const fn2_conv_desc* d, int transposed) { return wgrad_workspace(d, transposed, 0); }
FN2_API size_t fn2_conv_backward_weights_workspace_bytes_arith(const fn2_conv_desc* d, int transposed, int arith) { return wgrad_workspace(d, transposed, arith); }
FN2_API int fn2_conv_backward_weights(const fn2_conv_desc* d, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                      const float* top_diff, int top_channels, int top_c0, float* weight_diff, int accumulate,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return wgrad_run(d, transposed, 0, bottom, bottom_channels, bottom_c0, top_diff, top_channels, top_c0, weight_diff, accumulate, workspace, workspace_bytes, stream);
}

FN2_API int fn2_conv_backward_weights_arith_run(const fn2_conv_desc* d, int transposed, int arith, const float* bottom, int bottom_channels, int bottom_c0,
                                                const float* top_diff, int top_channels, int top_c0, float* weight_diff, int accumulate,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  return wgrad_run(d, transposed, arith, bottom, bottom_channels, bottom_c0, top_diff, top_channels, top_c0, weight_diff, accumulate, workspace, workspace_bytes, stream);
}

// weight_diff AND bias_diff of a layer from one pass over top_diff where a kernel has that form (the stem: csrc/conv_stem_wgrad.hip sums
// the operand it feeds to the matrix pipe); 1 = it has
FN2_API int fn2_conv_backward_weights_bias_fused(const fn2_conv_desc* d, int transposed) { return valid(d) && stem_class(d, transposed) ? 1 : 0; }

FN2_API int fn2_conv_backward_weights_bias(const fn2_conv_desc* d, int transposed, const float* bottom, const float* top_diff, float* weight_diff,
                                           float* bias_diff, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (!fn2_conv_backward_weights_bias_fused(d, transposed))
    return fn2::fail(FN2_ERR_UNSUPPORTED, "conv_backward_weights_bias: this layer has no fused weight + bias gradient kernel");
  if (!bottom || !top_diff || !weight_diff || !bias_diff) return fn2::fail(FN2_ERR_INVALID_ARG, "conv_backward_weights_bias: NULL blob");
  return fn2::conv_k7s2_wgrad_bias(top_diff, bottom, weight_diff, bias_diff, d->N, d->Cin, d->Hin, d->Win, d->Cout, accumulate, workspace, workspace_bytes, stream);
}
