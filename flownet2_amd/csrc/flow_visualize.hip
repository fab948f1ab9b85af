// Flow visualisation for gfx950: the Middlebury colour coding of a flow [N,2,H,W] and the KITTI-style error image of a prediction against
// ground truth, as interleaved bytes [N,H,W,3] -- one streaming pass each (8 bytes read and 3 written per pixel; the per-sample
// normalisation of the colour coding reads the flow once more, in a launch of its own, for its maximum).
//
// Composed from eager tensor operations either picture is some dozens of launches with a temporary of the full map each, and the
// maximum is read back by the host where a script divides by it.  Here a thread reads its pixels' planes, decides, and stores the bytes;
// the maximum goes through the workspace: flow_color_max writes one float per workgroup, flow_color reduces the at most 128 of its sample
// (all of them under NORM_BATCH).  A maximum does not depend on order, so there is nothing to fix about the order: no float atomics,
// nothing read back by the host, the same bytes for a sample alone and in any batch.
//
// A work item is (sample, chunk), B chunks per sample, B from H * W alone, as in flow_metrics.hip and flow_consistency.hip.  A thread owns
// one pixel per step, or four neighbouring pixels of a row where W is a multiple of 4; those are read as 16-byte loads where every float
// pointer given is 16-byte aligned and written as three 4-byte stores where rgb is 4-byte aligned (H W is then a multiple of 4, so a
// sample's first byte, 3 n H W, keeps the alignment of rgb).  Every operation is rounded on its own (fp contract off):
// include/flownet2_hip_flow_visualize.h states the arithmetic.
//
// Writes stay inside [N,H,W,3]: a unit is V pixels at r = u * V < H W with r + V <= H W (V == 4 only where 4 divides W, hence H W), and its
// bytes are 3 (n H W + r) .. 3 (n H W + r + V) - 1.  The wheel index is formed only for a known pixel (ok(u) && ok(v), so atan2f is a
// number) and is clamped to 0 .. 54.
#include "stream_reduce.hpp"
#include "../../include/flownet2_hip_flow_visualize.h"

#pragma clang fp contract(off)

namespace fn2 {

using namespace stream;

constexpr int kFvWheelSize = 55;
constexpr int kFvBins = 10;

// wheel entry k as R | G << 8 | B << 16
struct FvWheel {
  unsigned rgb[kFvWheelSize];
};

constexpr FvWheel fv_make_wheel() {
  FvWheel w = {};
  int k = 0;
  for (int i = 0; i < 15; ++i) w.rgb[k++] = 255u | (unsigned)(255 * i / 15) << 8;                          // RY
  for (int i = 0; i < 6; ++i) w.rgb[k++] = (unsigned)(255 - 255 * i / 6) | 255u << 8;                      // YG
  for (int i = 0; i < 4; ++i) w.rgb[k++] = 255u << 8 | (unsigned)(255 * i / 4) << 16;                      // GC
  for (int i = 0; i < 11; ++i) w.rgb[k++] = (unsigned)(255 - 255 * i / 11) << 8 | 255u << 16;              // CB
  for (int i = 0; i < 13; ++i) w.rgb[k++] = (unsigned)(255 * i / 13) | 255u << 16;                         // BM
  for (int i = 0; i < 6; ++i) w.rgb[k++] = 255u | (unsigned)(255 - 255 * i / 6) << 16;                     // MR
  return w;
}

constexpr FvWheel kFvWheelHost = fv_make_wheel();
static_assert(kFvWheelHost.rgb[0] == 0x0000FFu && kFvWheelHost.rgb[15] == 0x00FFFFu && kFvWheelHost.rgb[21] == 0x00FF00u &&
              kFvWheelHost.rgb[25] == 0xFFFF00u && kFvWheelHost.rgb[36] == 0xFF0000u && kFvWheelHost.rgb[49] == 0xFF00FFu &&
              kFvWheelHost.rgb[54] == (255u | 43u << 16), "the colour wheel's check points");
__constant__ FvWheel kFvWheel = fv_make_wheel();

// the error image's bins: lower edges of bins 1 .. 9, and the colours as R | G << 8 | B << 16
__constant__ float kFvEdges[kFvBins - 1] = {0.0625f, 0.125f, 0.25f, 0.5f, 1.f, 2.f, 4.f, 8.f, 16.f};
constexpr unsigned fv_rgb(unsigned r, unsigned g, unsigned b) { return r | g << 8 | b << 16; }
__constant__ unsigned kFvBinColor[kFvBins] = {fv_rgb(49, 54, 149),   fv_rgb(69, 117, 180), fv_rgb(116, 173, 209), fv_rgb(171, 217, 233),
                                              fv_rgb(224, 243, 248), fv_rgb(254, 224, 144), fv_rgb(253, 174, 97), fv_rgb(244, 109, 67),
                                              fv_rgb(215, 48, 39),   fv_rgb(165, 0, 38)};

struct FvColorArgs {
  const float* flow;
  unsigned char* rgb;
  float* maxrad_out;           // [N] or NULL
  float* partial;              // [N][B] (NULL under NORM_FIXED)
  int N, H, W;
  int chunks;                  // B
  int quad;                    // W % 4 == 0: four pixels per thread and step
  int vec;                     // and flow 16-byte aligned: 16-byte loads
  int words;                   // and rgb 4-byte aligned: 4-byte stores
  int norm;
  float max_flow;
};

struct FvErrorArgs {
  const float* pred; const float* gt; const float* valid; const float* occ;
  unsigned char* rgb;
  int N, H, W;
  int chunks, quad, vec, words;
  float abs_thresh, rel_thresh;
};

// V pixels' colours (R | G << 8 | B << 16 each) -> the 3 V bytes at p; `words`: p is 4-byte aligned and V == 4
template <int V>
__device__ __forceinline__ void fv_store(unsigned char* __restrict__ p, const unsigned (&c)[V], bool words) {
  if constexpr (V == 4) {
    if (words) {
      unsigned* q = reinterpret_cast<unsigned*>(p);
      q[0] = c[0] | c[1] << 24;                              // R0 G0 B0 R1
      q[1] = c[1] >> 8 | c[2] << 16;                         // G1 B1 R2 G2
      q[2] = c[2] >> 16 | c[3] << 8;                         // B2 R3 G3 B3
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    p[3 * k + 0] = (unsigned char)(c[k] & 255u);
    p[3 * k + 1] = (unsigned char)(c[k] >> 8 & 255u);
    p[3 * k + 2] = (unsigned char)(c[k] >> 16 & 255u);
  }
}

__device__ __forceinline__ float fv_rad(float u, float v) { return sqrtf(u * u + v * v); }      // the one radius of both launches

// ---- the maximum -----------------------------------------------------------------------------------------------------------------------
template <int V, bool VEC>
__device__ __forceinline__ float fv_max_chunk(const FvColorArgs& a, long long n, int chunk) {
  const size_t hw = (size_t)a.H * a.W;
  const long long units = (long long)(hw / V);
  const float* __restrict__ pu_ = a.flow + (size_t)n * 2 * hw;
  const float* __restrict__ pv_ = pu_ + hw;
  float m = 0.f;
  for (long long u = (long long)chunk * kThreads + threadIdx.x; u < units; u += (long long)a.chunks * kThreads) {
    const size_t r = (size_t)u * V;
    float cu[V], cv[V];
    load<V, VEC>(pu_ + r, cu);
    load<V, VEC>(pv_ + r, cv);
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (finite_1e9(cu[k]) && finite_1e9(cv[k])) m = fmaxf(m, fv_rad(cu[k], cv[k]));
  }
  return m;
}

__global__ void __launch_bounds__(kThreads) flow_color_max(FvColorArgs a) {
  __shared__ float lds[4];
  const long long items = (long long)a.N * a.chunks;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const long long n = w / a.chunks;
    const int chunk = (int)(w % a.chunks);
    float m;
    if (!a.quad) m = fv_max_chunk<1, false>(a, n, chunk);
    else if (a.vec) m = fv_max_chunk<4, true>(a, n, chunk);
    else m = fv_max_chunk<4, false>(a, n, chunk);
    m = block_max(m, lds);
    if (threadIdx.x == 0) a.partial[w] = m;
  }
}

// ---- the colour coding -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned fv_color_pixel(float u, float v, float maxrad) {
  if (!finite_1e9(u) || !finite_1e9(v)) return 0u;
  const float rn = fv_rad(u, v) / maxrad;
  const float ang = atan2f(-v, -u) / 3.14159265358979323846f;
  const float fk = ((ang + 1.0f) * 0.5f) * 54.0f;
  const int k0 = max(min((int)fk, kFvWheelSize - 1), 0);     // fk lies in [0, 54] up to rounding; the clamp keeps the table index inside
  const int k1 = k0 + 1 == kFvWheelSize ? 0 : k0 + 1;
  const float f = fk - (float)k0;
  const unsigned w0 = kFvWheel.rgb[k0], w1 = kFvWheel.rgb[k1];
  unsigned out = 0u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float c0 = (float)(w0 >> 8 * ch & 255u), c1 = (float)(w1 >> 8 * ch & 255u);
    const float c = c0 + f * (c1 - c0);
    const float o = rn <= 1.0f ? 255.0f - rn * (255.0f - c) : 0.75f * c;
    out |= ((unsigned)(int)o & 255u) << 8 * ch;
  }
  return out;
}

template <int V, bool VEC>
__device__ __forceinline__ void fv_color_chunk(const FvColorArgs& a, long long n, int chunk, float maxrad) {
  const size_t hw = (size_t)a.H * a.W;
  const long long units = (long long)(hw / V);
  const float* __restrict__ pu_ = a.flow + (size_t)n * 2 * hw;
  const float* __restrict__ pv_ = pu_ + hw;
  unsigned char* __restrict__ out = a.rgb + 3 * (size_t)n * hw;
  for (long long u = (long long)chunk * kThreads + threadIdx.x; u < units; u += (long long)a.chunks * kThreads) {
    const size_t r = (size_t)u * V;
    float cu[V], cv[V];
    unsigned c[V];
    load<V, VEC>(pu_ + r, cu);
    load<V, VEC>(pv_ + r, cv);
#pragma unroll
    for (int k = 0; k < V; ++k) c[k] = fv_color_pixel(cu[k], cv[k], maxrad);
    fv_store<V>(out + 3 * r, c, a.words != 0);
  }
}

__global__ void __launch_bounds__(kThreads) flow_color(FvColorArgs a) {
  __shared__ float lds[4];
  const long long items = (long long)a.N * a.chunks;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const long long n = w / a.chunks;
    const int chunk = (int)(w % a.chunks);
    float maxrad = a.max_flow;
    if (a.norm != FN2_FLOW_COLOR_NORM_FIXED) {
      // this sample's B <= 128 partial maxima, or all N B of the batch
      const long long first = a.norm == FN2_FLOW_COLOR_NORM_BATCH ? 0 : n * a.chunks;
      const long long count = a.norm == FN2_FLOW_COLOR_NORM_BATCH ? items : a.chunks;
      float m = 0.f;
      for (long long i = threadIdx.x; i < count; i += kThreads) m = fmaxf(m, a.partial[first + i]);
      m = block_max(m, lds);
      maxrad = m > 0.f ? m : 1.0f;
    }
    if (chunk == 0 && threadIdx.x == 0 && a.maxrad_out) a.maxrad_out[n] = maxrad;
    if (!a.quad) fv_color_chunk<1, false>(a, n, chunk, maxrad);
    else if (a.vec) fv_color_chunk<4, true>(a, n, chunk, maxrad);
    else fv_color_chunk<4, false>(a, n, chunk, maxrad);
  }
}

// ---- the error image -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned fv_half(unsigned c) {
  unsigned out = 0u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out |= ((unsigned)(int)(0.5f * (float)(c >> 8 * ch & 255u)) & 255u) << 8 * ch;
  return out;
}

__device__ __forceinline__ unsigned fv_error_pixel(const FvErrorArgs& a, float pu, float pv, float gu, float gv, bool use, bool occluded) {
  unsigned c = 0u;
  if (use && finite_1e9(gu) && finite_1e9(gv)) {
    int bin = kFvBins - 1;
    if (finite_1e9(pu) && finite_1e9(pv)) {
      const float du = pu - gu, dv = pv - gv;
      const float epe = sqrtf(du * du + dv * dv);
      const float mag = sqrtf(gu * gu + gv * gv);
      float n = epe / a.abs_thresh;
      if (mag > 0.f) n = fminf(n, (epe / mag) / a.rel_thresh);
      bin = 0;
#pragma unroll
      for (int k = 0; k < kFvBins - 1; ++k) bin += n >= kFvEdges[k] ? 1 : 0;
    }
    c = kFvBinColor[bin];
  }
  return occluded ? fv_half(c) : c;
}

template <int V, bool VEC>
__device__ __forceinline__ void fv_error_chunk(const FvErrorArgs& a, long long n, int chunk) {
  const size_t hw = (size_t)a.H * a.W;
  const long long units = (long long)(hw / V);
  const float* __restrict__ pu_ = a.pred + (size_t)n * 2 * hw;
  const float* __restrict__ gu_ = a.gt + (size_t)n * 2 * hw;
  unsigned char* __restrict__ out = a.rgb + 3 * (size_t)n * hw;
  for (long long u = (long long)chunk * kThreads + threadIdx.x; u < units; u += (long long)a.chunks * kThreads) {
    const size_t r = (size_t)u * V;
    float pu[V], pv[V], gu[V], gv[V], use[V], oc[V];
    unsigned c[V];
    load<V, VEC>(pu_ + r, pu);
    load<V, VEC>(pu_ + hw + r, pv);
    load<V, VEC>(gu_ + r, gu);
    load<V, VEC>(gu_ + hw + r, gv);
    if (a.valid) load<V, VEC>(a.valid + (size_t)n * hw + r, use);
    if (a.occ) load<V, VEC>(a.occ + (size_t)n * hw + r, oc);
#pragma unroll
    for (int k = 0; k < V; ++k)
      c[k] = fv_error_pixel(a, pu[k], pv[k], gu[k], gv[k], a.valid ? use[k] != 0.f : true, a.occ ? oc[k] != 0.f : false);
    fv_store<V>(out + 3 * r, c, a.words != 0);
  }
}

__global__ void __launch_bounds__(kThreads) flow_error_map(FvErrorArgs a) {
  const long long items = (long long)a.N * a.chunks;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const long long n = w / a.chunks;
    const int chunk = (int)(w % a.chunks);
    if (!a.quad) fv_error_chunk<1, false>(a, n, chunk);
    else if (a.vec) fv_error_chunk<4, true>(a, n, chunk);
    else fv_error_chunk<4, false>(a, n, chunk);
  }
}

static int fv_shape(const char* what, int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return fail(FN2_ERR_INVALID_ARG, "%s: bad shape [%d,2,%d,%d]", what, N, H, W);
  return check_planes(what, N, 2, H, W);
}

static size_t fv_ws_bytes(int N, int H, int W) { return sizeof(float) * (size_t)N * chunks((long long)H * W); }

static bool fv_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_flow_visualize_sizes(int N, int H, int W, size_t* workspace_bytes) {
  int rc = fv_shape("flow_visualize_sizes", N, H, W);
  if (rc) return rc;
  if (workspace_bytes) *workspace_bytes = fv_ws_bytes(N, H, W);
  return FN2_OK;
}

FN2_API int fn2_flow_color(const float* flow, int N, int H, int W, int norm, float max_flow, unsigned char* rgb, float* maxrad_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "flow_color";
  if (!flow) return fail(FN2_ERR_INVALID_ARG, "%s: flow == NULL", what);
  if (!rgb) return fail(FN2_ERR_INVALID_ARG, "%s: rgb == NULL", what);
  int rc = fv_shape(what, N, H, W);
  if (rc) return rc;
  if (norm != FN2_FLOW_COLOR_NORM_SAMPLE && norm != FN2_FLOW_COLOR_NORM_BATCH && norm != FN2_FLOW_COLOR_NORM_FIXED)
    return fail(FN2_ERR_INVALID_ARG, "%s: unknown norm %d", what, norm);
  const bool fixed = norm == FN2_FLOW_COLOR_NORM_FIXED;
  if (fixed && !(max_flow > 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: max_flow = %g (need > 0)", what, max_flow);
  if (!fixed && (!workspace || workspace_bytes < fv_ws_bytes(N, H, W)))
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, fv_ws_bytes(N, H, W));
  FvColorArgs a;
  a.flow = flow;
  a.rgb = rgb;
  a.maxrad_out = maxrad_out;
  a.partial = fixed ? nullptr : reinterpret_cast<float*>(workspace);
  a.N = N; a.H = H; a.W = W;
  a.chunks = chunks((long long)H * W);
  a.quad = (W % 4) == 0;
  a.vec = a.quad && aligned16(flow);
  a.words = a.quad && fv_aligned4(rgb);
  a.norm = norm;
  a.max_flow = fixed ? max_flow : 0.f;
  const long long items = (long long)N * a.chunks;
  const dim3 grid = grid_for(items);
  hipStream_t st = as_stream(stream);
  if (!fixed) hipLaunchKernelGGL(flow_color_max, grid, dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(flow_color, grid, dim3(kThreads), 0, st, a);
  return check_launch(what);
}

FN2_API int fn2_flow_error_map(const float* pred, const float* gt, const float* valid, const float* occ, int N, int H, int W,
                               float abs_thresh, float rel_thresh, unsigned char* rgb, void* stream) {
  const char* what = "flow_error_map";
  if (!pred) return fail(FN2_ERR_INVALID_ARG, "%s: pred == NULL", what);
  if (!gt) return fail(FN2_ERR_INVALID_ARG, "%s: gt == NULL", what);
  if (!rgb) return fail(FN2_ERR_INVALID_ARG, "%s: rgb == NULL", what);
  int rc = fv_shape(what, N, H, W);
  if (rc) return rc;
  if (!(abs_thresh > 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: abs_thresh = %g (need > 0)", what, abs_thresh);
  if (!(rel_thresh > 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: rel_thresh = %g (need > 0)", what, rel_thresh);
  FvErrorArgs a;
  a.pred = pred; a.gt = gt; a.valid = valid; a.occ = occ;
  a.rgb = rgb;
  a.N = N; a.H = H; a.W = W;
  a.chunks = chunks((long long)H * W);
  a.quad = (W % 4) == 0;
  a.vec = a.quad && aligned16(pred) && aligned16(gt) && aligned16(valid) && aligned16(occ);
  a.words = a.quad && fv_aligned4(rgb);
  a.abs_thresh = abs_thresh; a.rel_thresh = rel_thresh;
  const long long items = (long long)N * a.chunks;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(flow_error_map, grid_for(items), dim3(kThreads), 0, st, a);
  return check_launch(what);
}
