// Flow error metrics for gfx950: end-point error (sum, sum of squares, max), KITTI's Fl outliers, Sintel's three speed bands and its
// occluded split, and the angular error, of pred against gt [N,2,H,W] -- per sample and in total, in fp64, in two launches.
//
// Written as eager tensor operations this is two dozen launches with boolean temporaries of the full map and reductions whose order
// follows the batch.  Here, as in l1loss.hip and lpq_loss.hip: ONE streaming pass (validity, differences, two sqrtf, one atan2f, the
// classifications, wave64 reduction -> LDS -> one fp64 partial row per workgroup) plus a one-workgroup finalise that adds a sample's
// partial rows in index order and the sample rows in sample order.  No atomics on floats, nothing read back by the host.
//
// The summation order is a function of (H, W) alone: a workgroup belongs to ONE sample (work item = sample x chunk, B chunks per sample,
// B from H * W), so a sample's row has the same bits alone and in any batch.  A thread owns one pixel per step, or four neighbouring
// pixels of a plane where H * W is a multiple of 4; those are read as one 16-byte load per plane where every pointer given is 16-byte
// aligned and as four 4-byte loads otherwise -- the same values in the same order.  Every operation is rounded on its own (fp contract
// off): include/flownet2_hip_flow_metrics.h states the arithmetic.
//
// -Rpass-analysis=kernel-resource-usage (gfx950, -O3; the kernel holds the three load forms):
//   flow_metrics_partial  VGPRs 83  SGPRs 106  LDS 480 B  occupancy 5     flow_metrics_final  VGPRs 56  SGPRs 72  LDS 61440 B  occupancy 2
// no scratch in either.
#include "stream_reduce.hpp"
#include "../../include/flownet2_hip_flow_metrics.h"

#pragma clang fp contract(off)

namespace fn2 {

using namespace stream;

constexpr int kFmK = FN2_FLOW_METRICS_K;
constexpr unsigned kFmMaxMask = 1u << FN2_FLOW_METRICS_EPE_MAX;      // the column reduced by max

struct FmArgs {
  const float* pred; const float* gt; const float* valid; const float* occ;
  float* epe_map;
  double* partial;       // [N * B][K]
  double* results;       // [N + 1][K]
  int N, H, W;
  int chunks;            // B
  int quad;              // H * W % 4 == 0: four pixels per thread and step
  int vec;               // and every pointer given 16-byte aligned: 16-byte loads / stores
  float outlier_abs, outlier_rel, band0, band1;
};

// what one thread has seen; counts stay integers until the reduction (a thread sees fewer than 2^31 pixels)
struct FmAcc {
  double epe, sq, ae, band_epe[3], occ_epe;
  int valid, nonfinite, outliers, band[3], occ;
  float emax;
};

__device__ __forceinline__ bool fm_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for NaN and +-Inf

// One pixel; returns epe, NaN where the pixel is not counted.
__device__ __forceinline__ float fm_pixel(const FmArgs& a, float pu, float pv, float gu, float gv, bool use, bool occluded, FmAcc& t) {
  const bool valid = use && gu == gu && gv == gv && fabsf(gu) <= 1e9f && fabsf(gv) <= 1e9f;
  if (!valid) return __builtin_nanf("");
  if (!fm_finite(pu) || !fm_finite(pv)) {
    t.nonfinite += 1;
    return __builtin_nanf("");
  }
  const float du = pu - gu, dv = pv - gv;
  const float s = du * du + dv * dv;
  const float epe = sqrtf(s);
  const float mag = sqrtf(gu * gu + gv * gv);
  const float cx = pv - gv, cy = gu - pu, cz = pu * gv - pv * gu;
  const float ae = atan2f(sqrtf((cx * cx + cy * cy) + cz * cz), (1.f + pu * gu) + pv * gv);
  const int band = mag < a.band0 ? 0 : mag < a.band1 ? 1 : 2;
  t.valid += 1;
  t.epe += (double)epe;
  t.sq += (double)s;
  t.ae += (double)ae;
  t.emax = fmaxf(t.emax, epe);
  t.outliers += (epe > a.outlier_abs && epe > a.outlier_rel * mag) ? 1 : 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    t.band[b] += band == b ? 1 : 0;
    t.band_epe[b] += band == b ? (double)epe : 0.0;          // x + 0.0 leaves the bits of a non-negative sum
  }
  t.occ += occluded ? 1 : 0;
  t.occ_epe += occluded ? (double)epe : 0.0;
  return epe;
}

// Chunk `chunk` of sample n: units chunk * 256 + thread, then every B * 256 further on; row -> partial[(n * B + chunk) * K].
template <int V, bool VEC>
__device__ __forceinline__ void fm_chunk(const FmArgs& a, long long n, int chunk, double (*lds)[kFmK]) {
  const size_t hw = (size_t)a.H * a.W;
  const long long units = (long long)(hw / V);
  const float* __restrict__ pu_ = a.pred + (size_t)n * 2 * hw;
  const float* __restrict__ gu_ = a.gt + (size_t)n * 2 * hw;
  FmAcc t = {};
  for (long long u = (long long)chunk * kThreads + threadIdx.x; u < units; u += (long long)a.chunks * kThreads) {
    const size_t r = (size_t)u * V;
    float pu[V], pv[V], gu[V], gv[V], use[V], oc[V], e[V];
    load<V, VEC>(pu_ + r, pu);
    load<V, VEC>(pu_ + hw + r, pv);
    load<V, VEC>(gu_ + r, gu);
    load<V, VEC>(gu_ + hw + r, gv);
    if (a.valid) load<V, VEC>(a.valid + (size_t)n * hw + r, use);
    if (a.occ) load<V, VEC>(a.occ + (size_t)n * hw + r, oc);
#pragma unroll
    for (int k = 0; k < V; ++k)
      e[k] = fm_pixel(a, pu[k], pv[k], gu[k], gv[k], a.valid ? use[k] != 0.f : true, a.occ ? oc[k] != 0.f : false, t);
    if (a.epe_map) store<V, VEC>(a.epe_map + (size_t)n * hw + r, e);
  }
  double row[kFmK];
  row[FN2_FLOW_METRICS_VALID] = (double)t.valid;
  row[FN2_FLOW_METRICS_NONFINITE] = (double)t.nonfinite;
  row[FN2_FLOW_METRICS_EPE_SUM] = t.epe;
  row[FN2_FLOW_METRICS_EPE_SQ_SUM] = t.sq;
  row[FN2_FLOW_METRICS_EPE_MAX] = (double)t.emax;
  row[FN2_FLOW_METRICS_OUTLIERS] = (double)t.outliers;
  row[FN2_FLOW_METRICS_AE_SUM] = t.ae;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    row[FN2_FLOW_METRICS_BAND_COUNT0 + b] = (double)t.band[b];
    row[FN2_FLOW_METRICS_BAND_EPE_SUM0 + b] = t.band_epe[b];
  }
  row[FN2_FLOW_METRICS_OCC_COUNT] = (double)t.occ;
  row[FN2_FLOW_METRICS_OCC_EPE_SUM] = t.occ_epe;
  reduce_row<kFmK, kFmMaxMask>(row, lds, a.partial + ((size_t)n * a.chunks + chunk) * kFmK);
}

__global__ void __launch_bounds__(kThreads) flow_metrics_partial(FmArgs a) {
  __shared__ double lds[4][kFmK];
  const long long items = (long long)a.N * a.chunks;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const long long n = w / a.chunks;
    const int chunk = (int)(w % a.chunks);
    if (!a.quad) fm_chunk<1, false>(a, n, chunk, lds);
    else if (a.vec) fm_chunk<4, true>(a, n, chunk, lds);
    else fm_chunk<4, false>(a, n, chunk, lds);
  }
}

// dst[0 .. cnt) = src[0 .. cnt) by T threads, sixteen loads of a thread in flight before the first is stored: a plain copy loop waits
// for each load in turn (measured: 0.4 us per step, 30 steps for a sample of 128 partial rows).
template <int T>
__device__ __forceinline__ void fm_stage(double* dst, const double* __restrict__ src, int cnt, int t) {
  for (int i0 = t; i0 < cnt; i0 += 16 * T) {
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = i0 + j * T < cnt ? src[i0 + j * T] : 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (i0 + j * T < cnt) dst[i0 + j * T] = v[j];
  }
}

// One workgroup.  The additions are chains in index order, so what is spread over the threads is the reading: a wave copies the partial
// rows of S = 128 / B consecutive samples (one contiguous piece of the workspace) into its quarter of the LDS buffer with all its loads
// in flight at once, then a lane per (sample, column) adds that sample's B partials from LDS in index order.  The totals row likewise:
// 512 sample rows at a time into LDS, then a thread per column adds them in sample order.
__global__ void __launch_bounds__(kThreads) flow_metrics_final(FmArgs a) {
  constexpr int kStage = kMaxChunks * kFmK;              // doubles per wave
  __shared__ double lds[4 * kStage];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int B = a.chunks, S = kMaxChunks / B;
  double* stage = lds + wid * kStage;
  for (long long base = 0; base < a.N; base += 4 * S) {    // the same trip count in every wave: the barriers are uniform
    const long long n0 = base + (long long)wid * S;
    const long long left = a.N - n0;
    const int ns = (int)(left < 0 ? 0 : left < S ? left : S);
    const int cnt = ns * B * kFmK;
    const double* __restrict__ src = a.partial + (size_t)(n0 < a.N ? n0 : 0) * B * kFmK;
    fm_stage<64>(stage, src, cnt, lane);
    __syncthreads();
    const int k = lane & 15;
    if (k < kFmK) {
      for (int s = lane >> 4; s < ns; s += 4) {
        const double* p = stage + s * B * kFmK + k;
        double v = 0.0;
#pragma unroll 8
        for (int b = 0; b < B; ++b) v = k == FN2_FLOW_METRICS_EPE_MAX ? fmax(v, p[b * kFmK]) : v + p[b * kFmK];
        a.results[(size_t)(n0 + s) * kFmK + k] = v;
      }
    }
    __syncthreads();
  }
  __threadfence_block();                                   // the sample rows, written by other threads of this workgroup, are read below
  __syncthreads();
  constexpr int kRows = 4 * kStage / kFmK;                 // 512 sample rows fill the buffer
  double total = 0.0;
  for (long long base = 0; base < a.N; base += kRows) {
    const long long left = a.N - base;
    const int rows = (int)(left < kRows ? left : kRows);
    const double* src = a.results + (size_t)base * kFmK;
    fm_stage<kThreads>(lds, src, rows * kFmK, threadIdx.x);
    __syncthreads();
    if (threadIdx.x < kFmK) {
      const int k = threadIdx.x;
#pragma unroll 8
      for (int r = 0; r < rows; ++r) total = k == FN2_FLOW_METRICS_EPE_MAX ? fmax(total, lds[r * kFmK + k]) : total + lds[r * kFmK + k];
    }
    __syncthreads();
  }
  if (threadIdx.x < kFmK) a.results[(size_t)a.N * kFmK + threadIdx.x] = total;
}

static int fm_shape(const char* what, int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return fail(FN2_ERR_INVALID_ARG, "%s: bad shape [%d,2,%d,%d]", what, N, H, W);
  return check_planes(what, N, 2, H, W);
}

static size_t fm_ws_bytes(int N, int H, int W) { return sizeof(double) * kFmK * (size_t)N * chunks((long long)H * W); }

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_flow_metrics_sizes(int N, int H, int W, size_t* workspace_bytes, int* K) {
  int rc = fm_shape("flow_metrics_sizes", N, H, W);
  if (rc) return rc;
  if (workspace_bytes) *workspace_bytes = fm_ws_bytes(N, H, W);
  if (K) *K = kFmK;
  return FN2_OK;
}

FN2_API int fn2_flow_metrics(const float* pred, const float* gt, const float* valid, const float* occ, int N, int H, int W,
                             float outlier_abs, float outlier_rel, float band0, float band1, double* results, float* epe_map,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "flow_metrics";
  if (!pred || !gt || !results) return fail(FN2_ERR_INVALID_ARG, "%s: pred, gt or results == NULL", what);
  int rc = fm_shape(what, N, H, W);
  if (rc) return rc;
  if (!(outlier_abs >= 0.f) || !(outlier_rel >= 0.f) || !(band0 >= 0.f) || !(band1 >= 0.f))
    return fail(FN2_ERR_INVALID_ARG, "%s: outlier_abs = %g, outlier_rel = %g, band0 = %g, band1 = %g (need >= 0)", what, outlier_abs, outlier_rel,
                band0, band1);
  if (!(band0 < band1)) return fail(FN2_ERR_INVALID_ARG, "%s: band0 = %g >= band1 = %g", what, band0, band1);
  if (!workspace || workspace_bytes < fm_ws_bytes(N, H, W))
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, fm_ws_bytes(N, H, W));
  FmArgs a;
  a.pred = pred; a.gt = gt; a.valid = valid; a.occ = occ; a.epe_map = epe_map;
  a.partial = reinterpret_cast<double*>(workspace);
  a.results = results;
  a.N = N; a.H = H; a.W = W;
  const long long hw = (long long)H * W;
  a.chunks = chunks(hw);
  a.quad = (hw % 4) == 0;
  a.vec = a.quad && aligned16(pred) && aligned16(gt) && aligned16(valid) && aligned16(occ) && aligned16(epe_map);
  a.outlier_abs = outlier_abs; a.outlier_rel = outlier_rel; a.band0 = band0; a.band1 = band1;
  const long long items = (long long)N * a.chunks;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(flow_metrics_partial, grid_for(items), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(flow_metrics_final, dim3(1), dim3(kThreads), 0, st, a);
  return check_launch(what);
}
