// Building blocks shared by the "one streaming pass + one-workgroup finalise" kernels (l1loss, lpq_loss, flow_metrics, flow_consistency,
// flow_visualize, flow_track, unsup_loss): the launch constants, the four-pixel load / store, the wave64 and workgroup reductions, the tail
// of a chunk (a thread's row -> the workgroup's partial row), the plain finalise, the finite test, FlowWarp's bilinear taps, and on the
// host the chunk count, the alignment test, the grid and the 2^31 shape check.
//
// These carry what the seven files promise: a summation order that is a function of the shape alone (shuffle tree 32 .. 1, the four waves
// in order, partial rows in index order, sample rows in sample order -- no atomics on floats), so the same bits for a sample alone and in
// any batch; and the same values in the same order from one 16-byte access as from four 4-byte ones.  A change here moves the bits of all
// of them at once: tests/test_stream_bits.py pins them.
//
// Everything on the device side is a __device__ __forceinline__ FUNCTION, never a lambda (see mfma_tile.hpp).  Floating-point contraction
// follows where a function is DEFINED, not where it is inlined, and the files that include this differ (l1loss.hip contracts outside its
// _multi kernels, the others nowhere): so there is no pragma at file scope here, and a helper that multiplies and adds floats states
// `#pragma clang fp contract(off)` inside its own body.
#pragma once

#include <cstdint>

#include "fn2_common.hpp"

namespace fn2 {
namespace stream {

// ------------------------------------------------------------------------------------------------ launch constants
constexpr int kThreads = 256;                          // four wave64s: the reductions below are written for exactly this
constexpr int kUnitsPerBlock = 4 * kThreads;           // B = ceil(units / this), at most kMaxChunks
constexpr int kMaxChunks = 128;
constexpr int kMaxGrid = 1 << 16;                      // work items beyond this are taken in a workgroup-stride loop

// ------------------------------------------------------------------------------------------------ device: accesses
// V neighbouring floats: one 16-byte access (VEC, V == 4, p 16-byte aligned) or V 4-byte ones -- the same values in the same order
template <int V, bool VEC>
__device__ __forceinline__ void load(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (VEC) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = p[k];
  }
}

template <int V, bool VEC>
__device__ __forceinline__ void store(float* __restrict__ p, const float (&v)[V]) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) p[k] = v[k];
  }
}

__device__ __forceinline__ bool finite_1e9(float x) { return fabsf(x) <= 1e9f; }      // false for NaN and +-Inf

// ------------------------------------------------------------------------------------------------ device: reductions
// the wave's value in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// One block-level reduction of two doubles; result valid in thread 0.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds /* [2*4] */) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { lds[wid] = a; lds[4 + wid] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = lds[0] + lds[1] + lds[2] + lds[3];
    b = lds[4] + lds[5] + lds[6] + lds[7];
  }
}

// the largest v of the workgroup's 256 threads, to every thread; lds[4].  0 is the identity here: the callers' values are never negative.
__device__ __forceinline__ float block_max(float v, float* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const float m = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
  __syncthreads();                                           // the next reduction of this workgroup writes lds again
  return m;
}

// bit k of MAXMASK: column k of a row is reduced by max, not by sum
template <unsigned MAXMASK>
__device__ __forceinline__ bool is_max(int k) { return (MAXMASK >> k & 1u) != 0; }

// The tail of a chunk: every thread's row[K] -> the workgroup's row dst[K]: wave64 shuffle tree, then the four waves in order.
template <int K, unsigned MAXMASK>
__device__ __forceinline__ void reduce_row(const double (&row)[K], double (*lds)[K], double* __restrict__ dst) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = is_max<MAXMASK>(k) ? wave_max(row[k]) : wave_sum(row[k]);
    if (lane == 0) lds[wid][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    const double v = is_max<MAXMASK>(k) ? fmax(fmax(lds[0][k], lds[1][k]), fmax(lds[2][k], lds[3][k]))
                                        : ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
    dst[k] = v;
  }
  __syncthreads();                                           // the next work item of this workgroup writes lds again
}

// The plain finalise, one workgroup: partial [groups][N][B][K] -> results [groups][N + 1][K].  A thread per (group, sample, column) adds
// that sample's B partial rows in index order (eight loads in flight at a time); then a thread per (group, column) adds the sample rows
// in sample order into row N.  A group at or beyond groups_run was not run: its partial rows are not read and its rows are zeros.
template <int K, unsigned MAXMASK>
__device__ __forceinline__ void finalize_rows(const double* partial, double* results, int groups, int N, int B, int groups_run) {
  const long long cells = (long long)groups * N * K;
  for (long long c = threadIdx.x; c < cells; c += kThreads) {
    const long long gn = c / K;                              // g * N + n
    const int k = (int)(c % K);
    const long long g = groups == 1 ? 0 : gn / N, n = gn - g * N;
    double v = 0.0;
    if (g < groups_run) {
      const double* __restrict__ p = partial + (size_t)gn * B * K + k;
#pragma unroll 8
      for (int b = 0; b < B; ++b) v = is_max<MAXMASK>(k) ? fmax(v, p[(size_t)b * K]) : v + p[(size_t)b * K];
    }
    results[((size_t)g * (N + 1) + n) * K + k] = v;
  }
  __threadfence_block();                                     // the sample rows, written by other threads of this workgroup, are read below
  __syncthreads();
  if ((int)threadIdx.x < groups * K) {
    const int g = threadIdx.x / K, k = threadIdx.x % K;
    const double* p = results + (size_t)g * (N + 1) * K + k;
    double total = 0.0;
#pragma unroll 8
    for (long long n = 0; n < N; ++n) total = is_max<MAXMASK>(k) ? fmax(total, p[(size_t)n * K]) : total + p[(size_t)n * K];
    results[((size_t)g * (N + 1) + N) * K + k] = total;
  }
}

// ------------------------------------------------------------------------------------------------ device: FlowWarp's bilinear taps
// the four taps of a plane [H][W] around a point: corners, offsets into the plane and weights
struct BilinearTaps {
  int ixL, iyT, ixR, iyB;
  int oTL, oTR, oBL, oBR;                                    // exact in int: every shape check keeps a plane below 2^30 elements
  float wTL, wTR, wBL, wBR;
};

// (x, y) has passed the inside test: 0 <= x < W, so the conversion is defined; the min keeps the index inside where float(W) rounds up
// (W above 2^24).  The caller applies the taps to its own planes as ((wTL * TL + wTR * TR) + wBL * BL) + wBR * BR, in its own file.
__device__ __forceinline__ BilinearTaps bilinear_taps(float x, float y, int W, int H) {
#pragma clang fp contract(off)
  BilinearTaps t;
  t.ixL = min((int)x, W - 1); t.iyT = min((int)y, H - 1);
  t.ixR = min(t.ixL + 1, W - 1); t.iyB = min(t.iyT + 1, H - 1);
  const float al = x - (float)t.ixL, be = y - (float)t.iyT;
  t.wTL = (1.f - al) * (1.f - be); t.wTR = al * (1.f - be); t.wBL = (1.f - al) * be; t.wBR = al * be;
  t.oTL = t.iyT * W + t.ixL; t.oTR = t.iyT * W + t.ixR; t.oBL = t.iyB * W + t.ixL; t.oBR = t.iyB * W + t.ixR;
  return t;
}

// ------------------------------------------------------------------------------------------------ host
// B, the workgroups a sample (or a direction of one) is cut into: from its units alone, never from the batch
inline int chunks(long long units) {
  const long long b = (units + kUnitsPerBlock - 1) / kUnitsPerBlock;
  return (int)(b < 1 ? 1 : b > kMaxChunks ? kMaxChunks : b);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }      // NULL (absent) counts as aligned

inline dim3 grid_for(long long items) { return dim3((unsigned)(items < kMaxGrid ? items : kMaxGrid)); }

// N blobs of `planes` planes [H][W], every extent >= 1: refuses 2^31 elements or more (and a plane of 2^30 or more) under the caller's
// name.  In steps, so that no product wraps: H W < 2^62; then H W < 2^30 and planes < 2^31 give planes H W < 2^61; then planes H W < 2^31
// and N < 2^31 give N planes H W < 2^62.
inline int check_planes(const char* what, int N, int planes, int H, int W) {
  const long long hw = (long long)H * W, lim = 1LL << 31;
  if (hw >= (lim >> 1) || planes * hw >= lim || (long long)N * (planes * hw) >= lim)
    return fail(FN2_ERR_INVALID_ARG, "%s: blob [%d,%d,%d,%d] of 2^31 elements or more", what, N, planes, H, W);
  return FN2_OK;
}

}  // namespace stream
}  // namespace fn2
