// Forward warping (splatting) for gfx950: every source pixel of a map [N,C,H,W] is carried along t * flow and spread over the four cells
// around its landing point -- summation, average, linear and softmax splatting -- with its backward.
//
// The scatter is inverted, as in flow_warp.hip's image gradient (which is this operation with importance NONE, normalize 0, t = 1):
//   1. flow_splat_link    a thread per source: its status byte, and every SPLATTED source hangs itself on the list of its top-left tap's
//                         cell -- ONE int atomicExch per source on a head array, the only atomic of the file;
//   2. flow_splat_gather  a thread per (cell, group of up to 8 channels) collects the sources on the lists of its own cell and of the cells
//                         left / above / above-left (a source whose top-left tap is there reaches this cell with another tap), adds them
//                         in ASCENDING SOURCE INDEX and writes out / weight / hole with plain stores.  Up to kFsListMax candidates are
//                         sorted in LDS; a cell that more sources meet on (a sink of the flow) is served by selection passes over the
//                         same lists: each pass takes the smallest index greater than the last one taken.  That is the same order, so
//                         the bits never depend on how the atomics of pass 1 were served; quadratic, but at sinks only.
//                         Channel group 0 also keeps the sample's row: a work item is (sample, channel group, chunk), B chunks per sample
//                         from H * W alone, a thread takes the cells chunk * 256 + thread, then every B * 256 further on;
//   3. flow_splat_final   the shared one-workgroup finalise.
//   flow_splat_bwd        a thread per source reads its four tap cells: a gather already, nothing is scattered.
// Every operation is rounded on its own (fp contract off) but the accumulation num = fmaf(value, ws, num), which is written as an fmaf
// because flow_warp.hip's gather compiles to one: include/flownet2_hip_flow_splat.h states the arithmetic and the order.
//
// Reads stay inside the sample: a tap index is formed only after the finite tests and the inside test, from a coordinate in
// [0, W) x [0, H), clamped to W - 1 and H - 1; list entries are pixel indices of the same sample written by pass 1.
#include "stream_reduce.hpp"
#include "../../include/flownet2_hip_flow_splat.h"

#pragma clang fp contract(off)

namespace fn2 {

using namespace stream;

constexpr int kFsK = FN2_FLOW_SPLAT_K;
constexpr unsigned kFsMaxMask = 1u << FN2_FLOW_SPLAT_WEIGHT_MAX;      // the column reduced by max
constexpr int kFsListMax = 16;        // candidates sorted in LDS per cell; beyond: selection passes
constexpr int kFsChPerThread = 8;

struct FsArgs {
  const float* values;
  const float* flow;
  const float* metric;
  const float* src_valid;
  float* out;
  float* weight;
  float* hole;
  unsigned char* status;       // the caller's plane, or the workspace's: never NULL
  int* head;                   // [N][H W], pre-set to -1
  int* next;                   // [N][H W]
  double* partial;             // [N][B][K]
  double* results;             // [N + 1][K]
  int N, C, H, W;
  int chunks;                  // B
  int cgroups;
  float t, fill;
  int importance, normalize;
};

struct FsSource {
  float e, al, be;
  BilinearTaps taps;
};

// Steps 1 - 6 of the header for source sp of sample n.  s is filled only where the status is SPLATTED.
__device__ __forceinline__ int fs_classify(const float* __restrict__ flow, const float* __restrict__ metric,
                                           const float* __restrict__ src_valid, size_t n, unsigned sp, int H, int W, float t,
                                           int importance, FsSource& s) {
  const size_t hw = (size_t)H * W;
  if (src_valid && src_valid[n * hw + sp] == 0.f) return FN2_FLOW_SPLAT_STATUS_MASKED;
  const float u = flow[2 * n * hw + sp], v = flow[(2 * n + 1) * hw + sp];
  if (!finite_1e9(u) || !finite_1e9(v)) return FN2_FLOW_SPLAT_STATUS_NONFINITE;
  float e = 1.f;
  if (importance != FN2_FLOW_SPLAT_IMPORTANCE_NONE) {
    const float z = metric[n * hw + sp];
    if (!finite_1e9(z)) return FN2_FLOW_SPLAT_STATUS_NONFINITE;
    if (importance == FN2_FLOW_SPLAT_IMPORTANCE_LINEAR) {
      if (z < 0.f) return FN2_FLOW_SPLAT_STATUS_NONFINITE;
      e = z;
    } else {
      e = expf(z);
      if (e == __builtin_inff()) return FN2_FLOW_SPLAT_STATUS_NONFINITE;
    }
  }
  const int y = (int)(sp / (unsigned)W), x = (int)(sp - (unsigned)y * W);
  const float x2 = (float)x + t * u, y2 = (float)y + t * v;
  if (!(x2 >= 0.f && y2 >= 0.f && x2 < (float)W && y2 < (float)H)) return FN2_FLOW_SPLAT_STATUS_OUTSIDE;
  s.taps = bilinear_taps(x2, y2, W, H);
  s.al = x2 - (float)s.taps.ixL;
  s.be = y2 - (float)s.taps.iyT;
  s.e = e;
  return FN2_FLOW_SPLAT_STATUS_SPLATTED;
}

// grid: (pixel blocks of 256, n)
__global__ void __launch_bounds__(kThreads) flow_splat_link(FsArgs a) {
  const unsigned wh = (unsigned)a.H * a.W;
  const unsigned pix = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (pix >= wh) return;
  for (unsigned n = blockIdx.y; n < (unsigned)a.N; n += gridDim.y) {
    FsSource s;
    const int st = fs_classify(a.flow, a.metric, a.src_valid, n, pix, a.H, a.W, a.t, a.importance, s);
    a.status[(size_t)n * wh + pix] = (unsigned char)st;
    if (st == FN2_FLOW_SPLAT_STATUS_SPLATTED) a.next[(size_t)n * wh + pix] = atomicExch(a.head + (size_t)n * wh + s.taps.oTL, (int)pix);
  }
}

struct FsCell {
  float num[kFsChPerThread];
  float den;
};

// source sp (on one of the four lists, so SPLATTED: src_valid is not asked again) adds itself to cell pix, channels [c0, c1)
__device__ __forceinline__ void fs_add(const FsArgs& a, size_t n, unsigned sp, unsigned pix, int c0, int c1, FsCell& cell) {
  const size_t hw = (size_t)a.H * a.W;
  FsSource s;
  if (fs_classify(a.flow, a.metric, nullptr, n, sp, a.H, a.W, a.t, a.importance, s) != FN2_FLOW_SPLAT_STATUS_SPLATTED) return;
  const int o[4] = {s.taps.oTL, s.taps.oTR, s.taps.oBL, s.taps.oBR};
  const float wk[4] = {s.taps.wTL, s.taps.wTR, s.taps.wBL, s.taps.wBR};
  float w = 0.f;                         // taps of this source that land on this cell, TL..BR order
  int hits = 0;
  bool zero = false;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (o[k] == (int)pix) { w += wk[k]; ++hits; zero |= wk[k] == 0.f; }
  // a clamped right / bottom tap of weight 0 that coincides with a weighted one: a product of its own, as in warp_bwd_gather
  const bool zero_term = hits > 1 && zero;
  const float ws = a.importance == FN2_FLOW_SPLAT_IMPORTANCE_NONE ? w : w * s.e;
  const float* __restrict__ vsrc = a.values + (n * a.C + c0) * hw + sp;
#pragma unroll
  for (int j = 0; j < kFsChPerThread; ++j)
    if (c0 + j < c1) {
      const float v = vsrc[(size_t)j * hw];
      cell.num[j] = fmaf(v, ws, cell.num[j]);              // ONE rounding, stated in the header: what warp_bwd_gather compiles to
      if (zero_term) cell.num[j] = fmaf(v, 0.f, cell.num[j]);
    }
  cell.den += ws;
}

__global__ void __launch_bounds__(kThreads) flow_splat_gather(FsArgs a) {
  __shared__ int srcs[kFsListMax][kThreads];
  __shared__ double lds[4][kFsK];
  const int W = a.W, H = a.H, tid = threadIdx.x;
  const unsigned wh = (unsigned)H * W;
  const long long items = (long long)a.N * a.cgroups * a.chunks;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int chunk = (int)(it % a.chunks);
    const long long gn = it / a.chunks;
    const int cg = (int)(gn % a.cgroups);
    const size_t n = (size_t)(gn / a.cgroups);
    const int c0 = cg * kFsChPerThread, c1 = min(a.C, c0 + kFsChPerThread);
    const int* __restrict__ hd = a.head + n * wh;
    const int* __restrict__ nx = a.next + n * wh;
    int cnt_status[4] = {0, 0, 0, 0};
    int holes = 0, pixels = 0;
    double wsum = 0.0;
    float wmax = 0.f;
    for (unsigned pix = (unsigned)chunk * kThreads + tid; pix < wh; pix += (unsigned)a.chunks * kThreads) {
      const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * W);
      FsCell cell;
#pragma unroll
      for (int j = 0; j < kFsChPerThread; ++j) cell.num[j] = 0.f;
      cell.den = 0.f;
      // the candidates: lists of the cells (y, x), (y, x-1), (y-1, x), (y-1, x-1), walked side by side (one latency per list LEVEL)
      int hd4[4], e[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int cy = y - (d >> 1), cx = x - (d & 1);
        hd4[d] = (cy < 0 || cx < 0) ? -1 : hd[(unsigned)cy * W + cx];
        e[d] = hd4[d];
      }
      int cnt = 0;
      bool overflow = false;
      while (!overflow && (e[0] >= 0 || e[1] >= 0 || e[2] >= 0 || e[3] >= 0)) {
        int nxt[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) nxt[d] = e[d] >= 0 ? nx[e[d]] : -1;
#pragma unroll
        for (int d = 0; d < 4; ++d)
          if (e[d] >= 0) {
            if (cnt < kFsListMax) srcs[cnt][tid] = e[d]; else overflow = true;
            ++cnt;
          }
#pragma unroll
        for (int d = 0; d < 4; ++d) e[d] = nxt[d];
      }
      if (!overflow) {
        for (int i = 1; i < cnt; ++i) {                  // insertion sort, ascending source index
          const int v = srcs[i][tid];
          int j = i - 1;
          while (j >= 0 && srcs[j][tid] > v) { srcs[j + 1][tid] = srcs[j][tid]; --j; }
          srcs[j + 1][tid] = v;
        }
        for (int i = 0; i < cnt; ++i) fs_add(a, n, (unsigned)srcs[i][tid], pix, c0, c1, cell);
      } else {
        // a sink: selection passes, each takes the smallest index greater than the last one taken -- the same ascending order
        int last = -1;
        for (;;) {
          int best = 0x7fffffff;
#pragma unroll
          for (int d = 0; d < 4; ++d)
            for (int q = hd4[d]; q >= 0; q = nx[q])
              if (q > last && q < best) best = q;
          if (best == 0x7fffffff) break;
          fs_add(a, n, (unsigned)best, pix, c0, c1, cell);
          last = best;
        }
      }
      const bool filled = cell.den > 0.f;
      if (a.out) {
        float* __restrict__ dst = a.out + (n * a.C + c0) * wh + pix;
#pragma unroll
        for (int j = 0; j < kFsChPerThread; ++j)
          if (c0 + j < c1) dst[(size_t)j * wh] = !a.normalize ? cell.num[j] : filled ? cell.num[j] / cell.den : a.fill;
      }
      if (cg == 0) {
        const bool is_hole = cell.den == 0.f;
        if (a.weight) a.weight[n * wh + pix] = cell.den;
        if (a.hole) a.hole[n * wh + pix] = is_hole ? 1.f : 0.f;
        const unsigned st = a.status[n * wh + pix];
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt_status[k] += st == (unsigned)k ? 1 : 0;
        pixels += 1;
        holes += is_hole ? 1 : 0;
        if (cell.den == cell.den) {
          wsum += (double)cell.den;
          wmax = fmaxf(wmax, cell.den);
        }
      }
    }
    if (cg == 0) {
      double row[kFsK];
      row[FN2_FLOW_SPLAT_PIXELS] = (double)pixels;
      row[FN2_FLOW_SPLAT_MASKED] = (double)cnt_status[FN2_FLOW_SPLAT_STATUS_MASKED];
      row[FN2_FLOW_SPLAT_NONFINITE] = (double)cnt_status[FN2_FLOW_SPLAT_STATUS_NONFINITE];
      row[FN2_FLOW_SPLAT_OUTSIDE] = (double)cnt_status[FN2_FLOW_SPLAT_STATUS_OUTSIDE];
      row[FN2_FLOW_SPLAT_SPLATTED] = (double)cnt_status[FN2_FLOW_SPLAT_STATUS_SPLATTED];
      row[FN2_FLOW_SPLAT_HOLES] = (double)holes;
      row[FN2_FLOW_SPLAT_WEIGHT_SUM] = wsum;
      row[FN2_FLOW_SPLAT_WEIGHT_MAX] = (double)wmax;
      reduce_row<kFsK, kFsMaxMask>(row, lds, a.partial + (n * a.chunks + chunk) * kFsK);
    }
  }
}

// One workgroup.
__global__ void __launch_bounds__(kThreads) flow_splat_final(FsArgs a) {
  finalize_rows<kFsK, kFsMaxMask>(a.partial, a.results, 1, a.N, a.chunks, 1);
}

struct FsBwdArgs {
  const float* out_diff;
  const float* weight_diff;
  const float* values;
  const float* flow;
  const float* metric;
  const float* src_valid;
  const float* out;
  const float* weight;
  float* values_diff;
  float* flow_diff;
  float* metric_diff;
  int N, C, H, W;
  float t;
  int importance, normalize;
};

// grid: (pixel blocks of 256, n); a thread per source pixel
__global__ void __launch_bounds__(kThreads) flow_splat_bwd(FsBwdArgs a) {
  const unsigned wh = (unsigned)a.H * a.W;
  const unsigned pix = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (pix >= wh) return;
  const int C = a.C;
  const bool none = a.importance == FN2_FLOW_SPLAT_IMPORTANCE_NONE;
  for (size_t n = blockIdx.y; n < (size_t)a.N; n += gridDim.y) {
    FsSource s;
    const int st = fs_classify(a.flow, a.metric, a.src_valid, n, pix, a.H, a.W, a.t, a.importance, s);
    if (st != FN2_FLOW_SPLAT_STATUS_SPLATTED) {
      if (a.values_diff)
        for (int c = 0; c < C; ++c) a.values_diff[(n * C + c) * wh + pix] = 0.f;
      if (a.flow_diff) { a.flow_diff[2 * n * wh + pix] = 0.f; a.flow_diff[(2 * n + 1) * wh + pix] = 0.f; }
      if (a.metric_diff) a.metric_diff[n * wh + pix] = 0.f;
      continue;
    }
    const int o[4] = {s.taps.oTL, s.taps.oTR, s.taps.oBL, s.taps.oBR};
    const float wk[4] = {s.taps.wTL, s.taps.wTR, s.taps.wBL, s.taps.wBR};
    float den[4], gd[4], A[4];
    bool pos[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      den[k] = a.weight[n * wh + o[k]];
      pos[k] = den[k] > 0.f;
      gd[k] = 0.f;
      A[k] = 0.f;
    }
    const float* __restrict__ g = a.out_diff + n * C * wh;
    if (a.normalize) {
      const float* __restrict__ op = a.out + n * C * wh;
      float sgo[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) sgo[k] += g[(size_t)c * wh + o[k]] * op[(size_t)c * wh + o[k]];
#pragma unroll
      for (int k = 0; k < 4; ++k) gd[k] = pos[k] ? -sgo[k] / den[k] : 0.f;
    }
    if (a.weight_diff)
#pragma unroll
      for (int k = 0; k < 4; ++k) gd[k] += a.weight_diff[n * wh + o[k]];
    for (int c = 0; c < C; ++c) {
      const float v = a.values[(n * C + c) * wh + pix];
      float sv = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gk = g[(size_t)c * wh + o[k]];
        const float gn = !a.normalize ? gk : pos[k] ? gk / den[k] : 0.f;
        A[k] += gn * v;
        sv += wk[k] * gn;
      }
      if (a.values_diff) a.values_diff[(n * C + c) * wh + pix] = none ? sv : s.e * sv;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) A[k] = A[k] + gd[k];
    if (a.metric_diff) {
      float de = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) de += wk[k] * A[k];
      a.metric_diff[n * wh + pix] = none ? 0.f : a.importance == FN2_FLOW_SPLAT_IMPORTANCE_LINEAR ? de : de * s.e;
    }
    if (a.flow_diff) {
      const float mal = 1.f - s.al, mbe = 1.f - s.be;
      // x: TL, TR, BL, BR; y: TL, BL, TR, BR -- a clamped pair that shares a cell (equal A) cancels exactly in either
      float dx = 0.f, dy = 0.f;
      dx += A[0] * -mbe; dx += A[1] * mbe; dx += A[2] * -s.be; dx += A[3] * s.be;
      dy += A[0] * -mal; dy += A[2] * mal; dy += A[1] * -s.al; dy += A[3] * s.al;
      if (!none) { dx = s.e * dx; dy = s.e * dy; }
      a.flow_diff[2 * n * wh + pix] = a.t * dx;
      a.flow_diff[(2 * n + 1) * wh + pix] = a.t * dy;
    }
  }
}

static int fs_shape(const char* what, int N, int C, int H, int W) {
  if (N < 1 || C < 1 || H < 1 || W < 1) return fail(FN2_ERR_INVALID_ARG, "%s: bad shape [%d,%d,%d,%d]", what, N, C, H, W);
  return check_planes(what, N, C < 2 ? 2 : C, H, W);
}

// partial rows (doubles) first, then the list heads, the links and a status plane
static size_t fs_partial_bytes(int N, int H, int W) { return sizeof(double) * kFsK * (size_t)N * chunks((long long)H * W); }
static size_t fs_ws_bytes(int N, int H, int W) {
  const size_t nhw = (size_t)N * H * W;
  return fs_partial_bytes(N, H, W) + 2 * sizeof(int) * nhw + nhw;
}

static int fs_enums(const char* what, float t, int importance, int normalize, const float* metric) {
  if (!(fabsf(t) <= 3.4028234663852886e38f)) return fail(FN2_ERR_INVALID_ARG, "%s: t = %g is not finite", what, t);
  if (importance != FN2_FLOW_SPLAT_IMPORTANCE_NONE && importance != FN2_FLOW_SPLAT_IMPORTANCE_LINEAR &&
      importance != FN2_FLOW_SPLAT_IMPORTANCE_SOFTMAX)
    return fail(FN2_ERR_INVALID_ARG, "%s: importance = %d (NONE 0, LINEAR 1, SOFTMAX 2)", what, importance);
  if (normalize != 0 && normalize != 1) return fail(FN2_ERR_INVALID_ARG, "%s: normalize = %d (0 or 1)", what, normalize);
  if (importance != FN2_FLOW_SPLAT_IMPORTANCE_NONE && !metric)
    return fail(FN2_ERR_INVALID_ARG, "%s: metric == NULL with an importance other than NONE", what);
  return FN2_OK;
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_flow_splat_sizes(int N, int C, int H, int W, size_t* workspace_bytes, int* K) {
  int rc = fs_shape("flow_splat_sizes", N, C, H, W);
  if (rc) return rc;
  if (workspace_bytes) *workspace_bytes = fs_ws_bytes(N, H, W);
  if (K) *K = kFsK;
  return FN2_OK;
}

FN2_API int fn2_flow_splat_forward(const float* values, const float* flow, const float* metric, const float* src_valid, int N, int C, int H,
                                   int W, float t, int importance, int normalize, int fill, double* results, float* out, float* weight,
                                   float* hole, unsigned char* status, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "flow_splat_forward";
  if (!values) return fail(FN2_ERR_INVALID_ARG, "%s: values == NULL", what);
  if (!flow) return fail(FN2_ERR_INVALID_ARG, "%s: flow == NULL", what);
  if (!results) return fail(FN2_ERR_INVALID_ARG, "%s: results == NULL", what);
  int rc = fs_shape(what, N, C, H, W);
  if (rc) return rc;
  rc = fs_enums(what, t, importance, normalize, metric);
  if (rc) return rc;
  if (fill != FN2_FILL_ZERO && fill != FN2_FILL_NAN) return fail(FN2_ERR_INVALID_ARG, "%s: fill must be ZERO(1) or NOT_A_NUMBER(2)", what);
  if (!workspace || workspace_bytes < fs_ws_bytes(N, H, W))
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, fs_ws_bytes(N, H, W));
  const size_t nhw = (size_t)N * H * W;
  FsArgs a;
  a.values = values; a.flow = flow; a.metric = metric; a.src_valid = src_valid;
  a.out = out; a.weight = weight; a.hole = hole;
  a.partial = reinterpret_cast<double*>(workspace);
  a.head = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + fs_partial_bytes(N, H, W));
  a.next = a.head + nhw;
  a.status = status ? status : reinterpret_cast<unsigned char*>(a.next + nhw);
  a.results = results;
  a.N = N; a.C = C; a.H = H; a.W = W;
  a.chunks = chunks((long long)H * W);
  a.cgroups = (C + kFsChPerThread - 1) / kFsChPerThread;
  a.t = t;
  a.fill = fill == FN2_FILL_ZERO ? 0.f : __builtin_bit_cast(float, 0xFFE00000u);      // FlowWarp's NaN
  a.importance = importance; a.normalize = normalize;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(a.head, 0xff, sizeof(int) * nhw, st) != hipSuccess)                 // every list empty (-1)
    return fail(FN2_ERR_LAUNCH, "%s: hipMemsetAsync failed", what);
  const unsigned bx = (unsigned)(((size_t)H * W + kThreads - 1) / kThreads);
  const unsigned ny = (unsigned)(N < 65535 ? N : 65535);
  hipLaunchKernelGGL(flow_splat_link, dim3(bx, ny), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(flow_splat_gather, grid_for((long long)N * a.cgroups * a.chunks), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(flow_splat_final, dim3(1), dim3(kThreads), 0, st, a);
  return check_launch(what);
}

FN2_API int fn2_flow_splat_backward(const float* out_diff, const float* weight_diff, const float* values, const float* flow,
                                    const float* metric, const float* src_valid, const float* out, const float* weight, int N, int C, int H,
                                    int W, float t, int importance, int normalize, float* values_diff, float* flow_diff, float* metric_diff,
                                    void* stream) {
  const char* what = "flow_splat_backward";
  if (!out_diff) return fail(FN2_ERR_INVALID_ARG, "%s: out_diff == NULL", what);
  if (!values) return fail(FN2_ERR_INVALID_ARG, "%s: values == NULL", what);
  if (!flow) return fail(FN2_ERR_INVALID_ARG, "%s: flow == NULL", what);
  if (!weight) return fail(FN2_ERR_INVALID_ARG, "%s: weight == NULL", what);
  int rc = fs_shape(what, N, C, H, W);
  if (rc) return rc;
  rc = fs_enums(what, t, importance, normalize, metric);
  if (rc) return rc;
  if (normalize && !out) return fail(FN2_ERR_INVALID_ARG, "%s: out == NULL with normalize == 1", what);
  if (metric_diff && importance == FN2_FLOW_SPLAT_IMPORTANCE_NONE)
    return fail(FN2_ERR_INVALID_ARG, "%s: metric_diff asked for with importance NONE", what);
  FsBwdArgs a;
  a.out_diff = out_diff; a.weight_diff = weight_diff; a.values = values; a.flow = flow; a.metric = metric; a.src_valid = src_valid;
  a.out = out; a.weight = weight;
  a.values_diff = values_diff; a.flow_diff = flow_diff; a.metric_diff = metric_diff;
  a.N = N; a.C = C; a.H = H; a.W = W;
  a.t = t; a.importance = importance; a.normalize = normalize;
  const unsigned bx = (unsigned)(((size_t)H * W + kThreads - 1) / kThreads);
  const unsigned ny = (unsigned)(N < 65535 ? N : 65535);
  hipLaunchKernelGGL(flow_splat_bwd, dim3(bx, ny), dim3(kThreads), 0, as_stream(stream), a);
  return check_launch(what);
}
