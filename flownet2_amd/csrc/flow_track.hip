// Dense point trajectories for gfx950: points carried through T frames of forward / backward flow [N,T,2,H,W] in ONE gather launch, with
// per-sample counts, step and displacement sums in fp64 from a one-workgroup finalise; and the reseeding of lost coverage.
//
// Trajectories do not depend on each other, so a thread owns one point and runs the T loop itself: per frame it gathers the eight taps of
// the forward flow at its position, looks at the stop byte, gathers the eight taps of the backward flow at its target, applies the
// consistency test of flow_consistency.hip and moves.  Nothing but the trajectory (if asked for) is written per frame, and the stores of a
// frame's x and y planes are coalesced across the wave, as the reads of the points are.  The counts stay in registers; then, as in
// flow_consistency.hip: wave64 reduction -> LDS -> one fp64 partial row per workgroup, and a finalise that adds a sample's partial rows in
// index order and the sample rows in sample order.  No atomics on floats, nothing read back by the host.
//
// A work item is (sample, chunk), B chunks per sample, B from P alone: a sample's row has the same bits alone and in any batch.  Every
// access is a 4-byte or a 1-byte one, so no pointer needs more than its type's alignment.  Every operation is rounded on its own (fp
// contract off): include/flownet2_hip_flow_track.h states the arithmetic.
//
// Reads stay inside the sample: tap and stop indices are formed only from a position that has passed the finite test and the inside test,
// so from a coordinate in [0, W) x [0, H), and are clamped to W - 1 and H - 1.
#include "stream_reduce.hpp"
#include "../../include/flownet2_hip_flow_track.h"

#pragma clang fp contract(off)

namespace fn2 {

using namespace stream;

constexpr int kFtK = FN2_FLOW_TRACK_K;
constexpr unsigned kFtMaxMask = 1u << FN2_FLOW_TRACK_STEPS_MAX | 1u << FN2_FLOW_TRACK_DISP_MAX;      // the columns reduced by max
constexpr unsigned kFtNonfinite = FN2_FLOW_TRACK_STOP_NONFINITE, kFtOutside = FN2_FLOW_TRACK_STOP_OUTSIDE,
                   kFtInconsistent = FN2_FLOW_TRACK_STOP_INCONSISTENT, kFtMarked = FN2_FLOW_TRACK_STOP_MARKED;

struct FtArgs {
  const float* fw;
  const float* bw;
  const unsigned char* stop;
  const float* points;
  const unsigned char* state_in;
  float* tracks;
  float* points_out;
  unsigned char* state_out;
  int* steps;
  double* partial;             // [N][B][K]
  double* results;             // [N + 1][K]
  int N, T, H, W, P;
  int chunks;                  // B
  unsigned stop_mask;
  float alpha1, alpha2;
};

__device__ __forceinline__ bool ft_inside(float x, float y, int W, int H) { return x >= 0.f && y >= 0.f && x < (float)W && y < (float)H; }

// The bilinear value of the planes pu / pv at (x, y), which has passed ft_inside: FlowWarp's taps in the association of
// flow_consistency.hip.
__device__ __forceinline__ void ft_sample(const float* __restrict__ pu, const float* __restrict__ pv, int W, int H, float x, float y, float& u,
                                          float& v) {
  const BilinearTaps t = bilinear_taps(x, y, W, H);
  u = ((t.wTL * pu[t.oTL] + t.wTR * pu[t.oTR]) + t.wBL * pu[t.oBL]) + t.wBR * pu[t.oBR];
  v = ((t.wTL * pv[t.oTL] + t.wTR * pv[t.oTR]) + t.wBL * pv[t.oBL]) + t.wBR * pv[t.oBR];
}

// One frame step of an alive point at (x, y) inside the plane: 0 and the new position, or the reason it stops (x, y unchanged).
__device__ __forceinline__ unsigned ft_step(const FtArgs& a, const float* __restrict__ f, const float* __restrict__ b,
                                            const unsigned char* __restrict__ s, float& x, float& y) {
  const int W = a.W, H = a.H;
  const size_t hw = (size_t)H * W;
  float au, av;
  ft_sample(f, f + hw, W, H, x, y, au, av);
  if (!finite_1e9(au) || !finite_1e9(av)) return kFtNonfinite;
  if (s) {
    const int jx = min((int)(x + 0.5f), W - 1), jy = min((int)(y + 0.5f), H - 1);      // x + 0.5f <= W, as x < W
    if ((unsigned)s[(size_t)jy * W + jx] & a.stop_mask) return kFtMarked;
  }
  const float x2 = x + au, y2 = y + av;
  if (!ft_inside(x2, y2, W, H)) return kFtOutside;
  float bu, bv;
  ft_sample(b, b + hw, W, H, x2, y2, bu, bv);
  if (!finite_1e9(bu) || !finite_1e9(bv)) return kFtNonfinite;
  const float su = au + bu, sv = av + bv;
  const float sq = su * su + sv * sv;
  const float m = (au * au + av * av) + (bu * bu + bv * bv);
  if (sq > a.alpha1 * m + a.alpha2) return kFtInconsistent;
  x = x2;
  y = y2;
  return 0u;
}

// what one thread has seen; counts stay integers until the reduction (a thread sees fewer than 2^31 points, and steps sum below 2^31:
// a thread's points times T is at most N (T + 1) 2 P)
struct FtAcc {
  double disp;
  int points, alive, nonfinite, outside, inconsistent, marked, steps, smax;
  float dmax;
};

// Chunk `chunk` of sample n: points chunk * 256 + thread, then every B * 256 further on.  row -> partial[(n * B + chunk) * K].
__device__ __forceinline__ void ft_chunk(const FtArgs& a, long long n, int chunk, double (*lds)[kFtK]) {
  const int T = a.T, P = a.P;
  const size_t hw = (size_t)a.H * a.W;
  const float* fw = a.fw + (size_t)n * T * 2 * hw;
  const float* bw = a.bw + (size_t)n * T * 2 * hw;
  const unsigned char* stop = a.stop ? a.stop + (size_t)n * T * hw : nullptr;
  const float* px = a.points + (size_t)n * 2 * P;
  float* tr = a.tracks ? a.tracks + (size_t)n * (T + 1) * 2 * P : nullptr;
  const float nan = __builtin_nanf("");
  FtAcc t = {};
  for (long long q = (long long)chunk * kThreads + threadIdx.x; q < P; q += (long long)a.chunks * kThreads) {
    const size_t p = (size_t)q;
    const float x0 = px[p], y0 = px[P + p];
    const unsigned given = a.state_in ? (unsigned)a.state_in[(size_t)n * P + p] : 0u;
    unsigned st = given;
    float x = x0, y = y0;
    int steps = 0;
    if (st == 0u) {
      if (!finite_1e9(x) || !finite_1e9(y)) st = kFtNonfinite;
      else if (!ft_inside(x, y, a.W, a.H)) st = kFtOutside;
    }
    if (tr) {
      tr[p] = x0;
      tr[P + p] = y0;
    }
    for (int f = 0; f < T; ++f) {
      if (st == 0u) {
        st = ft_step(a, fw + (size_t)f * 2 * hw, bw + (size_t)f * 2 * hw, stop ? stop + (size_t)f * hw : nullptr, x, y);
        steps += st == 0u ? 1 : 0;
      }
      if (tr) {
        tr[(size_t)(f + 1) * 2 * P + p] = st == 0u ? x : nan;
        tr[(size_t)(f + 1) * 2 * P + P + p] = st == 0u ? y : nan;
      }
    }
    if (a.points_out) {
      a.points_out[(size_t)n * 2 * P + p] = x;
      a.points_out[(size_t)n * 2 * P + P + p] = y;
    }
    a.state_out[(size_t)n * P + p] = (unsigned char)st;
    if (a.steps) a.steps[(size_t)n * P + p] = steps;
    t.points += 1;
    if (given == 0u) {
      t.nonfinite += st == kFtNonfinite ? 1 : 0;
      t.outside += st == kFtOutside ? 1 : 0;
      t.inconsistent += st == kFtInconsistent ? 1 : 0;
      t.marked += st == kFtMarked ? 1 : 0;
    }
    t.steps += steps;
    t.smax = max(t.smax, steps);
    if (st == 0u) {
      const float dx = x - x0, dy = y - y0;
      const float d = sqrtf(dx * dx + dy * dy);
      t.alive += 1;
      t.disp += (double)d;
      t.dmax = fmaxf(t.dmax, d);
    }
  }
  double row[kFtK];
  row[FN2_FLOW_TRACK_POINTS] = (double)t.points;
  row[FN2_FLOW_TRACK_ALIVE] = (double)t.alive;
  row[FN2_FLOW_TRACK_NONFINITE] = (double)t.nonfinite;
  row[FN2_FLOW_TRACK_OUTSIDE] = (double)t.outside;
  row[FN2_FLOW_TRACK_INCONSISTENT] = (double)t.inconsistent;
  row[FN2_FLOW_TRACK_MARKED] = (double)t.marked;
  row[FN2_FLOW_TRACK_STEPS_SUM] = (double)t.steps;
  row[FN2_FLOW_TRACK_STEPS_MAX] = (double)t.smax;
  row[FN2_FLOW_TRACK_DISP_SUM] = t.disp;
  row[FN2_FLOW_TRACK_DISP_MAX] = (double)t.dmax;
  reduce_row<kFtK, kFtMaxMask>(row, lds, a.partial + ((size_t)n * a.chunks + chunk) * kFtK);
}

__global__ void __launch_bounds__(kThreads) flow_track_gather(FtArgs a) {
  __shared__ double lds[4][kFtK];
  const long long items = (long long)a.N * a.chunks;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) ft_chunk(a, w / a.chunks, (int)(w % a.chunks), lds);
}

// One workgroup; the plain finalise with one group.
__global__ void __launch_bounds__(kThreads) flow_track_final(FtArgs a) {
  finalize_rows<kFtK, kFtMaxMask>(a.partial, a.results, 1, a.N, a.chunks, 1);
}

// ---- reseeding ------------------------------------------------------------------------------------------------------------------------
struct FrArgs {
  float* points;               // [N][2][P]
  unsigned char* state;        // [N][P]
  unsigned char* born;         // [N][P] or NULL
  unsigned char* covered;      // [N][P], the workspace
  int N, H, W, cell, cw;       // cw = ceil(W / cell)
  long long P, total;          // total = N P < 2^30
};

__global__ void __launch_bounds__(kThreads) flow_track_reseed_clear(FrArgs a) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < a.total; i += (long long)gridDim.x * kThreads) a.covered[i] = 0;
}

// every alive point inside the plane marks its cell: the same byte from every writer
__global__ void __launch_bounds__(kThreads) flow_track_reseed_cover(FrArgs a) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < a.total; i += (long long)gridDim.x * kThreads) {
    if (a.state[i] != 0) continue;
    const long long n = i / a.P, p = i - n * a.P;
    const float x = a.points[(size_t)n * 2 * a.P + p], y = a.points[(size_t)n * 2 * a.P + a.P + p];
    if (!finite_1e9(x) || !finite_1e9(y) || !ft_inside(x, y, a.W, a.H)) continue;
    const int cx = min((int)x, a.W - 1) / a.cell, cy = min((int)y, a.H - 1) / a.cell;
    a.covered[(size_t)n * a.P + (size_t)cy * a.cw + cx] = 1;
  }
}

// every slot that is not alive and whose home cell nobody covers starts anew at the cell's centre
__global__ void __launch_bounds__(kThreads) flow_track_reseed_fill(FrArgs a) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < a.total; i += (long long)gridDim.x * kThreads) {
    const bool fill = a.state[i] != 0 && a.covered[i] == 0;
    if (fill) {
      const long long n = i / a.P, p = i - n * a.P;
      const int cy = (int)(p / a.cw), cx = (int)(p - (long long)cy * a.cw);
      const float half = 0.5f * (float)(a.cell - 1);
      a.points[(size_t)n * 2 * a.P + p] = fminf((float)(cx * a.cell) + half, (float)(a.W - 1));
      a.points[(size_t)n * 2 * a.P + a.P + p] = fminf((float)(cy * a.cell) + half, (float)(a.H - 1));
      a.state[i] = 0;
    }
    if (a.born) a.born[i] = fill ? 1 : 0;
  }
}

static int ft_shape(const char* what, int N, int T, int H, int W, int P) {
  if (N < 1 || T < 1 || H < 1 || W < 1 || P < 1)
    return fail(FN2_ERR_INVALID_ARG, "%s: bad shape [%d,%d,2,%d,%d] with %d points", what, N, T, H, W, P);
  // in steps, so that no product wraps: H W < 2^62; then 2 H W < 2^31 and T < 2^31 give T 2 H W < 2^62, and so on
  const long long lim = 1LL << 31, hw = (long long)H * W;
  if (hw >= (lim >> 1) || (long long)T * (2 * hw) >= lim || (long long)N * ((long long)T * (2 * hw)) >= lim)
    return fail(FN2_ERR_INVALID_ARG, "%s: blob [%d,%d,2,%d,%d] of 2^31 elements or more", what, N, T, H, W);
  if (2LL * P >= lim || ((long long)T + 1) * (2LL * P) >= lim || (long long)N * (((long long)T + 1) * (2LL * P)) >= lim)
    return fail(FN2_ERR_INVALID_ARG, "%s: blob [%d,%d,2,%d] of 2^31 elements or more", what, N, T + 1, P);
  return FN2_OK;
}

static size_t ft_partial_bytes(int N, int P) { return sizeof(double) * kFtK * (size_t)N * chunks(P); }

static size_t ft_ws_bytes(int N, int P) {
  const size_t a = ft_partial_bytes(N, P), b = (size_t)N * P;
  return a > b ? a : b;
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_flow_track_sizes(int N, int T, int H, int W, int P, size_t* workspace_bytes, int* K) {
  int rc = ft_shape("flow_track_sizes", N, T, H, W, P);
  if (rc) return rc;
  if (workspace_bytes) *workspace_bytes = ft_ws_bytes(N, P);
  if (K) *K = kFtK;
  return FN2_OK;
}

FN2_API int fn2_flow_track(const float* fw, const float* bw, const unsigned char* stop, unsigned stop_mask, const float* points,
                           const unsigned char* state_in, int N, int T, int H, int W, int P, float alpha1, float alpha2, double* results,
                           float* tracks, float* points_out, unsigned char* state_out, int* steps, void* workspace, size_t workspace_bytes,
                           void* stream) {
  const char* what = "flow_track";
  if (!fw) return fail(FN2_ERR_INVALID_ARG, "%s: fw == NULL", what);
  if (!bw) return fail(FN2_ERR_INVALID_ARG, "%s: bw == NULL", what);
  if (!points) return fail(FN2_ERR_INVALID_ARG, "%s: points == NULL", what);
  if (!state_out) return fail(FN2_ERR_INVALID_ARG, "%s: state_out == NULL", what);
  if (!results) return fail(FN2_ERR_INVALID_ARG, "%s: results == NULL", what);
  int rc = ft_shape(what, N, T, H, W, P);
  if (rc) return rc;
  if (!(alpha1 >= 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: alpha1 = %g (need >= 0)", what, alpha1);
  if (!(alpha2 >= 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: alpha2 = %g (need >= 0)", what, alpha2);
  if (!workspace || workspace_bytes < ft_partial_bytes(N, P))
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, ft_partial_bytes(N, P));
  FtArgs a;
  a.fw = fw; a.bw = bw; a.stop = stop; a.points = points; a.state_in = state_in;
  a.tracks = tracks; a.points_out = points_out; a.state_out = state_out; a.steps = steps;
  a.partial = reinterpret_cast<double*>(workspace);
  a.results = results;
  a.N = N; a.T = T; a.H = H; a.W = W; a.P = P;
  a.chunks = chunks(P);
  a.stop_mask = stop_mask;
  a.alpha1 = alpha1; a.alpha2 = alpha2;
  const long long items = (long long)N * a.chunks;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(flow_track_gather, grid_for(items), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(flow_track_final, dim3(1), dim3(kThreads), 0, st, a);
  return check_launch(what);
}

FN2_API int fn2_flow_track_reseed(float* points, unsigned char* state, unsigned char* born, int N, int H, int W, int cell, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  const char* what = "flow_track_reseed";
  if (!points) return fail(FN2_ERR_INVALID_ARG, "%s: points == NULL", what);
  if (!state) return fail(FN2_ERR_INVALID_ARG, "%s: state == NULL", what);
  if (N < 1 || H < 1 || W < 1 || cell < 1) return fail(FN2_ERR_INVALID_ARG, "%s: bad shape N = %d, H = %d, W = %d, cell = %d", what, N, H, W, cell);
  const long long ch = ((long long)H + cell - 1) / cell, cw = ((long long)W + cell - 1) / cell, lim = 1LL << 31;
  const long long P = ch * cw;                               // < 2^62
  if (2 * P >= lim || (long long)N * (2 * P) >= lim)
    return fail(FN2_ERR_INVALID_ARG, "%s: blob [%d,2,%lld] of 2^31 elements or more", what, N, P);
  if (!workspace || workspace_bytes < (size_t)N * (size_t)P)
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, (size_t)N * (size_t)P);
  FrArgs a;
  a.points = points; a.state = state; a.born = born;
  a.covered = reinterpret_cast<unsigned char*>(workspace);
  a.N = N; a.H = H; a.W = W; a.cell = cell; a.cw = (int)cw;
  a.P = P; a.total = (long long)N * P;
  const long long blocks = (a.total + kThreads - 1) / kThreads;
  const dim3 grid = grid_for(blocks);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(flow_track_reseed_clear, grid, dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(flow_track_reseed_cover, grid, dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(flow_track_reseed_fill, grid, dim3(kThreads), 0, st, a);
  return check_launch(what);
}
