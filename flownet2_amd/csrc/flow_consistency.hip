// Forward-backward flow consistency for gfx950: the occlusion / consistency masks of a forward and a backward flow [N,2,H,W], both
// directions in ONE launch, with per-sample counts and error sums in fp64 from a one-workgroup finalise.
//
// Composed from flow_warp and eager tensor operations this is a dozen launches or more per direction, each with a temporary of the full
// map.  Here a thread streams its own flow (the pixel, and its four neighbours for the motion-boundary test), gathers the eight taps of
// the other flow at its target, decides, writes the maps asked for and keeps its counts in registers; then, as in flow_metrics.hip: wave64
// reduction -> LDS -> one fp64 partial row per workgroup, and a finalise that adds a sample's partial rows in index order and the sample
// rows in sample order.  No atomics on floats, nothing read back by the host.
//
// A work item is (direction, sample, chunk), B chunks per sample, B from H * W alone: a sample's row has the same bits alone and in any
// batch.  A thread owns one pixel per step, or four neighbouring pixels of a row where W is a multiple of 4; those are read and written
// as 16-byte accesses where every pointer given is 16-byte aligned and as 4-byte ones otherwise -- the same values in the same order.
// Every operation is rounded on its own (fp contract off): include/flownet2_hip_flow_consistency.h states the arithmetic.
//
// Reads stay inside the sample: the own-flow neighbours are clamped to the plane, and the tap indices are formed only after the finite
// test and the inside test, from a coordinate in [0, W) x [0, H), and clamped to W - 1 and H - 1.
#include "stream_reduce.hpp"
#include "../../include/flownet2_hip_flow_consistency.h"

#pragma clang fp contract(off)

namespace fn2 {

using namespace stream;

constexpr int kFcK = FN2_FLOW_CONSISTENCY_K;
constexpr unsigned kFcMaxMask = 1u << FN2_FLOW_CONSISTENCY_ERR_MAX;      // the column reduced by max
constexpr unsigned kFcNonfinite = FN2_FLOW_CONSISTENCY_FLAG_NONFINITE, kFcOutside = FN2_FLOW_CONSISTENCY_FLAG_OUTSIDE,
                   kFcInconsistent = FN2_FLOW_CONSISTENCY_FLAG_INCONSISTENT, kFcBoundary = FN2_FLOW_CONSISTENCY_FLAG_BOUNDARY;
constexpr unsigned kFcOccluded = kFcNonfinite | kFcOutside | kFcInconsistent;

struct FcArgs {
  const float* flow[2];        // fw, bw: direction d checks flow[d] against flow[1 - d]
  unsigned char* flags[2];
  float* occ[2];
  float* err[2];
  float* warped[2];
  double* partial;             // [2][N][B][K]
  double* results;             // [2][N + 1][K]
  int N, H, W;
  int chunks;                  // B
  int quad;                    // W % 4 == 0: four pixels per thread and step
  int vec;                     // and every pointer given 16-byte aligned: 16-byte loads / stores
  float alpha1, alpha2, beta1, beta2;
};

// what one thread has seen; counts stay integers until the reduction (a thread sees fewer than 2^31 pixels)
struct FcAcc {
  double err;
  int pixels, nonfinite, outside, inconsistent, occluded, boundary;
  float emax;
};

struct FcPixel {
  float err, bu, bv;
  unsigned flags;
};

// One pixel (x, y) of direction a against the planes ou / ov of the other flow of the same sample.  n[8]: the own flow's neighbours
// uL, uR, uT, uB, vL, vR, vT, vB, already clamped to the plane.
__device__ __forceinline__ FcPixel fc_pixel(const FcArgs& a, const float* __restrict__ ou, const float* __restrict__ ov, int x, int y,
                                            float au, float av, const float (&n)[8]) {
  const float nan = __builtin_nanf("");
  FcPixel p = {nan, nan, nan, 0u};
  if (!finite_1e9(au) || !finite_1e9(av)) {
    p.flags = kFcNonfinite;
    return p;
  }
  const float mag = au * au + av * av;
  bool nb = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) nb = nb && finite_1e9(n[k]);
  if (nb) {
    const float ux = 0.5f * (n[1] - n[0]), uy = 0.5f * (n[3] - n[2]);
    const float vx = 0.5f * (n[5] - n[4]), vy = 0.5f * (n[7] - n[6]);
    const float g = ((ux * ux + uy * uy) + vx * vx) + vy * vy;
    if (g > a.beta1 * mag + a.beta2) p.flags |= kFcBoundary;
  }
  const float x2 = (float)x + au, y2 = (float)y + av;
  if (!(x2 >= 0.f && y2 >= 0.f && x2 < (float)a.W && y2 < (float)a.H)) {
    p.flags |= kFcOutside;
    return p;
  }
  const BilinearTaps t = bilinear_taps(x2, y2, a.W, a.H);
  const float bu = ((t.wTL * ou[t.oTL] + t.wTR * ou[t.oTR]) + t.wBL * ou[t.oBL]) + t.wBR * ou[t.oBR];
  const float bv = ((t.wTL * ov[t.oTL] + t.wTR * ov[t.oTR]) + t.wBL * ov[t.oBL]) + t.wBR * ov[t.oBR];
  p.bu = bu;
  p.bv = bv;
  if (!finite_1e9(bu) || !finite_1e9(bv)) {
    p.flags |= kFcNonfinite;
    return p;
  }
  const float su = au + bu, sv = av + bv;
  const float s = su * su + sv * sv;
  const float m = mag + (bu * bu + bv * bv);
  if (s > a.alpha1 * m + a.alpha2) p.flags |= kFcInconsistent;
  p.err = sqrtf(s);
  return p;
}

// Chunk `chunk` of (direction d, sample n): units chunk * 256 + thread, then every B * 256 further on; a unit is V pixels of one row.
// row -> partial[((d * N + n) * B + chunk) * K].
template <int V, bool VEC>
__device__ __forceinline__ void fc_chunk(const FcArgs& a, int d, long long n, int chunk, double (*lds)[kFcK]) {
  const int W = a.W, H = a.H;
  const size_t hw = (size_t)H * W;
  const long long units = (long long)(hw / V);
  const float* __restrict__ pu_ = a.flow[d] + (size_t)n * 2 * hw;
  const float* __restrict__ pv_ = pu_ + hw;
  const float* __restrict__ ou_ = a.flow[1 - d] + (size_t)n * 2 * hw;
  const float* __restrict__ ov_ = ou_ + hw;
  FcAcc t = {};
  for (long long u = (long long)chunk * kThreads + threadIdx.x; u < units; u += (long long)a.chunks * kThreads) {
    const unsigned r = (unsigned)u * V;                                    // H W < 2^30
    const int y = (int)(r / (unsigned)W), x = (int)(r - (unsigned)y * W);  // V == 4: W % 4 == 0, so x % 4 == 0 and x + 3 < W
    const size_t rT = (size_t)max(y - 1, 0) * W + x, rB = (size_t)min(y + 1, H - 1) * W + x;
    const size_t rL = (size_t)y * W + max(x - 1, 0), rR = (size_t)y * W + min(x + V, W - 1);
    float cu[V], cv[V], tu[V], tv[V], bu[V], bv[V];
    load<V, VEC>(pu_ + r, cu);
    load<V, VEC>(pv_ + r, cv);
    load<V, VEC>(pu_ + rT, tu);
    load<V, VEC>(pv_ + rT, tv);
    load<V, VEC>(pu_ + rB, bu);
    load<V, VEC>(pv_ + rB, bv);
    const float lu = pu_[rL], lv = pv_[rL], ru = pu_[rR], rv = pv_[rR];
    float e[V], oc[V], wu[V], wv[V];
    unsigned fl[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float nb[8] = {k == 0 ? lu : cu[k > 0 ? k - 1 : 0], k == V - 1 ? ru : cu[k < V - 1 ? k + 1 : k], tu[k], bu[k],
                           k == 0 ? lv : cv[k > 0 ? k - 1 : 0], k == V - 1 ? rv : cv[k < V - 1 ? k + 1 : k], tv[k], bv[k]};
      const FcPixel p = fc_pixel(a, ou_, ov_, x + k, y, cu[k], cv[k], nb);
      const bool occluded = (p.flags & kFcOccluded) != 0;
      e[k] = p.err; wu[k] = p.bu; wv[k] = p.bv; fl[k] = p.flags;
      oc[k] = occluded ? 1.f : 0.f;
      t.pixels += 1;
      t.nonfinite += (p.flags & kFcNonfinite) ? 1 : 0;
      t.outside += (p.flags & kFcOutside) ? 1 : 0;
      t.inconsistent += (p.flags & kFcInconsistent) ? 1 : 0;
      t.boundary += (p.flags & kFcBoundary) ? 1 : 0;
      t.occluded += occluded ? 1 : 0;
      if (p.err == p.err) {
        t.err += (double)p.err;
        t.emax = fmaxf(t.emax, p.err);
      }
    }
    const size_t plane = (size_t)n * hw + r;
    if (a.flags[d]) {
      if constexpr (VEC) {
        *reinterpret_cast<unsigned*>(a.flags[d] + plane) = fl[0] | (fl[1] << 8) | (fl[2] << 16) | (fl[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) a.flags[d][plane + k] = (unsigned char)fl[k];
      }
    }
    if (a.occ[d]) store<V, VEC>(a.occ[d] + plane, oc);
    if (a.err[d]) store<V, VEC>(a.err[d] + plane, e);
    if (a.warped[d]) {
      store<V, VEC>(a.warped[d] + (size_t)n * 2 * hw + r, wu);
      store<V, VEC>(a.warped[d] + (size_t)n * 2 * hw + hw + r, wv);
    }
  }
  double row[kFcK];
  row[FN2_FLOW_CONSISTENCY_PIXELS] = (double)t.pixels;
  row[FN2_FLOW_CONSISTENCY_NONFINITE] = (double)t.nonfinite;
  row[FN2_FLOW_CONSISTENCY_OUTSIDE] = (double)t.outside;
  row[FN2_FLOW_CONSISTENCY_INCONSISTENT] = (double)t.inconsistent;
  row[FN2_FLOW_CONSISTENCY_OCCLUDED] = (double)t.occluded;
  row[FN2_FLOW_CONSISTENCY_BOUNDARY] = (double)t.boundary;
  row[FN2_FLOW_CONSISTENCY_ERR_SUM] = t.err;
  row[FN2_FLOW_CONSISTENCY_ERR_MAX] = (double)t.emax;
  reduce_row<kFcK, kFcMaxMask>(row, lds, a.partial + (((size_t)d * a.N + n) * a.chunks + chunk) * kFcK);
}

__global__ void __launch_bounds__(kThreads) flow_consistency_partial(FcArgs a) {
  __shared__ double lds[4][kFcK];
  const long long per_dir = (long long)a.N * a.chunks;
  for (long long w = blockIdx.x; w < 2 * per_dir; w += gridDim.x) {
    const int d = w >= per_dir ? 1 : 0;
    const long long i = w - d * per_dir;
    const long long n = i / a.chunks;
    const int chunk = (int)(i % a.chunks);
    if (!a.quad) fc_chunk<1, false>(a, d, n, chunk, lds);
    else if (a.vec) fc_chunk<4, true>(a, d, n, chunk, lds);
    else fc_chunk<4, false>(a, d, n, chunk, lds);
  }
}

// One workgroup; the two directions are the groups of the plain finalise.
__global__ void __launch_bounds__(kThreads) flow_consistency_final(FcArgs a) {
  finalize_rows<kFcK, kFcMaxMask>(a.partial, a.results, 2, a.N, a.chunks, 2);
}

static int fc_shape(const char* what, int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return fail(FN2_ERR_INVALID_ARG, "%s: bad shape [%d,2,%d,%d]", what, N, H, W);
  return check_planes(what, N, 2, H, W);
}

static size_t fc_ws_bytes(int N, int H, int W) { return sizeof(double) * kFcK * 2 * (size_t)N * chunks((long long)H * W); }

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_flow_consistency_sizes(int N, int H, int W, size_t* workspace_bytes, int* K) {
  int rc = fc_shape("flow_consistency_sizes", N, H, W);
  if (rc) return rc;
  if (workspace_bytes) *workspace_bytes = fc_ws_bytes(N, H, W);
  if (K) *K = kFcK;
  return FN2_OK;
}

FN2_API int fn2_flow_consistency(const float* fw, const float* bw, int N, int H, int W, float alpha1, float alpha2, float beta1, float beta2,
                                 double* results, unsigned char* flags_fw, unsigned char* flags_bw, float* occ_fw, float* occ_bw,
                                 float* err_fw, float* err_bw, float* warped_fw, float* warped_bw, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* what = "flow_consistency";
  if (!fw) return fail(FN2_ERR_INVALID_ARG, "%s: fw == NULL", what);
  if (!bw) return fail(FN2_ERR_INVALID_ARG, "%s: bw == NULL", what);
  if (!results) return fail(FN2_ERR_INVALID_ARG, "%s: results == NULL", what);
  int rc = fc_shape(what, N, H, W);
  if (rc) return rc;
  const float thr[4] = {alpha1, alpha2, beta1, beta2};
  const char* names[4] = {"alpha1", "alpha2", "beta1", "beta2"};
  for (int k = 0; k < 4; ++k)
    if (!(thr[k] >= 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: %s = %g (need >= 0)", what, names[k], thr[k]);
  if (!workspace || workspace_bytes < fc_ws_bytes(N, H, W))
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, fc_ws_bytes(N, H, W));
  FcArgs a;
  a.flow[0] = fw; a.flow[1] = bw;
  a.flags[0] = flags_fw; a.flags[1] = flags_bw;
  a.occ[0] = occ_fw; a.occ[1] = occ_bw;
  a.err[0] = err_fw; a.err[1] = err_bw;
  a.warped[0] = warped_fw; a.warped[1] = warped_bw;
  a.partial = reinterpret_cast<double*>(workspace);
  a.results = results;
  a.N = N; a.H = H; a.W = W;
  a.chunks = chunks((long long)H * W);
  a.quad = (W % 4) == 0;
  a.vec = a.quad;
  for (int d = 0; d < 2; ++d)
    a.vec = a.vec && aligned16(a.flow[d]) && aligned16(a.flags[d]) && aligned16(a.occ[d]) && aligned16(a.err[d]) &&
            aligned16(a.warped[d]);
  a.alpha1 = alpha1; a.alpha2 = alpha2; a.beta1 = beta1; a.beta2 = beta2;
  const long long items = 2LL * N * a.chunks;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(flow_consistency_partial, grid_for(items), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(flow_consistency_final, dim3(1), dim3(kThreads), 0, st, a);
  return check_launch(what);
}
