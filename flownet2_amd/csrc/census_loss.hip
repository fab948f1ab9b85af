// Census data term of the unsupervised loss for gfx950: the soft Hamming distance between the ternary census signatures of an image and
// of the other image warped by the flow, over a (2 radius + 1)^2 patch, both directions in every launch, the per-sample rows and the loss
// in fp64 from a one-workgroup finalise.  include/flownet2_hip_census_loss.h states the arithmetic; DESIGN.md section 3.19 has the
// derivation of the backward, the byte counts and the launch structure.
//
// Composed from flow_warp, unfold and eager tensor operations this is 48 planes of temporaries per image and direction.  Here:
//   warp pass     a thread per pixel forms the two grey values G (own image) and Wg (other image at the flow's target, FlowWarp's taps)
//                 and the pixel's status, and writes them as three planes: into `saved` (the backward reads them again) or, without one,
//                 into the workspace.  The third plane holds the status until the stencil pass overwrites it with pd.
//   stencil pass  a workgroup stages a 32 x 8 tile of G and Wg plus a halo of `radius` in LDS (NaN outside the plane and where a value is
//                 not defined: one test decides whether a pair exists), a thread evaluates the pairs of its pixel from LDS -- every
//                 value is read (2 radius + 1)^2 times, which is what LDS is for --, writes pd and keeps its sums in registers; then, as
//                 in the other streaming losses: wave64 reduction -> LDS -> one fp64 partial row per workgroup.
//   finalise      adds a sample's partial rows in index order, the sample rows in sample order, and forms the loss.
//   backward      one launch over the same tiles, now of three planes (G, Wg, pd): a pure gather over the pixel's own patch (the header
//                 has the identity that makes it one), then the pixel's own taps again for d Wg / d flow.  No reduction, no atomics.
// The warp pass is a pass of its own, not folded into the stencil pass: a folded kernel would warp its halo again ((32 + 2r)(8 + 2r) /
// 256 = 2.1 times the gathers at radius 3), and the planes have to reach memory for the backward anyway.
//
// A work item of the stencil pass is (direction, sample, chunk), B = min(tiles, 128) chunks per sample from (H, W) alone: a sample's row
// has the same bits alone and in any batch.  Every operation is rounded on its own (fp contract off).
//
// Reads stay inside the sample: the warp pass forms tap indices only after the finite and inside tests, from a coordinate in
// [0, W) x [0, H), clamped to W - 1 and H - 1 (the backward takes the tests again instead of trusting `saved`); the staging loop reads a
// plane only at coordinates it has tested against [0, W) x [0, H); a thread whose pixel lies outside the plane (a ragged tile) does nothing
// but stage and reduce.
#include "stream_reduce.hpp"
#include "../../include/flownet2_hip_census_loss.h"

#pragma clang fp contract(off)

namespace fn2 {

using namespace stream;

constexpr int kClK = FN2_CENSUS_LOSS_K;                // every column is a sum
constexpr int kClMaxC = 4;
constexpr int kClTW = 32, kClTH = 8;                   // the tile: one pixel per thread
static_assert(kClTW * kClTH == kThreads, "one pixel of a tile per thread");
enum { kClCounted = 0, kClOccluded, kClOutside, kClNonfinite };

struct ClArgs {
  const float* img[2];         // direction d: Ia = img[d], Io = img[1 - d]
  const float* flow[2];
  const float* occ[2];         // forward
  float* planes;               // forward: [2][N][3][H][W], G, Wg, status then pd: `saved` or the workspace
  const float* saved;          // backward: what the forward left there
  float* diff[2];              // backward
  double* partial;             // forward: [dirs][N][B][K]
  double* results;             // forward: [2][N + 1][K]
  const double* totals;        // backward: the forward's results
  float* loss;
  const float* total_diff;
  int N, C, H, W;
  int tiles_x, tiles;          // tiles along x, tiles of a plane
  int chunks;                  // B
  int dirs;                    // directions run: 1 or 2
  float dw, eps_d, gam_d, c_t, c_h, gsc, mult;
};

__device__ __forceinline__ float cl_psi(float t, float eps, float gam) {
  const float r = t * t + eps * eps;
  return gam == 0.5f ? sqrtf(r) : powf(r, gam);
}

__device__ __forceinline__ float cl_dpsi(float t, float eps, float gam) {
  const float r = t * t + eps * eps;
  return gam == 0.5f ? t / sqrtf(r) : ((2.0f * gam) * t) * powf(r, gam - 1.0f);
}

__device__ __forceinline__ bool cl_defined(float v) { return v == v; }      // an undefined grey value is stored as a NaN

// ---- the warp pass ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) census_loss_warp(ClArgs a) {
  const size_t hw = (size_t)a.H * a.W;
  const long long total = (long long)a.dirs * a.N * (long long)hw;
  const float nan = __builtin_nanf("");
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const long long dn = i / (long long)hw;                                 // d * N + n
    const unsigned r = (unsigned)(i - dn * (long long)hw);                  // H W < 2^30
    const int d = dn >= a.N ? 1 : 0;
    const long long n = dn - (long long)d * a.N;
    const int y = (int)(r / (unsigned)a.W), x = (int)(r - (unsigned)y * a.W);
    const float* __restrict__ Ia = a.img[d] + (size_t)n * a.C * hw;
    const float* __restrict__ Io = a.img[1 - d] + (size_t)n * a.C * hw;
    const float* __restrict__ u = a.flow[d] + (size_t)n * 2 * hw;
    bool gdef = true;
    float gs = 0.f;
    for (int c = 0; c < a.C; ++c) {
      const float v = Ia[(size_t)c * hw + r];
      gdef = gdef && finite_1e9(v);
      gs += v;
    }
    const float G = gdef ? gs * a.gsc : nan;
    const float au = a.mult * u[r], av = a.mult * u[hw + r];
    const bool fin = finite_1e9(au) && finite_1e9(av);
    const bool occluded = a.occ[d] && !(a.occ[d][(size_t)n * hw + r] == 0.0f);
    bool inside = false;
    float Wg = nan;
    if (fin) {
      const float x2 = (float)x + au, y2 = (float)y + av;
      inside = x2 >= 0.f && y2 >= 0.f && x2 < (float)a.W && y2 < (float)a.H;
      if (inside) {
        const BilinearTaps t = bilinear_taps(x2, y2, a.W, a.H);
        bool tapfin = true;
        float ws = 0.f;
        for (int c = 0; c < a.C; ++c) {
          const float* __restrict__ p = Io + (size_t)c * hw;
          const float TL = p[t.oTL], TR = p[t.oTR], BL = p[t.oBL], BR = p[t.oBR];
          tapfin = tapfin && finite_1e9(TL) && finite_1e9(TR) && finite_1e9(BL) && finite_1e9(BR);
          ws += ((t.wTL * TL + t.wTR * TR) + t.wBL * BL) + t.wBR * BR;
        }
        if (tapfin) Wg = ws * a.gsc;
      }
    }
    const int cls = !fin ? kClNonfinite : occluded ? kClOccluded : !inside ? kClOutside
                    : (!cl_defined(G) || !cl_defined(Wg)) ? kClNonfinite : kClCounted;
    float* __restrict__ P = a.planes + (size_t)dn * 3 * hw + r;
    P[0] = G;
    P[hw] = Wg;
    P[2 * hw] = (float)cls;
  }
}

// ---- the staged tile --------------------------------------------------------------------------------------------------------------
// P planes [H][W] at `planes` (hw apart) -> lds[P][kClTH + 2 R][kClTW + 2 R] around the tile at (x0, y0); NaN outside the plane
template <int R, int P>
__device__ __forceinline__ void cl_stage(float (&lds)[P][kClTH + 2 * R][kClTW + 2 * R], const float* __restrict__ planes, size_t hw, int x0,
                                         int y0, int W, int H) {
  constexpr int WW = kClTW + 2 * R, HH = kClTH + 2 * R;
  const float nan = __builtin_nanf("");
  for (int i = threadIdx.x; i < WW * HH; i += kThreads) {
    const int ly = i / WW, lx = i - ly * WW;
    const int gy = y0 - R + ly, gx = x0 - R + lx;
    const bool in = gx >= 0 && gy >= 0 && gx < W && gy < H;
    const size_t o = in ? (size_t)gy * W + gx : 0;
#pragma unroll
    for (int p = 0; p < P; ++p) lds[p][ly][lx] = in ? planes[(size_t)p * hw + o] : nan;
  }
  __syncthreads();
}

struct ClPair {
  float h, e, den, rb;
};

// the pair of a centre (g0, w0) and a neighbour (gq, wq), both defined
__device__ __forceinline__ ClPair cl_pair(float g0, float w0, float gq, float wq, float c_t, float c_h) {
  const float a = gq - g0, ra = a * a + c_t, ta = a / sqrtf(ra);
  const float b = wq - w0, rb = b * b + c_t, tb = b / sqrtf(rb);
  const float e = ta - tb, s = e * e, den = s + c_h;
  return {s / den, e, den, rb};
}

// what one thread has seen; counts stay integers until the reduction (a thread sees fewer than 2^31 pixels and pairs: H W < 2^30 is cut
// into tiles of 256 threads, 48 pairs a pixel)
struct ClSums {
  double data, dist;
  int cnt[4];
  int pixels, pairs;
};

template <int R>
__device__ __forceinline__ void cl_forward_tile(const ClArgs& a, float* __restrict__ planes, size_t hw, int tile, ClSums& t,
                                                float (&lds)[2][kClTH + 2 * R][kClTW + 2 * R]) {
  const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
  const int x0 = txi * kClTW, y0 = tyi * kClTH;
  cl_stage<R, 2>(lds, planes, hw, x0, y0, a.W, a.H);
  const int tx = threadIdx.x & (kClTW - 1), ty = threadIdx.x / kClTW;
  const int x = x0 + tx, y = y0 + ty;
  if (x < a.W && y < a.H) {
    float* __restrict__ own = planes + 2 * hw + (size_t)y * a.W + x;       // the status, then pd: read and written by this thread alone
    const int cls = (int)own[0];
    t.pixels += 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) t.cnt[c] += cls == c ? 1 : 0;
    float pd = 0.0f;
    if (cls == kClCounted) {
      const float g0 = lds[0][ty + R][tx + R], w0 = lds[1][ty + R][tx + R];
      float dist = 0.f;
      int pairs = 0;
#pragma unroll
      for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
          const float gq = lds[0][ty + R + dy][tx + R + dx], wq = lds[1][ty + R + dy][tx + R + dx];
          const bool ex = cl_defined(gq) && cl_defined(wq) && !(dx == 0 && dy == 0);
          const ClPair p = cl_pair(g0, w0, gq, wq, a.c_t, a.c_h);
          dist = ex ? dist + p.h : dist;
          pairs += ex ? 1 : 0;
        }
      }
      t.pairs += pairs;
      t.dist += (double)dist;
      t.data += (double)cl_psi(dist, a.eps_d, a.gam_d);
      pd = cl_dpsi(dist, a.eps_d, a.gam_d);
    }
    own[0] = pd;
  }
  __syncthreads();                                           // the next tile of this workgroup stages into lds again
}

template <int R>
__global__ void __launch_bounds__(kThreads) census_loss_stencil(ClArgs a) {
  __shared__ float lds[2][kClTH + 2 * R][kClTW + 2 * R];
  __shared__ double red[4][kClK];
  const size_t hw = (size_t)a.H * a.W;
  const long long items = (long long)a.dirs * a.N * a.chunks;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const long long dn = w / a.chunks;                       // d * N + n
    const int chunk = (int)(w - dn * a.chunks);
    float* __restrict__ planes = a.planes + (size_t)dn * 3 * hw;
    ClSums t = {};
    for (int tile = chunk; tile < a.tiles; tile += a.chunks) cl_forward_tile<R>(a, planes, hw, tile, t, lds);
    double row[kClK];
    row[FN2_CENSUS_LOSS_PIXELS] = (double)t.pixels;
    row[FN2_CENSUS_LOSS_COUNTED] = (double)t.cnt[kClCounted];
    row[FN2_CENSUS_LOSS_OCCLUDED] = (double)t.cnt[kClOccluded];
    row[FN2_CENSUS_LOSS_OUTSIDE] = (double)t.cnt[kClOutside];
    row[FN2_CENSUS_LOSS_NONFINITE] = (double)t.cnt[kClNonfinite];
    row[FN2_CENSUS_LOSS_DATA_SUM] = t.data;
    row[FN2_CENSUS_LOSS_PAIRS] = (double)t.pairs;
    row[FN2_CENSUS_LOSS_DIST_SUM] = t.dist;
    reduce_row<kClK, 0u>(row, red, a.partial + (size_t)w * kClK);      // partial[((d * N + n) * B + chunk) * K]
  }
}

// One workgroup.  The two directions are the groups of the plain finalise, a direction that was not run gets zeros; then one thread forms
// the loss.
__global__ void __launch_bounds__(kThreads) census_loss_final(ClArgs a) {
  finalize_rows<kClK, 0u>(a.partial, a.results, 2, a.N, a.chunks, a.dirs);
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0 && a.loss) {
    double L = 0.0;
    for (int d = 0; d < a.dirs; ++d) {
      const double* t = a.results + ((size_t)d * (a.N + 1) + a.N) * kClK;
      L = L + ((double)a.dw * t[FN2_CENSUS_LOSS_DATA_SUM]) / fmax(t[FN2_CENSUS_LOSS_COUNTED], 1.0);
    }
    a.loss[0] = (float)L;
  }
}

// ---- the backward -----------------------------------------------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(kThreads) census_loss_grad(ClArgs a) {
  __shared__ float lds[3][kClTH + 2 * R][kClTW + 2 * R];
  const size_t hw = (size_t)a.H * a.W;
  const long long items = (long long)a.dirs * a.N * a.tiles;
  const int tx = threadIdx.x & (kClTW - 1), ty = threadIdx.x / kClTW;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const long long dn = w / a.tiles;                        // d * N + n
    const int tile = (int)(w - dn * a.tiles);
    const int d = dn >= a.N ? 1 : 0;
    const long long n = dn - (long long)d * a.N;
    const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
    const int x0 = txi * kClTW, y0 = tyi * kClTH;
    cl_stage<R, 3>(lds, a.saved + (size_t)dn * 3 * hw, hw, x0, y0, a.W, a.H);
    const int x = x0 + tx, y = y0 + ty;
    if (x < a.W && y < a.H) {
      const unsigned r = (unsigned)y * (unsigned)a.W + (unsigned)x;
      const float g0 = lds[0][ty + R][tx + R], w0 = lds[1][ty + R][tx + R], p0 = lds[2][ty + R][tx + R];
      float ou = 0.0f, ov = 0.0f;
      const float* __restrict__ u = a.flow[d] + (size_t)n * 2 * hw;
      const float au = a.mult * u[r], av = a.mult * u[hw + r];
      const float x2 = (float)x + au, y2 = (float)y + av;
      const bool there = finite_1e9(au) && finite_1e9(av) && x2 >= 0.f && y2 >= 0.f && x2 < (float)a.W && y2 < (float)a.H;
      if (cl_defined(g0) && cl_defined(w0) && there) {
        const double* __restrict__ tot = a.totals + ((size_t)d * (a.N + 1) + a.N) * kClK;
        const float gdiff = a.total_diff ? a.total_diff[0] : 1.f;
        const float kd = gdiff * (float)((double)a.dw / fmax(tot[FN2_CENSUS_LOSS_COUNTED], 1.0));
        float acc = 0.f;
#pragma unroll 1
        for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
          for (int dx = -R; dx <= R; ++dx) {
            const float gq = lds[0][ty + R + dy][tx + R + dx], wq = lds[1][ty + R + dy][tx + R + dx], pq = lds[2][ty + R + dy][tx + R + dx];
            const bool ex = cl_defined(gq) && cl_defined(wq) && !(dx == 0 && dy == 0);
            const ClPair p = cl_pair(g0, w0, gq, wq, a.c_t, a.c_h);
            const float F = -(((2.0f * a.c_h) * p.e) / (p.den * p.den)) * (a.c_t / (p.rb * sqrtf(p.rb)));
            acc = ex ? acc + (p0 + pq) * F : acc;
          }
        }
        const float DW = (-kd) * acc;
        const BilinearTaps t = bilinear_taps(x2, y2, a.W, a.H);
        const float gy = (float)t.iyB - y2, gx = (float)t.ixR - x2;
        const float* __restrict__ Io = a.img[1 - d] + (size_t)n * a.C * hw;
        float su = 0.f, sv = 0.f;
        for (int c = 0; c < a.C; ++c) {
          const float* __restrict__ p = Io + (size_t)c * hw;
          const float TL = p[t.oTL], TR = p[t.oTR], BL = p[t.oBL], BR = p[t.oBR];
          su += gy * (TR - TL) + (1.f - gy) * (BR - BL);
          sv += gx * (BL - TL) + (1.f - gx) * (BR - TR);
        }
        ou = a.mult * ((DW * a.gsc) * su);
        ov = a.mult * ((DW * a.gsc) * sv);
      }
      float* __restrict__ o = a.diff[d] + (size_t)n * 2 * hw + r;
      o[0] = ou;
      o[hw] = ov;
    }
    __syncthreads();                                         // the next tile of this workgroup stages into lds again
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int cl_shape(const char* what, int N, int C, int H, int W, int radius) {
  if (N < 1 || H < 1 || W < 1) return fail(FN2_ERR_INVALID_ARG, "%s: bad shape [%d,%d,%d,%d]", what, N, C, H, W);
  if (C < 1 || C > kClMaxC) return fail(FN2_ERR_INVALID_ARG, "%s: C = %d channels (need 1 .. %d)", what, C, kClMaxC);
  if (radius < 1 || radius > 3) return fail(FN2_ERR_INVALID_ARG, "%s: radius = %d (need 1 .. 3)", what, radius);
  return check_planes(what, N, C > 3 ? C : 3, H, W);         // the larger of an image [N,C,H,W] and one direction of saved [N,3,H,W]
}

static int cl_tiles_x(int W) { return (W + kClTW - 1) / kClTW; }
static int cl_tiles(int H, int W) { return cl_tiles_x(W) * ((H + kClTH - 1) / kClTH); }      // H W < 2^30
static int cl_chunks(int H, int W) { const int t = cl_tiles(H, W); return t < kMaxChunks ? t : kMaxChunks; }
static size_t cl_saved_floats(int N, int H, int W) { return (size_t)2 * N * 3 * H * W; }
static size_t cl_partial_bytes(int N, int H, int W) { return sizeof(double) * kClK * 2 * (size_t)N * cl_chunks(H, W); }
static size_t cl_ws_bytes(int N, int H, int W) { return cl_partial_bytes(N, H, W) + sizeof(float) * cl_saved_floats(N, H, W); }

// the checks both directions of differentiation share; fills what they share of `a`
static int cl_setup(const char* what, ClArgs& a, const float* img0, const float* img1, const float* fw, const float* bw, int N, int C, int H,
                    int W, float data_weight, float eps_d, float gamma_d, int radius, float c_t, float c_h, float intensity_scale,
                    float flow_mult) {
  if (!img0) return fail(FN2_ERR_INVALID_ARG, "%s: img0 == NULL", what);
  if (!img1) return fail(FN2_ERR_INVALID_ARG, "%s: img1 == NULL", what);
  if (!fw) return fail(FN2_ERR_INVALID_ARG, "%s: fw == NULL", what);
  int rc = cl_shape(what, N, C, H, W, radius);
  if (rc) return rc;
  if (!(data_weight >= 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: data_weight = %g (need >= 0)", what, data_weight);
  if (!(eps_d >= 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: eps_d = %g (need >= 0)", what, eps_d);
  const float pos[4] = {gamma_d, c_t, c_h, intensity_scale};
  const char* pos_names[4] = {"gamma_d", "c_t", "c_h", "intensity_scale"};
  for (int k = 0; k < 4; ++k)
    if (!(pos[k] > 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: %s = %g (need > 0)", what, pos_names[k], pos[k]);
  if (flow_mult != flow_mult) return fail(FN2_ERR_INVALID_ARG, "%s: flow_mult is NaN", what);
  a = ClArgs{};
  a.img[0] = img0; a.img[1] = img1;
  a.flow[0] = fw; a.flow[1] = bw;
  a.N = N; a.C = C; a.H = H; a.W = W;
  a.tiles_x = cl_tiles_x(W);
  a.tiles = cl_tiles(H, W);
  a.chunks = cl_chunks(H, W);
  a.dirs = bw ? 2 : 1;
  a.dw = data_weight; a.eps_d = eps_d; a.gam_d = gamma_d; a.c_t = c_t; a.c_h = c_h; a.mult = flow_mult;
  a.gsc = intensity_scale / (float)C;
  return FN2_OK;
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_census_loss_sizes(int N, int H, int W, int radius, size_t* workspace_bytes, size_t* saved_floats, int* K) {
  int rc = cl_shape("census_loss_sizes", N, 1, H, W, radius);
  if (rc) return rc;
  if (workspace_bytes) *workspace_bytes = cl_ws_bytes(N, H, W);
  if (saved_floats) *saved_floats = cl_saved_floats(N, H, W);
  if (K) *K = kClK;
  return FN2_OK;
}

FN2_API int fn2_census_loss_forward(const float* img0, const float* img1, const float* fw, const float* bw, const float* occ_fw,
                                    const float* occ_bw, int N, int C, int H, int W, float data_weight, float eps_d, float gamma_d, int radius,
                                    float c_t, float c_h, float intensity_scale, float flow_mult, double* results, float* loss, float* saved,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "census_loss_forward";
  if (!results) return fail(FN2_ERR_INVALID_ARG, "%s: results == NULL", what);
  ClArgs a;
  int rc = cl_setup(what, a, img0, img1, fw, bw, N, C, H, W, data_weight, eps_d, gamma_d, radius, c_t, c_h, intensity_scale, flow_mult);
  if (rc) return rc;
  if (!workspace || workspace_bytes < cl_ws_bytes(N, H, W))
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, cl_ws_bytes(N, H, W));
  a.occ[0] = occ_fw; a.occ[1] = occ_bw;
  a.partial = reinterpret_cast<double*>(workspace);
  a.planes = saved ? saved : reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + cl_partial_bytes(N, H, W));
  a.results = results;
  a.loss = loss;
  hipStream_t st = as_stream(stream);
  const long long pixels = (long long)a.dirs * N * ((long long)H * W);
  hipLaunchKernelGGL(census_loss_warp, grid_for((pixels + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a);
  const dim3 grid = grid_for((long long)a.dirs * N * a.chunks);
  if (radius == 1) hipLaunchKernelGGL(census_loss_stencil<1>, grid, dim3(kThreads), 0, st, a);
  else if (radius == 2) hipLaunchKernelGGL(census_loss_stencil<2>, grid, dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL(census_loss_stencil<3>, grid, dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(census_loss_final, dim3(1), dim3(kThreads), 0, st, a);
  return check_launch(what);
}

FN2_API int fn2_census_loss_backward(const float* img0, const float* img1, const float* fw, const float* bw, int N, int C, int H, int W,
                                     float data_weight, float eps_d, float gamma_d, int radius, float c_t, float c_h, float intensity_scale,
                                     float flow_mult, const double* results, const float* saved, const float* total_diff, float* fw_diff,
                                     float* bw_diff, void* stream) {
  const char* what = "census_loss_backward";
  if (!results) return fail(FN2_ERR_INVALID_ARG, "%s: results == NULL", what);
  if (!saved) return fail(FN2_ERR_INVALID_ARG, "%s: saved == NULL", what);
  if (!fw_diff) return fail(FN2_ERR_INVALID_ARG, "%s: fw_diff == NULL", what);
  if (bw_diff && !bw) return fail(FN2_ERR_INVALID_ARG, "%s: bw_diff without a bw", what);
  ClArgs a;
  int rc = cl_setup(what, a, img0, img1, fw, bw, N, C, H, W, data_weight, eps_d, gamma_d, radius, c_t, c_h, intensity_scale, flow_mult);
  if (rc) return rc;
  a.totals = results;
  a.saved = saved;
  a.total_diff = total_diff;
  a.diff[0] = fw_diff; a.diff[1] = bw_diff;
  a.dirs = bw_diff ? 2 : 1;
  const dim3 grid = grid_for((long long)a.dirs * N * a.tiles);
  hipStream_t st = as_stream(stream);
  if (radius == 1) hipLaunchKernelGGL(census_loss_grad<1>, grid, dim3(kThreads), 0, st, a);
  else if (radius == 2) hipLaunchKernelGGL(census_loss_grad<2>, grid, dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL(census_loss_grad<3>, grid, dim3(kThreads), 0, st, a);
  return check_launch(what);
}
