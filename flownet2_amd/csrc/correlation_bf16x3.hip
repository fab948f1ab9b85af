// Correlation forward, FlowNetC / FlowNet2 instance (kernel_size 1, stride_1 1, stride_2 2, max_displacement 20 = pad, MULTIPLY), in
// SPLIT-bf16 ("bf16x3") arithmetic on v_mfma_f32_16x16x32_bf16: an opt-in second arithmetic beside the exact kernels of
// correlation_units.hip / correlation_mfma.hip (FN2_CONV_ARITH_BF16X3 beside FN2_CORR_ROUTE_OWN).  One launch per call, no workspace, no
// pre-split copy of the maps; the top may be a channel slice of a wider blob, ReLU{negative_slope} fused (fn2_correlation_forward_fused).
//
// Arithmetic: that of csrc/conv_bf16x3.hip.  Every fp32 value of BOTH bottoms is cut into three bf16 pieces  h = rne(v), m = rne(v - h),
// l = rne(v - h - m)  inside the kernel (there are no weights: both operands are activations); the six leading piece products are summed
// in fp32 on ONE accumulator per output tile in the order mm, lh, hl, mh, hm, hh (first letter: the piece of bottom0).  K-steps are
// blocks of 32 channels in ascending order, no K split; 1 / C and the ReLU are applied to the final value on the way out.  The summation
// order of an output element therefore depends on neither the batch, the variant nor the run: every variant writes the same bits.
// Non-finite inputs: Inf splits into (inf, nan, nan); an output whose products cover an Inf or a NaN is non-finite, all others keep their
// bits (out-of-band products of a tile are computed and dropped, so they never reach another output).
//
// Formulation: in the class coordinates of one y parity (y = 2 i + py, x = 2 j + px) the op is a 2-D banded product
// between 4 x 4 patches of positions of the first map (M) and of the second (N).  The patch (I, p) = rows 4 I .. + 3, columns 4 p .. + 3
// meets the N tiles (a, b), a, b = 0 .. 5: rows 4 I - 10 + 4 a + ni, columns 4 (p + b) - 10 + nj; displacement (4 a + ni - mi - 10,
// 4 b + nj - mj - 10), products outside the 21 x 21 band are dropped.  Rows and columns outside the image are staged as zeros; a task
// whose four N rows all lie outside the image runs no K loop and writes zeros.
//   task  = (sample, py, I, a, group of PG neighbouring patches) = one workgroup of 2 PG waves; wave w owns the patch p0 + (w >> 1) and its
//           N tiles b = 3 (w & 1) .. + 2, both x parities: 6 accumulator tiles, 36 MFMAs per k-step.  Every output row segment (8 PG
//           pixels of one (displacement, y)) is written by one workgroup.
//   image = the k-step's operands in LDS, [piece 3][channel octet 4][first map: (row, px) 8 x SA | second map: (row, px) 8 x SB] entries
//           of 16 bytes (8 channels of one pixel): each thread fetches pixel quads of 8 channels (8 x global_load_dwordx4, a k-step ahead of
//           their use), splits them in registers (split8) and writes three entries per pixel.  Positions are stored by x parity, so a
//           lane's operand (row = lane & 15 -> (row of the patch, column), octet = lane >> 4) is one ds_read_b128 per piece, and the staged
//           rows serve both parities.  2 SA = 4, 2 SB = 12 (mod 16) entries and octet planes a multiple of 16 entries apart: the four
//           16-lane groups of a ds_read_b128 (two patch rows of one octet, the other two of its neighbour) fill the 256-byte bank row.
//           One image: barrier -> split -> barrier -> (fetch of the next k-step) + MFMAs.
//   out   = accumulators -> LDS image [mi][ni][o][x] over the operand image -> 16-byte stores of whole row segments (the exact kernels' epilogue).
// Budget: a k-step of pieces is 192 bytes per staged pixel; PG = 4 stages 4 x (32 + 72) pixels = 84 KiB (one workgroup of 8 waves per CU),
// PG = 2 stages 4 x (16 + 56) pixels = 60 KiB (two workgroups of 4 waves per CU); the output image (44 / 23 KiB) overlays it.
// Build figures (hipcc -O3, gfx950, from -Rpass-analysis=kernel-resource-usage), variant 0 / 1 = PG 4 / 2: 114 / 150 VGPRs, 86,016 / 61,440
// bytes of (dynamic) LDS, no spills, no scratch; 1 / 2 workgroups per CU (LDS), two waves per SIMD either way.
// Measured on an MI355X (profiles/corr_bf16x3_bench.md): SLOWER than the exact kernels at all three BASELINE shapes.  Both operands are
// activations, so every staged value is split by each task that stages it (a second-map row by up to 6 N patch rows x 2.25): about 390 VALU
// instructions per wave and k-step beside 36 MFMAs, where the exact kernel moves the same rows by LDS-DMA.  The arithmetic floor, 6/16 of the
// exact kernel's matrix time, is not what bounds this kernel.
#include "correlation.hpp"
#include "autotune.hpp"
#include "mfma_tile.hpp"
#include "split_bf16.hpp"

namespace fn2 {
namespace cbx {

using namespace mfma;
using namespace bf16x3;

constexpr int R = 10, D = 2 * R + 1, NBT = 6;         // displacement radius in class units, displacements per axis, N tiles around a patch
constexpr int OROWS = 16 * D;                           // (mi, ni, o) rows of the output image
constexpr int NU = 3;                                   // N tiles of a wave

struct Args {
  const float* b0; const float* b1; float* top;
  int N, C, H, W;
  int NI, NG;            // patch rows per y parity, patch groups per image row
  int ctot, c0, relu; float slope;
};

template <int PG_, int WGS_>
struct Cfg {
  static constexpr int PG = PG_, WGS = WGS_, WAVES = 2 * PG, THREADS = 64 * WAVES;
  static constexpr int QA = 2 * PG, QB = 2 * (PG + NBT - 1);          // pixel quads of a staged row of the first / second map
  static constexpr int SA = 4 * PG + 2, SB = 4 * (PG + NBT - 1) + 2;  // entries of a (row, x parity): class columns + 2
  static constexpr int BOFF = 8 * SA, PLANE = 8 * SA + 8 * SB;        // entries of a (piece, octet) plane; the second map's part of it
  static constexpr int PS = 4 * PLANE;                                // entries of a piece
  static constexpr int ITEMS_K = 4 * QA + 4 * QB, ITEMS = 4 * ITEMS_K;   // staging items (octet, row, pixel quad) of a k-step
  static constexpr int ROUNDS = (ITEMS + THREADS - 1) / THREADS;
  static constexpr int XS = 8 * PG + 1, IMGF = OROWS * XS;            // output image: floats per row / in all
  static constexpr int LDS_BYTES = 3 * PS * 16 > IMGF * 4 ? 3 * PS * 16 : IMGF * 4;
  static_assert((2 * SA) % 16 == 4 && (2 * SB) % 16 == 12 && PLANE % 16 == 0, "bank rules of ds_read_b128");
  static_assert(THREADS % (2 * PG) == 0 && NU * 2 == NBT, "row passes of the epilogue; two waves per patch");
};

template <class K>
__global__ void __launch_bounds__(K::THREADS, K::WGS)
corr_fwd_bf16x3(Args g) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  u32x4* const img = reinterpret_cast<u32x4*>(smem);
  // ---- task decode (scalar): group fastest, then a, I, py, sample
  unsigned t = blockIdx.x;
  const int grp = (int)(t % (unsigned)g.NG); t /= (unsigned)g.NG;
  const int a = (int)(t % NBT); t /= NBT;
  const int I = (int)(t % (unsigned)g.NI); t /= (unsigned)g.NI;
  const int py = (int)(t & 1u), n = (int)(t >> 1);
  const int Hc = (g.H - py + 1) >> 1;                    // class rows of this y parity
  if (4 * I >= Hc || n >= g.N) return;                   // no output row in this patch row (odd heights, y parity 1)
  const int p0 = grp * K::PG, i2_0 = 4 * I - R + 4 * a;
  const bool live = i2_0 + 3 >= 0 && i2_0 < Hc;          // some N row touches the image

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t plane = (size_t)g.H * g.W;
  const int pl = wave >> 1, bb0 = NU * (wave & 1);
  const bool active = 8 * (p0 + pl) < g.W;               // the wave's patch touches the image

  f32x4 acc[NU][2];
#pragma unroll
  for (int u = 0; u < NU; ++u) { acc[u][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[u][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  if (live) {
    // ---- staging items of this thread: (octet kq, staged row, pixel quad) -> 8 channels x 4 pixels
    const float* src[K::ROUNDS];
    bool ok[K::ROUNDS];
    int widx[K::ROUNDS], wps[K::ROUNDS];
#pragma unroll
    for (int r = 0; r < K::ROUNDS; ++r) {
      const int it = tid + r * K::THREADS;
      const int kq = it / K::ITEMS_K, q = it % K::ITEMS_K;
      const bool isA = q < 4 * K::QA;
      const int qb = q - 4 * K::QA;
      const int row = isA ? q / K::QA : qb / K::QB, quad = isA ? q % K::QA : qb % K::QB;
      const int i = isA ? 4 * I + row : i2_0 + row;
      const int y = 2 * i + py, x0 = 8 * p0 + 4 * quad - (isA ? 0 : 2 * R);
      ok[r] = it < K::ITEMS && i >= 0 && y < g.H && x0 >= 0 && x0 < g.W;       // W % 4 == 0: a quad is inside the row or outside it
      const float* map = (isA ? g.b0 : g.b1) + (size_t)n * g.C * plane;
      src[r] = map + (ok[r] ? (size_t)(8 * kq) * plane + (size_t)y * g.W + x0 : 0);
      wps[r] = isA ? K::SA : K::SB;
      widx[r] = kq * K::PLANE + (isA ? 0 : K::BOFF) + 2 * row * wps[r] + 2 * quad;
    }
    // ---- operands of this lane: row of the tile = lane & 15 = (row hi, column lo), octet = lane >> 4
    const int kq = lane >> 4, hi = (lane & 15) >> 2, lo = lane & 3;
    const int aidx = kq * K::PLANE + 2 * hi * K::SA + 4 * pl + lo;                         // + px SA
    const int bidx = kq * K::PLANE + K::BOFF + 2 * hi * K::SB + 4 * (pl + bb0) + lo;       // + px SB + 4 u

    f32x4 xr[K::ROUNDS][8];
    auto fetch = [&](int ks) {
#pragma unroll
      for (int r = 0; r < K::ROUNDS; ++r)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xr[r][j] = ok[r] ? *reinterpret_cast<const f32x4*>(src[r] + (size_t)(32 * ks + j) * plane) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    const int ksteps = g.C / 32;
    fetch(0);
#pragma unroll 1
    for (int ks = 0; ks < ksteps; ++ks) {
      __syncthreads();                     // every wave is done with the image of k-step ks - 1
#pragma unroll
      for (int r = 0; r < K::ROUNDS; ++r) {
        if (r + 1 < K::ROUNDS || tid + r * K::THREADS < K::ITEMS) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {    // pixel x0 + e: x parity e & 1, class column 2 quad + (e >> 1)
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = xr[r][j][e];
            store_pieces(img + widx[r] + (e & 1) * wps[r] + (e >> 1), K::PS, v);
          }
        }
      }
      __syncthreads();                     // the image is whole
      if (ks + 1 < ksteps) fetch(ks + 1);
      if (active) {
        u32x4 xa[2][3];
#pragma unroll
        for (int px = 0; px < 2; ++px)
#pragma unroll
          for (int q = 0; q < 3; ++q) xa[px][q] = img[q * K::PS + aidx + px * K::SA];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          u32x4 xb[2][3];
#pragma unroll
          for (int px = 0; px < 2; ++px)
#pragma unroll
            for (int q = 0; q < 3; ++q) xb[px][q] = img[q * K::PS + bidx + px * K::SB + 4 * u];
#pragma unroll
          for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int px = 0; px < 2; ++px)
              acc[u][px] = piece_mfma_16x16x32(i, xa[px], xb[px], acc[u][px]);
        }
      }
    }
  }

  // ---- accumulators -> LDS image [mi][ni][o][x] (over the operand image).  Accumulator role: row = 4 mi + reg (M position (mi, reg)),
  // column = N position (ni, nj); element (o = 4 b + nj - reg, x = 8 pl + 2 reg + px)
  __syncthreads();
  if (active) {
    const int mi = lane >> 4, ni = (lane & 15) >> 2, nj = lane & 3;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oo = 4 * (bb0 + u) + nj - r;              // o + R
        if (oo >= 0 && oo < D) {
          float* dst = smem + ((mi * 4 + ni) * D + oo) * K::XS + 8 * pl + 2 * r;
          dst[0] = acc[u][0][r];
          dst[1] = acc[u][1][r];
        }
      }
    }
  }
  __syncthreads();
  // ---- rows out: rowid = (rmi * 4 + rni) * D + oo  <->  top[n, (qq = 4 a + rni - rmi, oo), y = 2 (4 I + rmi) + py, 8 PG px from 8 p0]
  constexpr int LPR = 2 * K::PG, RPP = K::THREADS / LPR;    // 16-byte quads per row, rows per pass
  const int trow = tid / LPR, xq = tid % LPR;
  const int x = 8 * p0 + 4 * xq;
  if (x >= g.W) return;
  const bool pow2 = (g.C & (g.C - 1)) == 0;                 // x / 2^k == x * 2^-k exactly; otherwise the reference's true division
  const float scale = 1.0f / (float)g.C, sumelems = (float)g.C, slope = g.slope;
  const bool relu = g.relu != 0;
  float* const top_n = g.top + ((size_t)n * g.ctot + g.c0) * plane;
#pragma unroll 1
  for (int rowid = trow; rowid < OROWS; rowid += RPP) {
    const int blk = rowid / D, oo = rowid - blk * D, rmi = blk >> 2, rni = blk & 3;
    const int qq = 4 * a + rni - rmi, y = 2 * (4 * I + rmi) + py;
    if (qq < 0 || qq >= D || y >= g.H) continue;
    const float* s = smem + rowid * K::XS + 4 * xq;
    f32x4 v = f32x4{s[0], s[1], s[2], s[3]};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float f = pow2 ? v[e] * scale : v[e] / sumelems;
      if (relu) f = f > 0.f ? f : f * slope;
      v[e] = f;
    }
    *reinterpret_cast<f32x4*>(top_n + (size_t)(qq * D + oo) * plane + (size_t)y * g.W + x) = v;
  }
}

template <class K>
static int launch(const Args& base, hipStream_t st) {
  Args g = base;
  g.NG = cdiv(cdiv(g.W, 8), K::PG);
  const long long tasks = (long long)g.N * 2 * g.NI * NBT * g.NG;
  if (tasks > 0x7ffffff0ll) return fail(FN2_ERR_UNSUPPORTED, "correlation_bf16x3: grid too large");
  set_dynamic_lds_once<&corr_fwd_bf16x3<K>>(K::LDS_BYTES);
  hipLaunchKernelGGL((corr_fwd_bf16x3<K>), dim3((unsigned)tasks), dim3(K::THREADS), K::LDS_BYTES, st, g);
  return check_launch("correlation_forward (bf16x3)");
}

struct Variant {
  int pg, wgs;
  int (*fn)(const Args&, hipStream_t);
};
// 4 patches per task on 8 waves (one workgroup per CU), 2 patches on 4 waves (two per CU: narrow maps waste less of a group)
static const Variant kVariants[] = {{4, 1, &launch<Cfg<4, 1>>}, {2, 2, &launch<Cfg<2, 2>>}};
FN2_BF16X3_VARIANT_KNOBS(correlation_bf16x3)

// Cost model: rounds of workgroups over the chip's slots (256 CUs x workgroups per CU) x the staged pixels of a task (the split of the
// operands, not the matrix pipe, sets a k-step's time)
static double variant_cost(const Variant& v, const Args& g) {
  const long long tasks = (long long)g.N * 2 * g.NI * NBT * cdiv(cdiv(g.W, 8), v.pg), slots = 256 * v.wgs;
  return (double)((tasks + slots - 1) / slots) * (8 * v.pg + 8 * (v.pg + NBT - 1));
}

}  // namespace cbx

// geometry alone: the FlowNetC instance, whole k-steps of 32 channels, whole 16-byte pixel quads, the 32-bit offset limits of the exact kernels
bool corr_bf16x3_geometry_ok(const fn2_corr_params* p, int N, int C, int H, int W) {
  if (!p || N < 0 || C < 1 || H < 1 || W < 1) return false;
  if (p->kernel_size != 1 || p->stride1 != 1 || p->stride2 != 2 || p->max_displacement != 2 * cbx::R || p->pad != p->max_displacement ||
      p->corr_type != FN2_CORR_MULTIPLY)
    return false;
  if (C % 32 != 0 || W % 4 != 0) return false;
  if ((long long)C * H * W >= (1ll << 28) || (long long)cbx::D * cbx::D * H * W >= (1ll << 30)) return false;
  const long long NI = ((H + 1) / 2 + 3) / 4, NG = (W + 15) / 16;          // tasks of the finest variant
  return (long long)N * 2 * NI * cbx::NBT * NG <= 0x7ffffff0ll;
}

int corr_bf16x3_launch(const CorrGeom& cg, const float* b0, const float* b1, float* top, hipStream_t st) {
  cbx::Args g{};
  g.b0 = b0; g.b1 = b1; g.top = top;
  g.N = cg.N; g.C = cg.C; g.H = cg.H; g.W = cg.W;
  g.NI = ((cg.H + 1) / 2 + 3) / 4;
  g.ctot = cg.top_ctot; g.c0 = cg.top_c0; g.relu = cg.relu; g.slope = cg.slope;
  static TuneCache cache("correlation_bf16x3", cbx::kNumVariants);
  const TuneKey key{cg.N, cg.C, cg.H, cg.W, cg.relu, 0, 0, 0, 0, 0};
  return bf16x3::pick_and_run("correlation_bf16x3", cbx::g_forced_variant, cbx::kNumVariants, cache, key, st, [](int) { return true; },
                              [&](int i) { return cbx::variant_cost(cbx::kVariants[i], g); }, [&](int i) { return cbx::kVariants[i].fn(g, st); });
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_correlation_bf16x3_supported(const fn2_corr_params* p, int N, int C, int H, int W) {
  return corr_bf16x3_geometry_ok(p, N, C, H, W) ? 1 : 0;
}
