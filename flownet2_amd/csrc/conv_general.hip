// General-geometry Convolution / Deconvolution on v_mfma_f32_16x16x4_f32 (exact fp32): the last resort behind the specialised families.
// Contract, operand layout and summation order: include/flownet2_hip_conv_general.h.
//
// Everything is stated on the two SIDES of the layer, the larger map L and the smaller map S (Convolution: L = bottom, S = top;
// Deconvolution: L = top, S = bottom).  The weight blob is [Cs][Cl][k][k] for both kinds.  Then
//   forward gather    L -> S   Convolution forward, Deconvolution data gradient      M = Cs, K = Cl k k, Wp[cs][(cl, tap)] = W[cs][cl][tap]
//   transposed gather S -> L   Convolution data gradient, Deconvolution forward      M = Cl, K = Cs k k, Wp[cl][(cs, tap)] = W[cs][cl][tap]
//   weight gradient            dW[cs][(cl, tap)] = sum over (n, S pixels) of S[cs][p] x (forward gather of L)[(cl, tap)][p]
// so there are two gather kernels (one template), two pack layouts and one weight-gradient kernel for the four layer uses.
//
// Tiles.  A workgroup is 4 waves.  Gather kernel: 64 consecutive pixels (flattened y Wout + x, so a tile may wrap rows) of one sample x
// NG = 1, 2 or 4 groups of 16 output channels (by the channel count alone); per chunk of 16 k-rows every thread gathers 4 values (its
// pixel, k-rows wave, wave + 4, ...: the k decomposition is wave-uniform and advanced by carries, the divisions by the stride and the
// map width are multiplications), the next chunk's loads are in flight while the MFMAs of this one run; wave w multiplies pixels 16 w ..
// 16 w + 15 with the NG groups (the last block's missing groups repeat the last real one and are not stored).  Weight gradient: 16 k-columns x
// 64 channels, wave w owns channel group w, the reduction runs over chunks of 64 pixels staged the same way.
#include "mfma_tile.hpp"

#include "../../include/flownet2_hip_conv_general.h"

namespace fn2 {
namespace {

using mfma::f32x4;

constexpr int kPix = 64;        // pixels per tile / chunk
constexpr int kKC = 16;         // k-rows per chunk (four k-steps)
constexpr int kThreads = 256;
constexpr int kColStrideG = 80; // LDS row stride of the col tile, gather kernels: == 16 (mod 32), the k-step read [4 rows][16 pixels] is conflict-free
constexpr int kColStrideW = 66; // weight gradient: == 2 (mod 32), the read [16 rows][4 pixels] is conflict-free
constexpr long long kMaxElems = 0x7fffffffll;
constexpr long long kMaxTiles = 0x3fffff00ll;

// ------------------------------------------------------------------------------------------------ host geometry
struct Sides {
  int N, Cl, Hl, Wl, Cs, Hs, Ws, k, s, pad;
};

inline long long cdivll(long long a, long long b) { return (a + b - 1) / b; }

// the descriptor on its two sides; false: invalid, output extent below 1, or a blob beyond the 32-bit index limits
bool make_sides(const fn2_conv_desc* d, int transposed, Sides& g) {
  if (!d) return false;
  if (d->N < 1 || d->Cin < 1 || d->Hin < 1 || d->Win < 1 || d->Cout < 1 || d->kernel < 1 || d->stride < 1 || d->pad < 0) return false;
  long long Ho, Wo;
  if (!transposed) {
    if ((long long)d->Hin + 2ll * d->pad < d->kernel || (long long)d->Win + 2ll * d->pad < d->kernel) return false;
    Ho = ((long long)d->Hin + 2ll * d->pad - d->kernel) / d->stride + 1;
    Wo = ((long long)d->Win + 2ll * d->pad - d->kernel) / d->stride + 1;
  } else {
    Ho = (long long)d->stride * (d->Hin - 1) + d->kernel - 2ll * d->pad;
    Wo = (long long)d->stride * (d->Win - 1) + d->kernel - 2ll * d->pad;
  }
  if (Ho < 1 || Wo < 1 || Ho > kMaxElems || Wo > kMaxElems) return false;
  const long long kk = (long long)d->kernel * d->kernel;
  if (kk > kMaxElems) return false;
  const long long bottom = (long long)d->N * d->Cin, top = (long long)d->N * d->Cout;
  if (bottom > kMaxElems || top > kMaxElems) return false;
  const long long pb = (long long)d->Hin * d->Win, pt = Ho * Wo;
  if (pb > kMaxElems || pt > kMaxElems || bottom * pb > kMaxElems || top * pt > kMaxElems) return false;
  const long long cc = (long long)d->Cin * d->Cout;
  if (cc > kMaxElems || cc * kk > kMaxElems) return false;
  // the padded operands: (channels rounded to 16) x (K rounded to 16)
  const long long cmax = d->Cin > d->Cout ? d->Cin : d->Cout;
  if ((cdivll(cmax, 16) * 16) * (cdivll(cmax * kk, kKC) * kKC + kKC) > kMaxElems) return false;
  g.N = d->N; g.k = d->kernel; g.s = d->stride; g.pad = d->pad;
  if (!transposed) { g.Cl = d->Cin; g.Hl = d->Hin; g.Wl = d->Win; g.Cs = d->Cout; g.Hs = (int)Ho; g.Ws = (int)Wo; }
  else { g.Cs = d->Cin; g.Hs = d->Hin; g.Ws = d->Win; g.Cl = d->Cout; g.Hl = (int)Ho; g.Wl = (int)Wo; }
  return true;
}

// one GEMM view: M output channels, R reduction channels (K = R k k)
struct Gemm {
  int M, R, G, ksteps;      // G: 16-channel groups; ksteps: k-steps of the padded K (a multiple of 4)
  long long K, Kpad;
};

Gemm make_gemm(int M, int R, int k) {
  Gemm m;
  m.M = M; m.R = R; m.G = (M + 15) / 16;
  m.K = (long long)R * k * k;
  m.Kpad = cdivll(m.K, kKC) * kKC;
  m.ksteps = (int)(m.Kpad / 4);
  return m;
}

// which gather serves pass 0 (forward) / 1 (data gradient) of the layer kind: true = the transposed gather
inline bool pass_is_tr(int transposed, int pass) { return (pass == 1) != (transposed != 0); }
inline Gemm pass_gemm(const Sides& g, bool tr) { return tr ? make_gemm(g.Cl, g.Cs, g.k) : make_gemm(g.Cs, g.Cl, g.k); }
inline size_t packed_floats(const Gemm& m) { return (size_t)m.G * (size_t)m.ksteps * 64; }

struct WgradPlan {
  Gemm m;                   // M = Cs, R = Cl
  int ptiles, nsplit;       // 64-pixel chunks per sample; parts of the reduction
  long long chunks, per_part, tiles;
  size_t workspace_bytes;
};

WgradPlan make_wgrad(const Sides& g) {
  WgradPlan p;
  p.m = make_gemm(g.Cs, g.Cl, g.k);
  p.ptiles = (int)cdivll((long long)g.Hs * g.Ws, kPix);
  p.chunks = (long long)g.N * p.ptiles;
  const long long out_tiles = (p.m.Kpad / kKC) * ((p.m.G + 3) / 4);
  long long want = 2048 / out_tiles;                   // enough workgroups for the chip when the output has few tiles
  if (want > 64) want = 64;
  if (want > p.chunks) want = p.chunks;
  if (want < 1) want = 1;
  p.per_part = cdivll(p.chunks, want);
  p.nsplit = (int)cdivll(p.chunks, p.per_part);      // no empty part
  p.tiles = out_tiles * p.nsplit;
  p.workspace_bytes = sizeof(float) * (size_t)p.nsplit * (size_t)(16 * p.m.G) * (size_t)p.m.Kpad;
  return p;
}

// 16-channel groups per workgroup of the gather kernels: the three instantiations run the same accumulation chain per output value (the
// same bits); which one runs is a function of the channel count alone -- no autotuning -- unless the debug hook forces one
int& forced_groups() { static int f = 0; return f; }
inline int natural_groups(int G) { return G <= 1 ? 1 : G <= 2 ? 2 : 4; }
inline int groups_per_block(int G) { return forced_groups() ? forced_groups() : natural_groups(G); }

long long gather_tiles(const Sides& g, bool tr, const Gemm& m, int ng) {
  const long long P = tr ? (long long)g.Hl * g.Wl : (long long)g.Hs * g.Ws;
  return (long long)g.N * cdivll(P, kPix) * cdivll(m.G, ng);
}

bool supported(const fn2_conv_desc* d, int transposed, Sides& g) {
  if (!make_sides(d, transposed, g)) return false;
  const Gemm mf = pass_gemm(g, false), mt = pass_gemm(g, true);
  if (gather_tiles(g, false, mf, natural_groups(mf.G)) > kMaxTiles || gather_tiles(g, true, mt, natural_groups(mt.G)) > kMaxTiles) return false;
  const WgradPlan w = make_wgrad(g);
  return w.tiles <= kMaxTiles && w.workspace_bytes / sizeof(float) <= (size_t)kMaxElems;
}

// ------------------------------------------------------------------------------------------------ device: the col gather
struct GatherSrc {
  const float* in;          // channel c0 of sample 0 of the input blob
  int ctot, C, IH, IW;      // channels of the blob / of the slice, input map
  int OW;                   // width of the pixel space the tile runs over
  long long OP;             // its pixels
  int k, s, pad;
  unsigned ow_magic, s_magic;   // div_magic(OW), div_magic(s)
};

// n / d for 0 <= n < 2^32 without an integer division: with m = div_magic(d) = floor((2^32 - 1) / d), umulhi(n, m) is the quotient or one
// below it (m d = 2^32 - e with 1 <= e <= d, so n m / 2^32 lies in (n / d - 1, n / d]); one correction step makes it exact
inline unsigned div_magic(int d) { return 0xffffffffu / (unsigned)d; }

__device__ __forceinline__ void divmod(unsigned n, unsigned d, unsigned magic, unsigned& q, unsigned& r) {
  q = __umulhi(n, magic);
  r = n - q * d;
  if (r >= d) { ++q; r -= d; }
}

// the pixel of a thread in its tile, as the gather needs it: forward (y s - pad, x s - pad), transposed (y + pad, x + pad)
struct PixelBase { int by, bx; bool valid; };

template <bool TR>
__device__ __forceinline__ PixelBase pixel_base(const GatherSrc& a, long long p) {
  PixelBase b;
  b.valid = p < a.OP;
  unsigned uy, ux;
  divmod(b.valid ? (unsigned)p : 0u, (unsigned)a.OW, a.ow_magic, uy, ux);
  const int y = (int)uy, x = (int)ux;
  b.by = TR ? y + a.pad : y * a.s - a.pad;
  b.bx = TR ? x + a.pad : x * a.s - a.pad;
  return b;
}

// A k-row as (channel, ky, kx), wave-uniform: decomposed once, then advanced by a constant number of rows per chunk with two carries
// instead of two divisions
struct KRow { int c, ky, kx; };
struct KStep { int dc, dky, dkx; };

__device__ __forceinline__ KRow k_row(int kg, int k) {
  const int kk = k * k;
  KRow r;
  r.c = kg / kk;
  const int tap = kg - r.c * kk;
  r.ky = tap / k;
  r.kx = tap - r.ky * k;
  return r;
}

__device__ __forceinline__ KStep k_step(int rows, int k) {
  const KRow r = k_row(rows, k);
  return KStep{r.c, r.ky, r.kx};
}

__device__ __forceinline__ void k_advance(KRow& r, const KStep& d, int k) {
  r.kx += d.dkx;
  if (r.kx >= k) { r.kx -= k; ++r.ky; }
  r.ky += d.dky;
  if (r.ky >= k) { r.ky -= k; ++r.c; }
  r.c += d.dc;
}

// col[k-row][pixel] of sample slice `src`; 0 outside the image, beyond K and for a pixel beyond the tile's map
template <bool TR>
__device__ __forceinline__ float gather_one(const GatherSrc& a, const float* src, const KRow& kr, const PixelBase& b) {
  int yi, xi;
  bool ok = b.valid && kr.c < a.C;
  if constexpr (TR) {
    const int ty = b.by - kr.ky, tx = b.bx - kr.kx;
    unsigned qy, ry, qx, rx;
    divmod((unsigned)max(ty, 0), (unsigned)a.s, a.s_magic, qy, ry);
    divmod((unsigned)max(tx, 0), (unsigned)a.s, a.s_magic, qx, rx);
    yi = (int)qy; xi = (int)qx;
    ok = ok && ty >= 0 && tx >= 0 && ry == 0 && rx == 0 && yi < a.IH && xi < a.IW;
  } else {
    yi = b.by + kr.ky; xi = b.bx + kr.kx;
    ok = ok && yi >= 0 && yi < a.IH && xi >= 0 && xi < a.IW;
  }
  float v = 0.f;
  if (ok) v = src[(size_t)kr.c * a.IH * a.IW + (size_t)yi * a.IW + xi];
  return v;
}

// ------------------------------------------------------------------------------------------------ the two gather kernels
struct GatherArgs {
  GatherSrc g;
  const float* wp;          // packed operand
  const float* bias;
  float* out;               // channel c0 of sample 0 of the output blob
  int out_ctot, M, G, ksteps, ptiles, mblocks;
  int relu;
  float slope;
};

template <bool TR, int NG>
__global__ __launch_bounds__(kThreads) void conv_general_gather(GatherArgs a) {
  __shared__ float col[kKC * kColStrideG];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned task = blockIdx.x;
  const int mb = task % a.mblocks; task /= a.mblocks;
  const int pt = task % a.ptiles;
  const int n = task / a.ptiles;
  const long long p0 = (long long)pt * kPix;
  const size_t iplane = (size_t)a.g.IH * a.g.IW;
  const float* src = a.g.in + (size_t)n * a.g.ctot * iplane;
  const PixelBase pb = pixel_base<TR>(a.g, p0 + lane);

  // this wave's NG weight groups; beyond the last real group the last one again (computed, not stored)
  const float* wl[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int g = min(NG * mb + j, a.G - 1);
    wl[j] = a.wp + (size_t)g * a.ksteps * 64 + lane;
  }
  f32x4 acc[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = a.ksteps / 4;
  const KStep kstep = k_step(kKC, a.g.k);
  KRow kr[4];
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    kr[i] = k_row(wave + 4 * i, a.g.k);
    v[i] = gather_one<TR>(a.g, src, kr[i], pb);
  }
  // the weight operand of a chunk (4 k-steps x NG groups) is fetched a chunk ahead, like the col values
  float w[4][NG];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int j = 0; j < NG; ++j) w[ks][j] = wl[j][(size_t)ks * 64];
  const int arow = (lane >> 4) * kColStrideG + 16 * wave + (lane & 15);
  for (int ch = 0; ch < nchunks; ++ch) {
#pragma unroll
    for (int i = 0; i < 4; ++i) col[(wave + 4 * i) * kColStrideG + lane] = v[i];
    __syncthreads();
    // the next chunk's loads fly during this chunk's MFMAs (col beyond K: zeros, nothing is loaded; weights: the last chunk again)
    float wn[4][NG];
    const int nx = min(ch + 1, nchunks - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < NG; ++j) wn[ks][j] = wl[j][(size_t)(4 * nx + ks) * 64];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      k_advance(kr[i], kstep, a.g.k);
      v[i] = gather_one<TR>(a.g, src, kr[i], pb);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float av = col[arow + 4 * ks * kColStrideG];
#pragma unroll
      for (int j = 0; j < NG; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[ks][j], acc[j], 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < NG; ++j) w[ks][j] = wn[ks][j];
  }

  // lane (pixel quad lane >> 4, channel lane & 15) holds 4 consecutive pixels of one channel
  const long long p = p0 + 16 * wave + 4 * (lane >> 4);
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int co = 16 * (NG * mb + j) + (lane & 15);
    if (co >= a.M || p >= a.g.OP) continue;
    const float bv = a.bias ? a.bias[co] : 0.f;
    const f32x4 r = mfma::bias_relu4(acc[j], bv, a.relu, a.slope);
    float* o = a.out + ((size_t)n * a.out_ctot + co) * (size_t)a.g.OP + p;
    if (p + 3 < a.g.OP && (reinterpret_cast<uintptr_t>(o) & 15) == 0) *reinterpret_cast<f32x4*>(o) = r;
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (p + e < a.g.OP) o[e] = r[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct WgradArgs {
  GatherSrc g;              // the forward gather of the L blob over the S pixel space
  const float* x;           // channel c0 of sample 0 of the S blob
  int x_ctot, A, G, ablocks, ktiles, ptiles;
  long long chunks, per_part, Kpad;
  float* ws;                // [nsplit][16 G][Kpad]
};

// the values of a thread for pixel chunk q: 4 of the col tile (k-rows kr) and 16 of the S blob (channels ch0, ch0 + 4, ...)
__device__ __forceinline__ void wgrad_fetch(const WgradArgs& a, const KRow (&kr)[4], long long q, int ch0, int lane, float (&cv)[4], float (&xv)[16]) {
  const int n = (int)(q / a.ptiles);
  const long long p = (q - (long long)n * a.ptiles) * kPix + lane;
  const float* src = a.g.in + (size_t)n * a.g.ctot * a.g.IH * a.g.IW;
  const PixelBase pb = pixel_base<false>(a.g, p);
#pragma unroll
  for (int i = 0; i < 4; ++i) cv[i] = gather_one<false>(a.g, src, kr[i], pb);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int ch = ch0 + 4 * i;
    xv[i] = (ch < a.A && pb.valid) ? a.x[((size_t)n * a.x_ctot + ch) * (size_t)a.g.OP + p] : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void conv_general_wgrad(WgradArgs a) {
  __shared__ float col[kKC * kColStrideW];
  __shared__ float xs[64 * kColStrideW];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned task = blockIdx.x;
  const int kt = task % a.ktiles; task /= a.ktiles;
  const int ab = task % a.ablocks;
  const int part = task / a.ablocks;
  const long long q0 = (long long)part * a.per_part, q1 = min(q0 + a.per_part, a.chunks);
  const bool active = 4 * ab + wave < a.G;          // a wave beyond the last channel group only helps staging

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  float cv[4], xv[16];
  KRow kr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) kr[i] = k_row(kt * kKC + wave + 4 * i, a.g.k);
  // chunk q's values are fetched while chunk q - 1 is multiplied (the last chunk of the part is fetched twice: no branch)
  wgrad_fetch(a, kr, q0, 64 * ab + wave, lane, cv, xv);
  for (long long q = q0; q < q1; ++q) {
    __syncthreads();      // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) col[(wave + 4 * i) * kColStrideW + lane] = cv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) xs[(wave + 4 * i) * kColStrideW + lane] = xv[i];
    __syncthreads();
    wgrad_fetch(a, kr, min(q + 1, q1 - 1), 64 * ab + wave, lane, cv, xv);
    if (active) {
      const float* xr = xs + (16 * wave + (lane & 15)) * kColStrideW + (lane >> 4);
      const float* cr = col + (lane & 15) * kColStrideW + (lane >> 4);
#pragma unroll
      for (int st = 0; st < kPix / 4; ++st) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[4 * st], cr[4 * st], acc, 0, 0, 0);
    }
  }
  if (active) {
    // lane holds channels 16 g + 4 (lane >> 4) + r of k-column 16 kt + (lane & 15)
    float* o = a.ws + ((size_t)part * (16 * a.G) + 16 * (4 * ab + wave) + 4 * (lane >> 4)) * (size_t)a.Kpad + (size_t)kt * kKC + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(size_t)r * a.Kpad] = acc[r];
  }
}

// weight_diff[a][k] (+)= the parts in part order
__global__ void conv_general_wgrad_finalize(const float* ws, float* dw, int A, long long K, long long Kpad, int rows, int nsplit, int accumulate) {
  const long long total = (long long)A * K;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long ch = i / K, k = i - ch * K;
    float s = ws[ch * Kpad + k];
    for (int part = 1; part < nsplit; ++part) s += ws[((long long)part * rows + ch) * Kpad + k];
    dw[i] = accumulate ? dw[i] + s : s;
  }
}

// bias_diff[c] (+)= sum over (n, pixels) of diff[n][c][.]: thread t adds elements t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(kThreads) void conv_general_bias_grad(const float* diff, int ctot, int N, long long P, float* db, int accumulate) {
  __shared__ float part[kThreads];
  const int c = blockIdx.x;
  const long long total = (long long)N * P;
  float s = 0.f;
  for (long long i = threadIdx.x; i < total; i += kThreads) {
    const long long n = i / P, p = i - n * P;
    s += diff[((size_t)n * ctot + c) * (size_t)P + p];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) db[c] = accumulate ? db[c] + part[0] : part[0];
}

// ------------------------------------------------------------------------------------------------ packing
// W [Cs][Cl][kk] -> Wp[g][ks][lane]; swapped: rows are Cl (the transposed gather), else Cs
__global__ void conv_general_pack(const float* w, float* wp, int M, int R, int kk, long long K, int ksteps, long long total, int swapped) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    const long long r = i >> 6;
    const int ks = (int)(r % ksteps), g = (int)(r / ksteps);
    const int m = 16 * g + (lane & 15);
    const long long kg = 4ll * ks + (lane >> 4);
    float v = 0.f;
    if (m < M && kg < K) {
      const long long c = kg / kk, tap = kg - c * kk;
      v = swapped ? w[(c * M + m) * kk + tap] : w[(long long)m * K + kg];
    }
    wp[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------ host entry helpers
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

int run_gather(const Sides& g, bool tr, const float* in, int in_ctot, int in_c0, const float* packed, const float* bias, float* out, int out_ctot,
               int out_c0, int relu, float slope, hipStream_t st) {
  const Gemm m = pass_gemm(g, tr);
  GatherArgs a;
  const int IH = tr ? g.Hs : g.Hl, IW = tr ? g.Ws : g.Wl, OH = tr ? g.Hl : g.Hs, OW = tr ? g.Wl : g.Ws;
  a.g.in = in + (size_t)in_c0 * IH * IW;
  a.g.ctot = in_ctot; a.g.C = m.R; a.g.IH = IH; a.g.IW = IW; a.g.OW = OW; a.g.OP = (long long)OH * OW;
  a.g.k = g.k; a.g.s = g.s; a.g.pad = g.pad;
  a.g.ow_magic = div_magic(OW); a.g.s_magic = div_magic(g.s);
  a.wp = packed; a.bias = bias;
  a.out = out + (size_t)out_c0 * a.g.OP;
  a.out_ctot = out_ctot; a.M = m.M; a.G = m.G; a.ksteps = m.ksteps;
  const int ng = groups_per_block(m.G);
  a.ptiles = (int)cdivll(a.g.OP, kPix); a.mblocks = (m.G + ng - 1) / ng;
  a.relu = relu; a.slope = slope;
  const long long tiles = gather_tiles(g, tr, m, ng);
  if (tiles > kMaxTiles) return fail(FN2_ERR_UNSUPPORTED, "fn2_conv_general: grid too large");
  const dim3 grid((unsigned)tiles), block(kThreads);
#define FN2_GATHER(TR_, NG_) hipLaunchKernelGGL((conv_general_gather<TR_, NG_>), grid, block, 0, st, a)
  if (tr) { if (ng == 1) FN2_GATHER(true, 1); else if (ng == 2) FN2_GATHER(true, 2); else FN2_GATHER(true, 4); }
  else { if (ng == 1) FN2_GATHER(false, 1); else if (ng == 2) FN2_GATHER(false, 2); else FN2_GATHER(false, 4); }
#undef FN2_GATHER
  return check_launch("fn2_conv_general");
}

int check_slices(const char* what, const fn2_conv_desc* d, int bottom_channels, int bottom_c0, int top_channels, int top_c0) {
  if (bottom_c0 < 0 || bottom_channels < 1 || (long long)bottom_c0 + d->Cin > bottom_channels || top_c0 < 0 || top_channels < 1 ||
      (long long)top_c0 + d->Cout > top_channels)
    return fail(FN2_ERR_INVALID_ARG, "%s: channel slice outside the blob", what);
  return FN2_OK;
}

int refuse(const char* what, const fn2_conv_desc* d, int transposed) {
  if (!d) return fail(FN2_ERR_UNSUPPORTED, "%s: null descriptor", what);
  return fail(FN2_ERR_UNSUPPORTED, "%s: no kernel for %s N=%d Cin=%d %dx%d Cout=%d kernel=%d stride=%d pad=%d (invalid, empty output, or beyond the 32-bit index limits)",
              what, transposed ? "Deconvolution" : "Convolution", d->N, d->Cin, d->Hin, d->Win, d->Cout, d->kernel, d->stride, d->pad);
}

}  // namespace
}  // namespace fn2

using namespace fn2;

FN2_API int fn2_conv_general_supported(const fn2_conv_desc* desc, int transposed) {
  Sides g;
  return supported(desc, transposed, g) ? 1 : 0;
}

FN2_API int fn2_debug_set_conv_general_groups(int groups) {
  if (groups != 0 && groups != 1 && groups != 2 && groups != 4)
    return fail(FN2_ERR_INVALID_ARG, "fn2_debug_set_conv_general_groups: %d (0 = by geometry, 1, 2 or 4)", groups);
  forced_groups() = groups;
  return FN2_OK;
}

FN2_API int fn2_conv_general_sizes(const fn2_conv_desc* desc, int transposed, size_t* forward_packed, size_t* backward_data_packed,
                                   size_t* backward_weights_packed, size_t* backward_weights_workspace) {
  if (forward_packed) *forward_packed = 0;
  if (backward_data_packed) *backward_data_packed = 0;
  if (backward_weights_packed) *backward_weights_packed = 0;
  if (backward_weights_workspace) *backward_weights_workspace = 0;
  Sides g;
  if (!supported(desc, transposed, g)) return refuse("fn2_conv_general_sizes", desc, transposed);
  if (forward_packed) *forward_packed = packed_floats(pass_gemm(g, pass_is_tr(transposed, 0)));
  if (backward_data_packed) *backward_data_packed = packed_floats(pass_gemm(g, pass_is_tr(transposed, 1)));
  if (backward_weights_workspace) *backward_weights_workspace = make_wgrad(g).workspace_bytes;
  return FN2_OK;
}

FN2_API int fn2_conv_general_pack_weights(const fn2_conv_desc* desc, int transposed, int pass, const float* weight, float* packed, void* stream) {
  Sides g;
  if (!supported(desc, transposed, g)) return refuse("fn2_conv_general_pack_weights", desc, transposed);
  if (pass < 0 || pass > 2) return fail(FN2_ERR_INVALID_ARG, "fn2_conv_general_pack_weights: pass %d (0 forward, 1 data gradient, 2 weight gradient)", pass);
  if (pass == 2) return FN2_OK;      // the weight gradient has no weight operand
  if (!weight || !packed) return fail(FN2_ERR_INVALID_ARG, "fn2_conv_general_pack_weights: null blob");
  if (misaligned(weight) || misaligned(packed)) return fail(FN2_ERR_INVALID_ARG, "fn2_conv_general_pack_weights: blobs must be 4-byte aligned");
  const bool tr = pass_is_tr(transposed, pass);
  const Gemm m = pass_gemm(g, tr);
  const long long total = (long long)packed_floats(m);
  hipLaunchKernelGGL(conv_general_pack, dim3(blocks_for(total, 256)), dim3(256), 0, as_stream(stream), weight, packed, m.M, m.R, g.k * g.k, m.K,
                     m.ksteps, total, tr ? 1 : 0);
  return check_launch("fn2_conv_general_pack_weights");
}

FN2_API int fn2_conv_general_forward(const fn2_conv_desc* desc, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                     const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                                     int relu, float negative_slope, void* stream) {
  const char* what = "fn2_conv_general_forward";
  Sides g;
  if (!supported(desc, transposed, g)) return refuse(what, desc, transposed);
  if (!bottom || !packed_weight || !top) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (const int rc = check_slices(what, desc, bottom_channels, bottom_c0, top_channels, top_c0)) return rc;
  if (misaligned(bottom) || misaligned(packed_weight) || misaligned(top) || misaligned(bias))
    return fail(FN2_ERR_INVALID_ARG, "%s: blobs must be 4-byte aligned", what);
  return run_gather(g, pass_is_tr(transposed, 0), bottom, bottom_channels, bottom_c0, packed_weight, bias, top, top_channels, top_c0, relu,
                    negative_slope, as_stream(stream));
}

FN2_API int fn2_conv_general_backward_data(const fn2_conv_desc* desc, int transposed, const float* top_diff, int top_channels, int top_c0,
                                           const float* packed_weight, float* bottom_diff, int bottom_channels, int bottom_c0, void* stream) {
  const char* what = "fn2_conv_general_backward_data";
  Sides g;
  if (!supported(desc, transposed, g)) return refuse(what, desc, transposed);
  if (!top_diff || !packed_weight || !bottom_diff) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (const int rc = check_slices(what, desc, bottom_channels, bottom_c0, top_channels, top_c0)) return rc;
  if (misaligned(top_diff) || misaligned(packed_weight) || misaligned(bottom_diff)) return fail(FN2_ERR_INVALID_ARG, "%s: blobs must be 4-byte aligned", what);
  return run_gather(g, pass_is_tr(transposed, 1), top_diff, top_channels, top_c0, packed_weight, nullptr, bottom_diff, bottom_channels, bottom_c0, 0,
                    0.f, as_stream(stream));
}

FN2_API int fn2_conv_general_backward_weights(const fn2_conv_desc* desc, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                              const float* top_diff, int top_channels, int top_c0, float* weight_diff, float* bias_diff,
                                              int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "fn2_conv_general_backward_weights";
  Sides g;
  if (!supported(desc, transposed, g)) return refuse(what, desc, transposed);
  if (!bottom || !top_diff || !weight_diff) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (const int rc = check_slices(what, desc, bottom_channels, bottom_c0, top_channels, top_c0)) return rc;
  if (misaligned(bottom) || misaligned(top_diff) || misaligned(weight_diff) || misaligned(bias_diff) || misaligned(workspace))
    return fail(FN2_ERR_INVALID_ARG, "%s: blobs must be 4-byte aligned", what);
  const WgradPlan p = make_wgrad(g);
  if (!workspace || workspace_bytes < p.workspace_bytes)
    return fail(FN2_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", what, p.workspace_bytes, workspace ? workspace_bytes : (size_t)0);
  hipStream_t st = as_stream(stream);
  // the S blob multiplies the forward gather of the L blob
  const float* sblob = transposed ? bottom : top_diff;
  const int s_ctot = transposed ? bottom_channels : top_channels, s_c0 = transposed ? bottom_c0 : top_c0;
  const float* lblob = transposed ? top_diff : bottom;
  const int l_ctot = transposed ? top_channels : bottom_channels, l_c0 = transposed ? top_c0 : bottom_c0;
  WgradArgs a;
  a.g.in = lblob + (size_t)l_c0 * g.Hl * g.Wl;
  a.g.ctot = l_ctot; a.g.C = g.Cl; a.g.IH = g.Hl; a.g.IW = g.Wl; a.g.OW = g.Ws; a.g.OP = (long long)g.Hs * g.Ws;
  a.g.k = g.k; a.g.s = g.s; a.g.pad = g.pad;
  a.g.ow_magic = div_magic(g.Ws); a.g.s_magic = div_magic(g.s);
  a.x = sblob + (size_t)s_c0 * a.g.OP;
  a.x_ctot = s_ctot; a.A = g.Cs; a.G = p.m.G; a.ablocks = (p.m.G + 3) / 4; a.ktiles = (int)(p.m.Kpad / kKC); a.ptiles = p.ptiles;
  a.chunks = p.chunks; a.per_part = p.per_part; a.Kpad = p.m.Kpad;
  a.ws = static_cast<float*>(workspace);
  hipLaunchKernelGGL(conv_general_wgrad, dim3((unsigned)p.tiles), dim3(kThreads), 0, st, a);
  if (const int rc = check_launch(what)) return rc;
  hipLaunchKernelGGL(conv_general_wgrad_finalize, dim3(blocks_for((long long)g.Cs * p.m.K, 256)), dim3(256), 0, st, a.ws, weight_diff, g.Cs, p.m.K,
                     p.m.Kpad, 16 * p.m.G, p.nsplit, accumulate);
  if (const int rc = check_launch(what)) return rc;
  if (bias_diff) {
    const long long Pt = transposed ? (long long)g.Hl * g.Wl : (long long)g.Hs * g.Ws;
    hipLaunchKernelGGL(conv_general_bias_grad, dim3((unsigned)desc->Cout), dim3(kThreads), 0, st, top_diff + (size_t)top_c0 * Pt, top_channels, g.N, Pt,
                       bias_diff, accumulate);
    if (const int rc = check_launch(what)) return rc;
  }
  return FN2_OK;
}
