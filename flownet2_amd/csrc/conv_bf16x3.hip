// Direct convolution (Convolution{kernel_size KS, stride S, pad} + bias + ReLU{negative_slope}) in SPLIT-bf16 ("bf16x3") arithmetic on
// v_mfma_f32_16x16x32_bf16: an opt-in second arithmetic for the layers of csrc/conv_mfma.hip (instantiated for 5x5 / 2, the encoders'
// conv2 / conv3), same blob conventions: NCHW in and out, channel slices on both blobs, zero padding by out-of-range buffer loads, one
// launch per mini-batch, no workspace and no second pass over global memory (no pre-split copy of the activations).
//
// Arithmetic.  Every fp32 value v is cut into three bf16 pieces  h = rne(v), m = rne(v - h), l = rne(v - h - m)  (v_cvt_pk_bf16_f32 and
// plain subtractions; both differences are exact, h + m + l == v for every normal v with 24 significant bits).  Of the nine piece
// products of x * w the six leading ones are formed -- each exact in fp32 (8 x 8 significant bits) -- and summed in fp32:
//     x * w ~ mm + lh + hl + mh + hm + hh          (first letter: the activation's piece; the dropped ml, lm, ll are < 2^-24 |x w|)
// Per output element the summation order is FIXED: k-steps in the order (chunk of 8 input channels, k-step of 4 taps), and inside a
// k-step the six MFMAs in the order above on ONE accumulator (small terms first).  It does not depend on the tile variant, the batch or
// the run, so the result is bit-reproducible, a sample has the bits it has alone, and every variant writes the same bits.  It is NOT
// bit-identical to the exact kernel (another summation order, 3 products dropped); it meets that kernel's fp64 bound, 4e-6 x scale
// (measured: 0.09 - 0.45 of it, tests/test_conv_bf16x3.py).
// Non-finite inputs: Inf splits into (inf, nan, nan), NaN into (nan, nan, nan), so an output whose window covers an Inf or a NaN is
// non-finite -- possibly NaN where the exact kernel gives Inf.  Outputs whose window covers no such pixel are unaffected: the padding
// slots of a k-step (below) re-read a pixel of the output's OWN window against a zero weight.
//
// GEMM view.  As conv_mfma: output pixels in 4x4 patches (M tile), output channels in groups of 16 (N tile).  A k-step is 32 k values =
// 8 input channels x 4 taps: lane (pixel p, kq = lane >> 4) holds, for j = 0 .. 7, channel 8 chunk + j at tap 4 t + kq of the KS * KS
// taps in (ky, kx) order; taps >= KS * KS (5x5: 3 of 28) carry zero weights and read the pixel of one of the last two taps.
//   * pixel operand: the fp32 window of a workgroup tile for 8 channels arrives by LDS-DMA as in conv_mfma (mfma_tile.hpp), then the
//     workgroup splits it ONCE into a bf16 image [piece][row][column][8 channels] (16 bytes per pixel and piece), so that a lane's
//     operand of a tap is one ds_read_b128 per piece and every window element is converted once, not once per tap that reads it.
//     One fp32 stage and one image: barrier -> split -> barrier -> (DMA of the next chunk into the stage) + MFMAs from the image.
//   * weight operand: split once when packed (fn2::conv_bf16x3_pack_weights): the packed layout of
//     split_bf16.hpp with groups of 16 output channels, fetched a k-step ahead.
//   * wave tile MW channel groups x NP patches, workgroup WM x WNX x WNY waves, epilogue as conv_mfma (store_row4).
// Build figures (hipcc -O3, gfx950; __launch_bounds__(256, 2) allows 256 registers): variant 0 (32x4-pixel tile) 124 VGPRs, 70,848 bytes of
// LDS; variant 1 (16x8) 126 VGPRs, 72,896 bytes; no spills, two workgroups per CU (LDS), four waves per SIMD by registers.
#include "conv_internal.hpp"
#include "mfma_tile.hpp"
#include "split_bf16.hpp"

namespace fn2 {
namespace cx {

using namespace mfma;
using namespace bf16x3;      // the toolkit of split_bf16.hpp

struct Args {
  const float* in; const u32x4* wp; const float* bias; float* out;
  int N, Cin, Hin, Win, in_ctot, in_c0;
  int Cout, Hout, Wout, out_ctot, out_c0;
  int pad;
  int nchunks;        // chunks of 8 input channels
  int kalloc;         // k-steps of the packed weights per 16-channel group, the spare one included
  int tx, ty;         // workgroup tiles per sample along x / y
  int ng;             // Cout / (16 * MW * WM)
  unsigned total;     // tiles = workgroups
  float slope; int relu;
};

template <int KS_, int S_, int MW_, int NP_, int WM_, int WNX_, int WNY_>
struct Cfg : Window<(4 * WNY_ - 1) * S_ + KS_, (4 * NP_ * WNX_ - 1) * S_ + KS_ + 4, 2, WM_ * WNX_ * WNY_> {      // 2 channel quads = the 8 channels of a chunk
  static constexpr int KS = KS_, S = S_, MW = MW_, NP = NP_, WM = WM_, WNX = WNX_, WNY = WNY_;
  static constexpr int NW = WM * WNX * WNY, THREADS = 64 * NW;
  static constexpr int PADL = 4;                                     // window columns left of S * x0 (16-byte aligned start)
  static constexpr int TW = 4 * NP * WNX, TH = 4 * WNY;              // output pixels of a workgroup tile
  static constexpr int TAPS = KS * KS, KST = cdiv(TAPS, 4);          // k-steps per chunk
  // bf16 image: 16 bytes per pixel and piece, rows of WCP == 4 (mod 8) pixels.  A ds_read_b128 is served in groups of 16 lanes = two patch
  // rows at tap T and two at tap T + 1; with this row stride the stride-2 pixels of the first pair take the even 16-byte slots of the
  // 256-byte bank row and those of the second pair (one column on) the odd ones: no conflict unless T + 1 starts a new tap row
  static constexpr int WCP = up_mod(Cfg::WC, 4, 8);
  static constexpr int PIX = Cfg::WR * WCP;
  static constexpr int LDS_BYTES = 4 * Cfg::BUF + 3 * 16 * PIX;      // fp32 stage + image
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
  static_assert(3 * 16 * PIX < 65536, "the piece planes are reached by ds_read immediates");
};

constexpr int kstep_alloc(int Cin, int KS) { return cdiv(Cin, 8) * cdiv(KS * KS, 4) + 1; }      // + 1: the weight fetch runs a k-step ahead

template <class K>
__device__ __forceinline__ void conv_body(const Args& a, int g, int bx, int by, int n) {
  static_assert(K::THREADS == 256, "launch bounds");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int KS = K::KS, S = K::S, MW = K::MW, NP = K::NP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % K::WM, wnx = (wave / K::WM) % K::WNX, wny = wave / (K::WM * K::WNX);
  const int x0 = bx * K::TW, y0 = by * K::TH;
  u32x4* const img = reinterpret_cast<u32x4*>(smem + K::BUF);       // [piece][row][column]

  // ---- LDS-DMA plan of the fp32 stage (mfma_tile.hpp); chunk c adds 8 planes to every in-image offset
  const size_t plane = (size_t)a.Hin * a.Win;
  const __amdgpu_buffer_rsrc_t rs = nchw_rsrc(a.in, n, a.in_ctot, a.in_c0, a.Cin, plane);
  unsigned voff[K::RPW];
  window_plan<K>(voff, wave, lane, S * y0 - a.pad, S * x0 - K::PADL, a.Hin, a.Win, plane);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)smem;
  const unsigned chunk_bytes = 4u * 8u * (unsigned)plane;
  const ChunkStage<K> stage{rs, voff, chunk_bytes, lds_base, wave};

  // ---- operands
  const int kq = lane >> 4, py = (lane & 15) >> 2, px = lane & 3;
  const int abase = (S * (4 * wny + py)) * K::WCP + S * (4 * NP * wnx + px) + K::PADL - a.pad;        // image pixel of tap (0, 0) of patch 0
  int tapoff[K::KST];
#pragma unroll
  for (int t = 0; t < K::KST; ++t) {
    int T = 4 * t + kq;                                             // padding slots (zero weight): one of the last two taps' pixels, a column
    if (T >= K::TAPS) T = ((kq & 1) && T - 1 >= K::TAPS) ? K::TAPS - 1 : K::TAPS - 2;      // away from the slot read with it (kq ^ 1)
    tapoff[t] = abase + (T / KS) * K::WCP + T % KS;
  }
  const int cg0 = (g * K::WM + wm) * MW;                            // first 16-channel group of this wave
  const u32x4* wl = packed_lane(a.wp, cg0, a.kalloc, lane);         // group cg0 + j, k-step ks: load_pieces(wl, j kalloc + ks, ..)

  f32x4 acc[MW][NP];
#pragma unroll
  for (int j = 0; j < MW; ++j)
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[j][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 w[MW][3], wn[MW][3];
  stage(0);
#pragma unroll
  for (int j = 0; j < MW; ++j) load_pieces(wl, (size_t)j * a.kalloc, wn[j]);

  for (int c = 0; c < a.nchunks; ++c) {
    wait_vmcnt<0>();                     // this wave's part of the stage has landed
    __syncthreads();                     // ... everyone's; and every wave is done with the image of chunk c - 1
    // ---- split the stage into the bf16 image: one pixel (8 channels) per thread and pass
#pragma unroll
    for (int it = 0; it < cdiv(K::WR * K::WC, 256); ++it) {
      const int i = it * 256 + tid;
      if (i < K::WR * K::WC) {
        const int row = i / K::WC, col = i % K::WC, idx = row * K::WCP + col;
        const float* s = smem + row * K::RS + col;
        float v[8];
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) v[ch] = s[ch * K::CS];
        store_pieces(img + idx, K::PIX, v);
      }
    }
    __syncthreads();                     // the image is whole, the stage is free
    if (c + 1 < a.nchunks) stage(c + 1);
#pragma unroll
    for (int t = 0; t < K::KST; ++t) {
      const int ks = c * K::KST + t;
#pragma unroll
      for (int j = 0; j < MW; ++j) {
#pragma unroll
        for (int q = 0; q < 3; ++q) w[j][q] = wn[j][q];
        load_pieces(wl, (size_t)j * a.kalloc + ks + 1, wn[j]);                  // (the packed array carries a spare k-step per group)
      }
      u32x4 x[NP][3];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) x[p][q] = img[q * K::PIX + tapoff[t] + 4 * S * p];
      // the six products, small terms first: (activation piece, weight piece) = mm, lh, hl, mh, hm, hh
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < MW; ++j)
#pragma unroll
          for (int p = 0; p < NP; ++p)
            acc[j][p] = piece_mfma_16x16x32(i, x[p], w[j], acc[j][p]);
    }
  }

  // ---- epilogue: lane (row block = lane >> 4, channel = lane & 15) holds 4 consecutive x of output row y0 + 4 wny + (lane >> 4)
  const int y = y0 + 4 * wny + (lane >> 4);
  if (y < a.Hout) {
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      const int co = 16 * (cg0 + j) + (lane & 15);
      const float bv = a.bias ? a.bias[co] : 0.f;
      float* orow = a.out + (((size_t)n * a.out_ctot + a.out_c0 + co) * a.Hout + y) * a.Wout;
#pragma unroll
      for (int p = 0; p < NP; ++p) store_row4(orow, x0 + 4 * (NP * wnx + p), a.Wout, acc[j][p], bv, a.relu, a.slope);
    }
  }
}

// Task list: (sample, tile row, tile column, channel group), channel group fastest (xcd_task: neighbours share an input window)
template <class K>
__global__ void __launch_bounds__(256, 2)
conv_bf16x3(Args a) {
  unsigned t;
  if (!xcd_task(blockIdx.x, a.total, t)) return;
  const int g = t % a.ng; t /= a.ng;
  const int bx = t % a.tx; t /= a.tx;
  conv_body<K>(a, g, bx, (int)(t % a.ty), (int)(t / a.ty));
}

// weight [Cout][Cin][KS][KS] -> the packed layout of split_bf16.hpp, groups of 16 output channels
__global__ void __launch_bounds__(256) pack_weights(const float* __restrict__ wsrc, u32x4* __restrict__ wp, int Cout, int Cin, int KS, int kalloc) {
  int lane, ks, grp;
  if (!pack_thread(Cout / 16, kalloc, lane, ks, grp)) return;
  const int kst = cdiv(KS * KS, 4), chunk = ks / kst, tap = 4 * (ks % kst) + (lane >> 4), co = 16 * grp + (lane & 15);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = 8 * chunk + j;
    v[j] = (ks < kalloc - 1 && tap < KS * KS && ci < Cin) ? wsrc[((size_t)co * Cin + ci) * KS * KS + tap] : 0.f;
  }
  u32x4 h, m, l;                    // (store_pieces, written out: through the helper this kernel allocates other registers)
  split8(v, h, m, l);
  u32x4* dst = wp + ((size_t)grp * kalloc + ks) * kStepVecs + lane;
  dst[0] = h; dst[kPieceVecs] = m; dst[2 * kPieceVecs] = l;
}

template <class K>
static int launch(const Args& base, hipStream_t st) {
  Args a = base;
  a.tx = cdiv(a.Wout, K::TW); a.ty = cdiv(a.Hout, K::TH);
  a.ng = a.Cout / (16 * K::MW * K::WM);
  a.nchunks = cdiv(a.Cin, 8);
  return launch_tiles<&conv_bf16x3<K>>(a, (long long)a.N * a.tx * a.ty * a.ng, K::THREADS, K::LDS_BYTES, "conv_bf16x3", "conv_bf16x3_forward", st);
}

struct Variant {
  int ks, s, mw, np, wm, wnx, wny;
  int (*fn)(const Args&, hipStream_t);
};

#define FN2_CX_ROW(KS, S, MW, NP, WM, WNX, WNY) {KS, S, MW, NP, WM, WNX, WNY, &launch<Cfg<KS, S, MW, NP, WM, WNX, WNY>>},
// 5x5 stride 2: 32x4- and 16x8-pixel tiles of 64 channels, two workgroups per CU.  (Measured and dropped: a 56x4-pixel tile with NP = 7 --
// 110 KB of LDS, one workgroup per CU, which then idles through every split and barrier: 478 / 548 us where these take 308 / 334.)
static const Variant kVariants[] = {FN2_CX_ROW(5, 2, 2, 4, 2, 2, 1) FN2_CX_ROW(5, 2, 2, 4, 2, 1, 2)};
FN2_BF16X3_VARIANT_KNOBS(conv_bf16x3)

static bool variant_applies(const Variant& v, const Args& a, int KS, int S) {
  return v.ks == KS && v.s == S && a.Win % 4 == 0 && a.Cout % (16 * v.mw * v.wm) == 0;
}

// Cost model: rounds of workgroups over the 512 slots of the chip (tiles hanging over the image edge included) x accumulator tiles of a
// wave; the taller tile first among equals (it re-reads fewer window columns: the faster one on conv2 and conv3)
static double variant_cost(const Variant& v, const Args& a) {
  const long long wgs = (long long)a.N * cdiv(a.Wout, 4 * v.np * v.wnx) * cdiv(a.Hout, 4 * v.wny) * (a.Cout / (16 * v.mw * v.wm));
  return (double)((wgs + 511) / 512) * v.mw * v.np * (v.wny > 1 ? 1.0 : 1.05);
}

bool geometry_ok(int Cin, int Hin, int Win, int Cout, int kernel, int stride, int pad) {
  if (kernel != 5 || stride != 2 || pad != 2) return false;           // the instantiated geometry; the kernel is a template on (KS, S)
  if (!fn2_conv_mfma_supported(Cin, Hin, Win, Cout, kernel, stride, pad)) return false;
  Args a{};
  a.Win = Win; a.Cout = Cout;
  for (int i = 0; i < kNumVariants; ++i)
    if (variant_applies(kVariants[i], a, kernel, stride)) return true;
  return false;
}

}  // namespace cx

size_t conv_bf16x3_packed_floats(int Cout, int Cin, int kernel) {
  if (Cout <= 0 || Cout % 16 != 0 || Cin <= 0 || kernel <= 0) return 0;
  return bf16x3::packed_floats(Cout / 16, cx::kstep_alloc(Cin, kernel));
}

int conv_bf16x3_pack_weights(const float* weight, float* packed, int Cout, int Cin, int kernel, void* stream) {
  const int kalloc = cx::kstep_alloc(Cin, kernel);
  return bf16x3::pack_operand("conv_bf16x3_pack_weights", weight, packed, conv_bf16x3_packed_floats(Cout, Cin, kernel) != 0,
                              [&] { return fail(FN2_ERR_UNSUPPORTED, "conv_bf16x3_pack_weights: needs Cout %% 16 == 0 (got %d)", Cout); },
                              Cout / 16, kalloc, stream, cx::pack_weights, Cout, Cin, kernel, kalloc);
}

int conv_bf16x3_forward(const float* bottom, const float* packed_weight, const float* bias, float* top, int N, int Cin, int Hin, int Win,
                        int bottom_channels, int bottom_c0, int Cout, int top_channels, int top_c0, int kernel, int stride, int pad,
                        int relu, float negative_slope, void* stream) {
  if (N < 0) return fail(FN2_ERR_INVALID_ARG, "conv_bf16x3: bad batch");
  if (N == 0) return FN2_OK;
  if (const int rc = mfma::check_conv_args("conv_bf16x3", bottom, packed_weight, top, Cin, bottom_channels, bottom_c0, Cout, top_channels, top_c0, [&] {
        return cx::geometry_ok(Cin, Hin, Win, Cout, kernel, stride, pad) ? FN2_OK
            : fail(FN2_ERR_UNSUPPORTED, "conv_bf16x3: unsupported geometry (Cin %d, %dx%d, Cout %d, k %d s %d p %d)", Cin, Hin, Win, Cout, kernel, stride, pad);
      }))
    return rc;
  cx::Args a{};
  a.in = bottom; a.wp = reinterpret_cast<const cx::u32x4*>(packed_weight); a.bias = bias; a.out = top;
  a.N = N; a.Cin = Cin; a.Hin = Hin; a.Win = Win; a.in_ctot = bottom_channels; a.in_c0 = bottom_c0;
  a.Cout = Cout; a.Hout = (Hin + 2 * pad - kernel) / stride + 1; a.Wout = (Win + 2 * pad - kernel) / stride + 1;
  a.out_ctot = top_channels; a.out_c0 = top_c0; a.pad = pad;
  a.kalloc = cx::kstep_alloc(Cin, kernel);
  a.slope = negative_slope; a.relu = relu;
  hipStream_t st = as_stream(stream);
  static TuneCache cache("conv_bf16x3", cx::kNumVariants);
  const TuneKey key{N, Cin, Hin, Win, Cout, kernel, stride, pad, bottom_channels == Cin, top_channels == Cout};
  return bf16x3::pick_and_run("conv_bf16x3", cx::g_forced_variant, cx::kNumVariants, cache, key, st,
                              [&](int i) { return cx::variant_applies(cx::kVariants[i], a, kernel, stride); },
                              [&](int i) { return cx::variant_cost(cx::kVariants[i], a); }, [&](int i) { return cx::kVariants[i].fn(a, st); });
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_conv_bf16x3_supported(const fn2_conv_desc* d) {
  if (!d || d->N < 1 || d->Cin < 1 || d->Cout < 1 || d->Hin < 1 || d->Win < 1) return 0;
  return cx::geometry_ok(d->Cin, d->Hin, d->Win, d->Cout, d->kernel, d->stride, d->pad) ? 1 : 0;
}
