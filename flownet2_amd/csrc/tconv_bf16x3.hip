// Data gradient of a stride-2 Convolution (the transposed convolution of csrc/tconv_mfma.hip, kernel 5 / pad 2) in SPLIT-bf16 ("bf16x3")
// arithmetic on v_mfma_f32_16x16x32_bf16: an opt-in second arithmetic for the layers of FN2_BWD_ROUTE_TCONV (conv2 / conv3 of the encoders),
//
//     bottom_diff[n][cb][Y][X] = dact(mask) * sum_{ct, ky, kx : Y = 2 y - pad + ky, X = 2 x - pad + kx}  top_diff[n][ct][y][x] * W[ct][cb][ky][kx]
//
// with the blob conventions of fn2::tc::tconv_mfma: NCHW in and out, channel slices on both blobs, the four parity classes of output
// pixels from ONE staged input window, zero padding by out-of-range buffer loads, an output up to one pixel larger than
// 2 (Hin - 1) + k - 2 pad (odd-sized bottoms), one launch per mini-batch, no workspace, no pre-split copy of top_diff in global memory.
// It is the data-gradient form only: no bias, no ReLU of its own; the optional epilogue multiplies by the leaky-ReLU derivative of the
// layer in front (`mask`, the expression of tconv_body: m > 0.f ? 1.f : slope), scalar tail for odd widths included.
//
// Arithmetic (split_bf16.hpp, conv_bf16x3.hip).  Every fp32 value v is cut into three bf16 pieces  h = rne(v), m = rne(v - h),
// l = rne(v - h - m); of the nine piece products of x * w the six leading ones are formed -- each exact in fp32 -- and summed in fp32:
//     x * w ~ mm + lh + hl + mh + hm + hh          (first letter: the piece of top_diff; the dropped ml, lm, ll are < 2^-24 |x w|)
//
// K-step layout: 16 top_diff channels x 2 taps.  An output pixel of parity class (py, px) = (Y & 1, X & 1) receives the taps
// ky == py + pad, kx == px + pad (mod 2): 9 / 6 / 6 / 4 of the 25 taps.  The taps of a class, in ascending (ky, kx) order, are paired:
// 5 / 3 / 3 / 2 = 13 k-steps per chunk of 16 channels, 26 slots for 25 taps (the 8 channels x 4 taps of the forward kernel would fill 32).
// Lane (pixel p = lane & 15, kq = lane >> 4) holds, for j = 0 .. 7, channel 16 chunk + 8 (kq & 1) + j at the tap 2 t + (kq >> 1) of its
// class.  The one slot past the 9 taps of class (0, 0) carries zero weights and re-reads the pixel of that class's last tap: a pixel of
// the output's OWN window; channels past the last one of a ragged chunk arrive as zeros (out-of-range loads) against zero weights.
//
// Summation order per output element -- FIXED: chunks of 16 channels ascending; within a chunk the k-steps of the element's class
// ascending (pairs of taps in (ky, kx) order); within a k-step the six MFMAs mm, lh, hl, mh, hm, hh on ONE fp32 accumulator.  It does not
// depend on the tile variant, the batch or the run: the same bits across runs, a sample has the bits it has alone, every variant writes
// the same bits.  It is NOT bit-identical to the exact kernel; it meets that route's fp64 bound (1e-5 x scale, tests/test_dgrad_bf16x3.py).
// Non-finite inputs: Inf splits into (inf, nan, nan), NaN into (nan, nan, nan): exactly the outputs whose taps cover such a pixel are
// non-finite (possibly NaN where the exact kernel gives Inf); all others keep their bits.
//
//   * pixel operand: the fp32 window of a workgroup tile for 16 channels arrives by LDS-DMA (mfma_tile.hpp), then the workgroup splits it
//     ONCE into a bf16 image [piece][channel octet][row][column] (16 bytes per pixel, octet and piece): a lane's operand of a k-step is
//     one ds_read_b128 per piece.  barrier -> split -> barrier -> (DMA of the next chunk into the stage) + MFMAs from the image.
//   * weight operand: split once when packed (fn2::tconv_bf16x3_pack_weights) from the Convolution's own blob [Ct][Cb][k][k]:
//     the packed layout of split_bf16.hpp with groups of 16 bottom channels, fetched a k-step ahead.
//   * wave tile MW channel groups x NP patches of 4x4 class positions x 4 classes; epilogue as tconv_body: 8 consecutive output pixels
//     (x parities interleaved) per lane, patch and row parity, two 16-byte stores.
// Build figures (hipcc -O3, gfx950; __launch_bounds__(256, 2) allows 256 registers): variant 0 (tile of 32x4 class positions = 64x8 output
// pixels) 242 VGPRs, 51,456 bytes of LDS; variant 1 (16x8 = 32x16 output pixels) 242 VGPRs, 58,112 bytes; no spills, no scratch, two
// workgroups per CU (by registers: two waves per SIMD; LDS would allow three / two).
#include "conv_internal.hpp"
#include "mfma_tile.hpp"
#include "split_bf16.hpp"

#include <utility>

namespace fn2 {
namespace tx {

using namespace mfma;
using namespace bf16x3;

struct Args {
  const float* in; const u32x4* wp; float* out;
  int N, Cin, Hin, Win, in_ctot, in_c0;
  int Cout, Hout, Wout, out_ctot, out_c0;
  int nchunks;        // chunks of 16 top_diff channels
  int kalloc;         // k-steps of the packed weights per 16-channel group, the spare one included
  int tx, ty, ng;
  unsigned total;
  const float* mask; int mask_ctot, mask_c0; float mask_slope;
};

// parity class algebra of one axis (as csrc/tconv_mfma.hip): taps k == p + PAD (mod 2); tap k reads input position  class position + d_of(k)
template <int KS, int PAD> struct Par {
  static constexpr int par_of(int k) { return (k + PAD) & 1; }
  static constexpr int d_of(int k) { return ((par_of(k) + PAD) >> 1) - (k - ((par_of(k) + PAD) & 1)) / 2; }
  static constexpr int dmin() { int m = 99; for (int k = 0; k < KS; ++k) m = d_of(k) < m ? d_of(k) : m; return m; }
  static constexpr int dmax() { int m = -99; for (int k = 0; k < KS; ++k) m = d_of(k) > m ? d_of(k) : m; return m; }
  static constexpr int ntaps1(int p) { int n = 0; for (int k = 0; k < KS; ++k) n += par_of(k) == p; return n; }      // taps of one axis in class p
  static constexpr int tap1(int p, int i) { for (int k = 0; k < KS; ++k) if (par_of(k) == p && i-- == 0) return k; return -1; }
  // the k-step table of a chunk: classes 0 .. 3 (cls = 2 py + px) in turn, each with cdiv(taps, 2) k-steps
  static constexpr int ntaps(int cls) { return ntaps1(cls >> 1) * ntaps1(cls & 1); }
  static constexpr int ksteps(int cls) { return (ntaps(cls) + 1) / 2; }
  static constexpr int kst() { return ksteps(0) + ksteps(1) + ksteps(2) + ksteps(3); }
  static constexpr int cls_of(int r) { int c = 0; while (r >= ksteps(c)) r -= ksteps(c++); return c; }
  static constexpr int t_of(int r) { int c = 0; while (r >= ksteps(c)) r -= ksteps(c++); return r; }
  // slot s = 2 t + (kq >> 1) of class cls -> tap (ky, kx); false: the padding slot (zero weight)
  static constexpr bool real(int cls, int s) { return s < ntaps(cls); }
  static constexpr int ky_of(int cls, int s) { const int n = ntaps(cls); const int i = s < n ? s : n - 1; return tap1(cls >> 1, i / ntaps1(cls & 1)); }
  static constexpr int kx_of(int cls, int s) { const int n = ntaps(cls); const int i = s < n ? s : n - 1; return tap1(cls & 1, i % ntaps1(cls & 1)); }
};

template <int KS_, int PAD_, int MW_, int NP_, int WM_, int WNX_, int WNY_>
struct Cfg : Window<4 * WNY_ + Par<KS_, PAD_>::dmax() - Par<KS_, PAD_>::dmin(), 4 * NP_ * WNX_ + 4 + Par<KS_, PAD_>::dmax(), 4, WM_ * WNX_ * WNY_> {      // 4 channel quads
  static constexpr int KS = KS_, PAD = PAD_, MW = MW_, NP = NP_, WM = WM_, WNX = WNX_, WNY = WNY_;
  using P = Par<KS, PAD>;
  static constexpr int NW = WM * WNX * WNY, THREADS = 64 * NW;
  static constexpr int DMIN = P::dmin(), DMAX = P::dmax(), ND = DMAX - DMIN + 1;
  static constexpr int PADL = 4;                                     // window column 0 <-> input column j0 - PADL (16-byte aligned)
  static constexpr int TW = 4 * NP * WNX, TH = 4 * WNY;              // class positions of a workgroup tile (2 TW x 2 TH output pixels)
  static constexpr int KST = P::kst();                               // k-steps per chunk
  static_assert(Cfg::WR == TH + ND - 1 && Cfg::WC == TW + PADL + DMAX, "window of the tile");
  static_assert(-DMIN <= PADL, "left margin");
  // bf16 image: 16 bytes per pixel, octet and piece; rows of WCP == 4 (mod 16) pixels: the 4x4 pixels of a patch (stride 1 in both
  // directions) take the 16 distinct 16-byte slots of a 256-byte bank row
  static constexpr int WCP = up_mod(Cfg::WC, 4, 16);
  static constexpr int PIXO = Cfg::WR * WCP, PIX = 2 * PIXO;         // pixels per octet plane / per piece
  static constexpr int LDS_BYTES = 4 * Cfg::BUF + 3 * 16 * PIX;      // fp32 stage + image
  static_assert(LDS_BYTES <= 80 * 1024, "LDS (two workgroups per CU)");
  static_assert(NW == 4, "256 threads");
};

inline int kalloc_for(int Cin, int kst) { return cdiv(Cin, 16) * kst + 1; }      // + 1: the weight fetch runs a k-step ahead

// image pixel of the lane's operand of k-step r of a chunk, patch 0 (+ 4 p: patch p); th: the lane holds the second tap of the pair
template <class K>
__device__ __forceinline__ constexpr int tap_off(int r, int abase, bool th) {
  using P = typename K::P;
  const int cls = P::cls_of(r), t = P::t_of(r);
  const int o0 = P::d_of(P::ky_of(cls, 2 * t)) * K::WCP + P::d_of(P::kx_of(cls, 2 * t));
  const int o1 = P::d_of(P::ky_of(cls, 2 * t + 1)) * K::WCP + P::d_of(P::kx_of(cls, 2 * t + 1));
  return abase + (th ? o1 : o0);
}

// k-step R of a chunk (a compile-time index: the accumulators of its class are registers): the weight operand moves up and the next one
// is fetched; the operand reads run one patch ahead of the 6 MW MFMAs of a patch (pinned, as in tconv_body: all reads of a k-step in
// front of its MFMAs would hold 3 NP operands of 4 registers beside the 4 MW NP accumulators)
template <class K, int R>
__device__ __forceinline__ void kstep(f32x4 (&acc)[4][K::MW][K::NP], u32x4 (&x)[2][3], u32x4 (&w)[K::MW][3], u32x4 (&wn)[K::MW][3], const u32x4* img,
                                      const u32x4* wl, size_t kalloc, int ks0, int abase, bool th) {
  constexpr int MW = K::MW, NP = K::NP, cls = K::P::cls_of(R);
#pragma unroll
  for (int j = 0; j < MW; ++j) {
#pragma unroll
    for (int q = 0; q < 3; ++q) w[j][q] = wn[j][q];
    load_pieces(wl, (size_t)j * kalloc + ks0 + R + 1, wn[j]);                  // (the packed array carries a spare k-step per group)
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int s = R * NP + p;
    if (s + 1 < K::KST * NP) {
      const int off = tap_off<K>((s + 1) / NP, abase, th) + 4 * ((s + 1) % NP);
#pragma unroll
      for (int q = 0; q < 3; ++q) x[(s + 1) & 1][q] = img[q * K::PIX + off];
    }
    __builtin_amdgcn_sched_barrier(0);       // the reads first: they land while this patch's MFMAs run
    // the six products, small terms first: (top_diff piece, weight piece) = mm, lh, hl, mh, hm, hh
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < MW; ++j)
        acc[cls][j][p] = piece_mfma_16x16x32(i, x[s & 1], w[j], acc[cls][j][p]);
    // the patch's accumulators pass through an empty asm: without it the instruction selector defers the MFMAs of the second channel
    // group of every patch to the end of the chunk and spills the operands they wait for (652 registers in the gfx950 build)
#pragma unroll
    for (int j = 0; j < MW; ++j) asm volatile("" : "+v"(acc[cls][j][p]));
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <class K, int... Rs>
__device__ __forceinline__ void ksteps_of_chunk(std::integer_sequence<int, Rs...>, f32x4 (&acc)[4][K::MW][K::NP], u32x4 (&x)[2][3], u32x4 (&w)[K::MW][3],
                                                u32x4 (&wn)[K::MW][3], const u32x4* img, const u32x4* wl, size_t kalloc, int ks0, int abase, bool th) {
  (kstep<K, Rs>(acc, x, w, wn, img, wl, kalloc, ks0, abase, th), ...);
}

template <class K>
__device__ __forceinline__ void tconv_body(const Args& a, int g, int bx, int by, int n) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int MW = K::MW, NP = K::NP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % K::WM, wnx = (wave / K::WM) % K::WNX, wny = wave / (K::WM * K::WNX);
  const int j0 = bx * K::TW, i0 = by * K::TH;                       // class position of the tile
  u32x4* const img = reinterpret_cast<u32x4*>(smem + K::BUF);       // [piece][octet][row][column]

  // ---- LDS-DMA plan of the fp32 stage; chunk c adds 16 planes to every in-image offset
  const size_t plane = (size_t)a.Hin * a.Win;
  const __amdgpu_buffer_rsrc_t rs = nchw_rsrc(a.in, n, a.in_ctot, a.in_c0, a.Cin, plane);
  unsigned voff[K::RPW];
  window_plan<K>(voff, wave, lane, i0 + K::DMIN, j0 - K::PADL, a.Hin, a.Win, plane);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)smem;
  const unsigned chunk_bytes = 4u * 16u * (unsigned)plane;
  const ChunkStage<K> stage{rs, voff, chunk_bytes, lds_base, wave};

  // ---- operands: lane (pixel p16 -> (pi, pj) of the 4x4 patch, kq): channel octet kq & 1, tap 2 t + (kq >> 1) of the k-step's class
  const int kq = lane >> 4, p16 = lane & 15, pi = p16 >> 2, pj = p16 & 3;
  const int abase = (kq & 1) * K::PIXO + (4 * wny + pi - K::DMIN) * K::WCP + (4 * NP * wnx + pj) + K::PADL;      // + d_of(ky) * WCP + d_of(kx)
  const bool th = (kq >> 1) != 0;
  const int cg0 = (g * K::WM + wm) * MW;                            // first 16-channel group of this wave
  const u32x4* wl = packed_lane(a.wp, cg0, a.kalloc, lane);         // group cg0 + j, k-step ks: load_pieces(wl, j kalloc + ks, ..)

  f32x4 acc[4][MW][NP];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < MW; ++j)
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[c][j][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 w[MW][3], wn[MW][3];
  stage(0);
#pragma unroll
  for (int j = 0; j < MW; ++j) load_pieces(wl, (size_t)j * a.kalloc, wn[j]);

  for (int c = 0; c < a.nchunks; ++c) {
    wait_vmcnt<0>();                     // this wave's part of the stage has landed
    __syncthreads();                     // ... everyone's; and every wave is done with the image of chunk c - 1
    // ---- split the stage into the bf16 image: one (pixel, channel octet) per thread and pass
#pragma unroll
    for (int it = 0; it < cdiv(2 * K::WR * K::WC, 256); ++it) {
      const int i = it * 256 + tid;
      if (i < 2 * K::WR * K::WC) {
        const int o = i / (K::WR * K::WC), pix = i % (K::WR * K::WC);
        const int row = pix / K::WC, col = pix % K::WC, idx = o * K::PIXO + row * K::WCP + col;
        const float* s = smem + 8 * o * K::CS + row * K::RS + col;
        float v[8];
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) v[ch] = s[ch * K::CS];
        store_pieces(img + idx, K::PIX, v);
      }
    }
    __syncthreads();                     // the image is whole, the stage is free
    if (c + 1 < a.nchunks) stage(c + 1);
    u32x4 x[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) x[0][q] = img[q * K::PIX + tap_off<K>(0, abase, th)];
    __builtin_amdgcn_sched_barrier(0);
    ksteps_of_chunk<K>(std::make_integer_sequence<int, K::KST>{}, acc, x, w, wn, img, wl, (size_t)a.kalloc, c * K::KST, abase, th);
  }

  // ---- epilogue (tconv_body's): lane (patch row = lane >> 4, channel = lane & 15) holds 4 consecutive class columns of class row i:
  // for both row parities the 8 output pixels X = 2 jc .. 2 jc + 7 (x parities interleaved)
  const int i = i0 + 4 * wny + (lane >> 4);
#pragma unroll
  for (int py = 0; py < 2; ++py) {
    const int Y = 2 * i + py;
    if (Y < a.Hout) {
#pragma unroll
      for (int j = 0; j < MW; ++j) {
        const int co = 16 * (cg0 + j) + (lane & 15);
        float* orow = a.out + (((size_t)n * a.out_ctot + a.out_c0 + co) * a.Hout + Y) * a.Wout;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const int X0 = 2 * (j0 + 4 * (NP * wnx + p));
          const f32x4 e = acc[2 * py][j][p], o = acc[2 * py + 1][j][p];
          f32x4 v[2] = {f32x4{e[0], o[0], e[1], o[1]}, f32x4{e[2], o[2], e[3], o[3]}};
          if (a.mask) {
            const float* mrow = a.mask + (((size_t)n * a.mask_ctot + a.mask_c0 + co) * a.Hout + Y) * a.Wout;
            float m[8];
            if (X0 + 7 < a.Wout) {
              const f32x4 m0 = *reinterpret_cast<const f32x4*>(mrow + X0), m1 = *reinterpret_cast<const f32x4*>(mrow + X0 + 4);
#pragma unroll
              for (int r = 0; r < 4; ++r) { m[r] = m0[r]; m[4 + r] = m1[r]; }
            } else {
#pragma unroll
              for (int r = 0; r < 8; ++r) m[r] = X0 + r < a.Wout ? mrow[X0 + r] : 1.f;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r >> 2][r & 3] *= m[r] > 0.f ? 1.f : a.mask_slope;      // the expression of bias_leaky_relu_bwd: the same bits
          }
          store4(orow, X0, a.Wout, v[0]);
          store4(orow, X0 + 4, a.Wout, v[1]);
        }
      }
    }
  }
}

// Task list: (sample, tile row, tile column, channel group), channel group fastest (xcd_task: neighbours share an input window)
template <class K>
__global__ void __launch_bounds__(256, 2)
tconv_bf16x3(Args a) {
  unsigned t;
  if (!xcd_task(blockIdx.x, a.total, t)) return;
  const int g = t % a.ng; t /= a.ng;
  const int bx = t % a.tx; t /= a.tx;
  tconv_body<K>(a, g, bx, (int)(t % a.ty), (int)(t / a.ty));
}

// weight [Ct][Cb][KS][KS] (the Convolution's own blob) -> the packed layout of split_bf16.hpp, groups of 16 bottom channels
template <int KS, int PAD>
__global__ void __launch_bounds__(256) pack_weights(const float* __restrict__ wsrc, u32x4* __restrict__ wp, int Cb, int Ct, int kalloc) {
  using P = Par<KS, PAD>;
  // (pack_thread's decomposition, written out: through the helper this kernel's code comes out in another order)
  const long long total = (long long)(Cb / 16) * kalloc * 64;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63), ks = (int)((i >> 6) % kalloc), grp = (int)((i >> 6) / kalloc);
  const int chunk = ks / P::kst(), r = ks % P::kst(), kq = lane >> 4, cb = 16 * grp + (lane & 15);
  const int cls = P::cls_of(r), s = 2 * P::t_of(r) + (kq >> 1);
  const bool real = ks < kalloc - 1 && P::real(cls, s);
  const int tap = P::ky_of(cls, s) * KS + P::kx_of(cls, s);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ct = 16 * chunk + 8 * (kq & 1) + j;
    v[j] = (real && ct < Ct) ? wsrc[((size_t)ct * Cb + cb) * KS * KS + tap] : 0.f;
  }
  u32x4 h, m, l;                    // (store_pieces, written out: through the helper this kernel allocates other registers)
  split8(v, h, m, l);
  u32x4* dst = wp + ((size_t)grp * kalloc + ks) * kStepVecs + lane;
  dst[0] = h; dst[kPieceVecs] = m; dst[2 * kPieceVecs] = l;
}

template <class K>
static int launch(const Args& base, hipStream_t st) {
  Args a = base;
  const int Hc = cdiv(a.Hout, 2), Wc = cdiv(a.Wout, 2);
  a.tx = cdiv(Wc, K::TW); a.ty = cdiv(Hc, K::TH);
  a.ng = a.Cout / (16 * K::MW * K::WM);
  a.nchunks = cdiv(a.Cin, 16);
  a.kalloc = kalloc_for(a.Cin, K::KST);
  return launch_tiles<&tconv_bf16x3<K>>(a, (long long)a.N * a.tx * a.ty * a.ng, K::THREADS, K::LDS_BYTES, "tconv_bf16x3", "tconv_bf16x3", st);
}

struct Variant {
  int ks, pad, mw, np, wm, wnx, wny;
  int (*fn)(const Args&, hipStream_t);
};

#define FN2_TX_ROW(KS, PAD, MW, NP, WM, WNX, WNY) {KS, PAD, MW, NP, WM, WNX, WNY, &launch<Cfg<KS, PAD, MW, NP, WM, WNX, WNY>>},
// 5x5 / 2 / 2: tiles of 32x4 and 16x8 class positions (64x8 / 32x16 output pixels) x 64 channels.  (Measured and dropped: the 3x3 / 2 / 1
// class from the same template, 5 k-steps per chunk -- 335.8 us against the exact kernel's 157.7 at conv4's shape, top_diff [8,512,20,28];
// profiles/dgrad_bf16x3_bench.md.)
static const Variant kVariants[] = {FN2_TX_ROW(5, 2, 2, 4, 2, 2, 1) FN2_TX_ROW(5, 2, 2, 4, 2, 1, 2)};
FN2_BF16X3_VARIANT_KNOBS(tconv_bf16x3)

static bool variant_applies(const Variant& v, const Args& a, int KS, int pad) {
  return v.ks == KS && v.pad == pad && a.Cout % (16 * v.mw * v.wm) == 0;
}

// rounds of workgroups over the 512 slots of the chip x accumulator tiles of a wave; the taller tile first among equals
static double variant_cost(const Variant& v, const Args& a) {
  const int Hc = cdiv(a.Hout, 2), Wc = cdiv(a.Wout, 2);
  const long long wgs = (long long)a.N * cdiv(Wc, 4 * v.np * v.wnx) * cdiv(Hc, 4 * v.wny) * (a.Cout / (16 * v.mw * v.wm));
  return (double)((wgs + 511) / 512) * v.mw * v.np * (v.wny > 1 ? 1.0 : 1.05);
}

// top_diff [Cin, Hin, Win] -> bottom_diff [Cout, Hout, Wout]
static bool geometry_ok(int Cin, int Hin, int Win, int Cout, int Hout, int Wout, int kernel, int pad) {
  if (kernel != 5 || pad != 2) return false;                          // the instantiated class; the kernel is a template on (KS, PAD)
  if (!fn2_tconv_supported(Cin, Hin, Win, Cout, Hout, Wout, kernel, pad)) return false;      // Cout % 64, Win % 4, sizes, the output's range
  Args a{};
  a.Cout = Cout;
  for (int i = 0; i < kNumVariants; ++i)
    if (variant_applies(kVariants[i], a, kernel, pad)) return true;
  return false;
}

}  // namespace tx

size_t tconv_bf16x3_packed_floats(int Cb, int Ct, int kernel, int pad) {
  if (Cb <= 0 || Cb % 16 != 0 || Ct <= 0 || kernel != 5 || pad != 2) return 0;
  return bf16x3::packed_floats(Cb / 16, tx::kalloc_for(Ct, tx::Par<5, 2>::kst()));
}

int tconv_bf16x3_pack_weights(const float* weight, float* packed, int Cb, int Ct, int kernel, int pad, void* stream) {
  const int kalloc = tx::kalloc_for(Ct, tx::Par<5, 2>::kst());
  return bf16x3::pack_operand("tconv_bf16x3_pack_weights", weight, packed, tconv_bf16x3_packed_floats(Cb, Ct, kernel, pad) != 0, [&] {
    return fail(FN2_ERR_UNSUPPORTED, "tconv_bf16x3_pack_weights: needs kernel 5, pad 2 and bottom channels %% 16 == 0 (got k %d p %d, %d)", kernel, pad, Cb);
  }, Cb / 16, kalloc, stream, tx::pack_weights<5, 2>, Cb, Ct, kalloc);
}

int tconv_bf16x3_masked(const float* top_diff, const float* packed_weight, float* bottom_diff, int N, int Cin, int Hin, int Win, int top_channels, int top_c0,
                        int Cout, int Hout, int Wout, int bottom_channels, int bottom_c0, int kernel, int pad,
                        const float* mask, int mask_channels, int mask_c0, float mask_slope, void* stream) {
  if (N < 0) return fail(FN2_ERR_INVALID_ARG, "tconv_bf16x3: bad batch");
  if (N == 0) return FN2_OK;
  if (const int rc = mfma::check_conv_args("tconv_bf16x3", top_diff, packed_weight, bottom_diff, Cin, top_channels, top_c0, Cout, bottom_channels, bottom_c0, [&] {
        return tx::geometry_ok(Cin, Hin, Win, Cout, Hout, Wout, kernel, pad) ? FN2_OK
            : fail(FN2_ERR_UNSUPPORTED, "tconv_bf16x3: unsupported geometry (Cin %d, %dx%d, Cout %d, out %dx%d, k %d p %d)", Cin, Hin, Win, Cout, Hout, Wout, kernel, pad);
      }))
    return rc;
  tx::Args a{};
  a.in = top_diff; a.wp = reinterpret_cast<const tx::u32x4*>(packed_weight); a.out = bottom_diff;
  a.N = N; a.Cin = Cin; a.Hin = Hin; a.Win = Win; a.in_ctot = top_channels; a.in_c0 = top_c0;
  a.Cout = Cout; a.Hout = Hout; a.Wout = Wout; a.out_ctot = bottom_channels; a.out_c0 = bottom_c0;
  if (mask) {
    if (mask_c0 < 0 || mask_c0 + Cout > mask_channels) return fail(FN2_ERR_INVALID_ARG, "tconv_bf16x3: mask slice outside its blob");
    if ((reinterpret_cast<uintptr_t>(mask) & 15) != 0) return fail(FN2_ERR_UNSUPPORTED, "tconv_bf16x3: mask blob must be 16-byte aligned");
  }
  a.mask = mask; a.mask_ctot = mask_channels; a.mask_c0 = mask_c0; a.mask_slope = mask_slope;
  hipStream_t st = as_stream(stream);
  static TuneCache cache("tconv_bf16x3", tx::kNumVariants);
  const TuneKey key{N, Cin, Hin, Win, Cout, Hout, Wout, kernel * 16 + pad, top_channels == Cin, bottom_channels == Cout};
  return bf16x3::pick_and_run("tconv_bf16x3", tx::g_forced_variant, tx::kNumVariants, cache, key, st,
                              [&](int i) { return tx::variant_applies(tx::kVariants[i], a, kernel, pad); },
                              [&](int i) { return tx::variant_cost(tx::kVariants[i], a); }, [&](int i) { return tx::kVariants[i].fn(a, st); });
}

}  // namespace fn2

using namespace fn2;

// the layers of FN2_BWD_ROUTE_TCONV this kernel takes: Convolution{5, 2, 2} with Cin % 64 == 0 and a top_diff width that is a multiple of 4
FN2_API int fn2_tconv_bf16x3_supported(const fn2_conv_desc* d, int transposed) {
  if (transposed || !d || d->N < 1 || d->Cin < 1 || d->Cout < 1 || d->Hin < 1 || d->Win < 1 || d->kernel != 5 || d->stride != 2 || d->pad != 2) return 0;
  if (d->Hin + 2 * d->pad < d->kernel || d->Win + 2 * d->pad < d->kernel) return 0;
  const int Ht = (d->Hin + 2 * d->pad - d->kernel) / d->stride + 1, Wt = (d->Win + 2 * d->pad - d->kernel) / d->stride + 1;
  return tx::geometry_ok(d->Cout, Ht, Wt, d->Cin, d->Hin, d->Win, d->kernel, d->pad) ? 1 : 0;
}
