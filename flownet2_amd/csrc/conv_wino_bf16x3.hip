// 3x3 / stride 1 / pad 1 convolution + bias + ReLU as Winograd F(2x2, 3x3) in SPLIT-bf16 ("bf16x3") arithmetic on v_mfma_f32_32x32x16_bf16:
// an opt-in second arithmetic for the layers of csrc/conv_wino.hip, same blob conventions: NCHW in and out, channel slices on both blobs,
// zero padding by out-of-range buffer loads, one launch per mini-batch, no workspace, no pre-split copy of the activations in global memory.
//     Y = A^T [ sum_c (G g_c G^T) (.) (B^T d_c B) ] A          per 2x2 output tile, d = the 4x4 input patch under it
// The 16 element-wise products are 16 independent [tiles x channels] x [channels x Cout] GEMMs, one fp32 accumulator tile per Winograd
// position: rows = 32 output TILES, columns = 32 output channels, a k-step = 16 input channels.
//
// Arithmetic.  U = G g G^T and V = B^T d B are computed in fp32, operation for operation as conv_wino.hip computes them (wino_u,
// wino_transform).  Every U and V value v is then cut into three bf16 pieces  h = rne(v), m = rne(v - h), l = rne(v - h - m)
// (split_bf16.hpp), and of the nine piece products of V * U the six leading ones are formed -- each exact in fp32 -- and summed in fp32:
//     V * U ~ mm + lh + hl + mh + hm + hh          (first letter: the activation's piece; the dropped ml, lm, ll are < 2^-24 |V U|)
// Per Winograd position there is ONE accumulator; k-steps run in ascending channel order without a K split, and inside a k-step the six
// MFMAs go in the order above (small terms first).  The order does not depend on the tile variant, the batch or the run: the result is
// bit-reproducible, a sample has the bits it has alone, and every variant writes the same bits.  It is NOT bit-identical to the exact
// kernel (another summation order inside a k-step, 3 products dropped); it meets that kernel's fp64 bound (tests/test_wino_bf16x3.py).
// Non-finite inputs: Inf splits into (inf, nan, nan), NaN into (nan, nan, nan), so an output whose 3x3 window covers an Inf or a NaN is
// non-finite -- possibly NaN where the exact kernel gives Inf.  Outputs whose window covers no such pixel are unaffected: there are no
// padding slots -- a row of an MFMA is one tile, a k value one channel of that tile's own patch -- and in F(2x2, 3x3) the V entries an
// output reads (A^T . A) are sums of the pixels of its own 3x3 window only.  Channels >= Cin of the last k-step carry zero weights and
// meet zero activations (out of range for the buffer descriptor of the Cin-channel slice), never the neighbouring channels of a wider blob.
//
// Data flow of a workgroup (4 waves, 64 tiles = a TGY x TGX block of 2x2-pixel tiles, 64 output channels), per k-step of 16 channels:
//   * the fp32 window (2 TGY + 2 rows, 2 TGX + 2 columns from x0 - 4) arrives by 16-byte LDS-DMA (mfma_tile.hpp) in [channel][row][column]
//     order, strides RS == 8 (mod 32), CS == 8 (mod 16): the patch reads of a wave are 2-way at worst;
//   * thread (tile, channel quad) transforms its 4 patches ONCE for the whole workgroup -- the exact kernel redoes the transform in every
//     lane for every 16-channel group it serves -- splits the 16 x 4 values and writes the bf16 image [piece][position][tile][16 channels]
//     (32 bytes per tile: a wave's ds_write_b64 and ds_read_b128 each cover contiguous bytes);
//   * wave (tile half wt, channel half wc): per position one ds_read_b128 per piece for A, one global_load_dwordx4 per piece for B (fetched
//     four positions ahead, through the k-step boundary: the operand carries a spare k-step), six MFMAs.
//   One fp32 stage and one image: barrier -> transform + split -> barrier -> (DMA of the next k-step into the stage) + MFMAs from the image.
//   * weight operand, split once when packed: [Cout / 32][ceil(Cin / 16) + 1][16 positions][3 pieces][64 lanes][8 bf16]
//     = (Cout / 32) x (ceil(Cin / 16) + 1) x 12288 floats; lane (column = lane & 31, k half = lane >> 5) holds channels 16 ks + 8 (lane >> 5) + j.
//   * epilogue: the accumulator layout (column on the lane, rows 8 a + 4 (lane >> 5) + r in the registers) leaves all 16 positions of 4
//     horizontally adjacent tiles in one lane: A^T . A in registers, bias + ReLU, two 16-byte stores per output row.
//   Tasks: (channel group, sample, tile row, tile column), tile column fastest: an XCD's contiguous range stays inside one or two channel
//   groups, whose operand (conv3_1: 3 MB per 64 channels) then lives in that XCD's L2.
// Build figures (hipcc -O3, gfx950; __launch_bounds__(256, 1): 512 registers per lane): both variants 256 architectural + 256 accumulator
// VGPRs (the 16 positions x 16 accumulator registers ARE the 256), no spills, no scratch; LDS variant 0 (16x16-pixel tile) 145,408 bytes,
// variant 1 (8x32-pixel tile) 124,928 bytes: one workgroup per CU, one wave per SIMD.
// Measured on an MI355X (profiles/wino_bf16x3_bench.md): this kernel is NOT a speed-up.  1.37 / 1.16 times the exact kernel's time at
// FlowNetC's conv3_1 / conv4_1 (batch 8 @448x320), 1.41 / 1.17 / 1.44 at the three largest Winograd layers of FlowNet2 (batch 4 @768x384),
// 1.52 on a 64-channel layer, 1.14 on an 11-channel one: no geometry class is faster, so none is singled out -- the switch is kept, like the
// correlation's, so that the measured answer can be reproduced.  With one wave per SIMD nothing runs beside the transform + split pass
// between the two barriers of a k-step (about as many VALU cycles as the k-step has MFMA cycles), and 320 - 384 workgroups on 256 CUs
// are two rounds where the exact kernel's smaller tiles balance.
#include "conv_internal.hpp"
#include "mfma_tile.hpp"
#include "split_bf16.hpp"

namespace fn2 {
namespace wx {

using namespace mfma;
using namespace bf16x3;      // the toolkit of split_bf16.hpp
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

struct Args {
  const float* in; const u32x4* up; const float* bias; float* out;
  int N, Cin, Hin, Win, in_ctot, in_c0;
  int Cout, Hout, Wout, out_ctot, out_c0;
  int nsteps;         // k-steps of 16 input channels
  int kalloc;         // k-steps of the packed weights per 32-channel group, the spare one included
  int tx, ty;         // workgroup tiles per sample along x / y
  int ng;             // Cout / 64
  unsigned total;     // tiles = workgroups
  float slope; int relu;
};

constexpr int kKC = 16;                  // input channels of a k-step
constexpr int kStepVecs = 16 * bf16x3::kStepVecs;      // 16-byte vectors of the weight operand per k-step and 32-channel group: 16 positions
constexpr int kAhead = 4;                // positions the weight fetch runs ahead

template <int TGY_, int TGX_>
struct Cfg {
  static constexpr int TGY = TGY_, TGX = TGX_, NW = 4, THREADS = 256, PADL = 4;
  static constexpr int TH = 2 * TGY, TW = 2 * TGX;                     // output pixels of a workgroup tile
  static constexpr int WR = TH + 2, WC = TW + 2 + PADL;                // window rows / columns (columns from x0 - PADL)
  static constexpr int RS = up_mod(cdiv(WC, 4) * 4, 8, 32);            // row stride (dwords)
  static constexpr int CS = up_mod(WR * RS, 8, 16);                    // channel stride
  static constexpr int SLOTS_C = CS / 4, SLOTS = kKC * SLOTS_C;        // 16-byte slots per channel / per k-step
  static constexpr int NRUN = cdiv(SLOTS, 64), RPW = cdiv(NRUN, NW);   // 1 KiB LDS-DMA runs per k-step / per wave
  static constexpr int BUF = NRUN * 256;                               // dwords of the fp32 stage
  static constexpr int PPLANE = 64 * 32;                               // bytes of the image per (piece, position): 64 tiles x 16 bf16
  static constexpr int LDS_BYTES = 4 * BUF + 3 * 16 * PPLANE;
  static_assert(TGY * TGX == 64 && TGX % 4 == 0 && LDS_BYTES <= 160 * 1024, "workgroup shape");
};

// V = B^T d B of one patch, rows first: per element the operations of conv_wino.hip's wino_transform, in its order
__device__ __forceinline__ void transform_patch(const float* dp, int RS, float (&v)[16]) {
  float w[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float d0 = dp[j], d1 = dp[RS + j], d2 = dp[2 * RS + j], d3 = dp[3 * RS + j];
    w[0][j] = d0 - d2; w[1][j] = d1 + d2; w[2][j] = d2 - d1; w[3][j] = d1 - d3;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[4 * i + 0] = w[i][0] - w[i][2];
    v[4 * i + 1] = w[i][1] + w[i][2];
    v[4 * i + 2] = w[i][2] - w[i][1];
    v[4 * i + 3] = w[i][1] - w[i][3];
  }
}

template <class K>
__device__ __forceinline__ void wino_body(const Args& a, int g, int bx, int by, int n) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave & 1, wc = wave >> 1;                              // tile half, channel half of this wave
  const int x0 = bx * K::TW, y0 = by * K::TH;
  char* const img = reinterpret_cast<char*>(smem + K::BUF);            // [piece][position][tile][16 bf16]

  // ---- LDS-DMA plan of the fp32 stage (mfma_tile.hpp); k-step c adds 16 planes to every in-image offset
  const size_t plane = (size_t)a.Hin * a.Win;
  const __amdgpu_buffer_rsrc_t rs = nchw_rsrc(a.in, n, a.in_ctot, a.in_c0, a.Cin, plane);
  unsigned voff[K::RPW];
  window_plan<K>(voff, wave, lane, y0 - 1, x0 - K::PADL, a.Hin, a.Win, plane);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)smem;
  const unsigned step_bytes = 4u * kKC * (unsigned)plane;
  const ChunkStage<K> stage{rs, voff, step_bytes, lds_base, wave};

  // ---- transform item of this thread: tile it of the 64, channels 4 cq .. 4 cq + 3 of the k-step
  const int cq = tid & 3, it = tid >> 2;
  const float* const sp = smem + 4 * cq * K::CS + 2 * (it / K::TGX) * K::RS + 2 * (it % K::TGX) + K::PADL - 1;      // patch element (0, 0)
  char* const ip = img + it * 32 + cq * 8;

  // ---- operands of the MFMAs
  const char* const ap = img + (wt * 32 + (lane & 31)) * 32 + (lane >> 5) * 16;
  const u32x4* const bl = a.up + (size_t)(2 * g + wc) * a.kalloc * kStepVecs + lane;      // position p, piece q of k-step ks: bl[ks kStepVecs + (3 p + q) 64]

  f32x16 acc[16];
#pragma unroll
  for (int p = 0; p < 16; ++p)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;

  u32x4 b[kAhead][3];
  stage(0);
#pragma unroll
  for (int p = 0; p < kAhead; ++p)
#pragma unroll
    for (int q = 0; q < 3; ++q) b[p][q] = bl[(3 * p + q) * kPieceVecs];

  for (int c = 0; c < a.nsteps; ++c) {
    wait_vmcnt<0>();                     // this wave's part of the stage has landed
    __syncthreads();                     // ... everyone's; and every wave is done with the image of k-step c - 1
    {
      float v[4][16];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) transform_patch(sp + ch * K::CS, K::RS, v[ch]);
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        float e0 = v[0][p], e1 = v[1][p], e2 = v[2][p], e3 = v[3][p];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          u32x2 w;
          w[0] = piece2(e0, e1);
          w[1] = piece2(e2, e3);
          *reinterpret_cast<u32x2*>(ip + (q * 16 + p) * K::PPLANE) = w;
        }
      }
    }
    __syncthreads();                     // the image is whole, the stage is free
    if (c + 1 < a.nsteps) stage(c + 1);
    const u32x4* const bk = bl + (size_t)c * kStepVecs;
    u32x4 x[2][3];                       // A operands, read one position ahead of the MFMAs that take them
#pragma unroll
    for (int q = 0; q < 3; ++q) x[0][q] = *reinterpret_cast<const u32x4*>(ap + (q * 16) * K::PPLANE);
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      u32x4 w[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (p + 1 < 16) x[(p + 1) & 1][q] = *reinterpret_cast<const u32x4*>(ap + (q * 16 + p + 1) * K::PPLANE);
        w[q] = b[p % kAhead][q];
        b[p % kAhead][q] = bk[(3 * (p + kAhead) + q) * kPieceVecs];      // (runs into the next k-step; the operand carries a spare one)
      }
      // the six products, small terms first: (activation piece, weight piece) = mm, lh, hl, mh, hm, hh
#pragma unroll
      for (int i = 0; i < 6; ++i)
        acc[p] = piece_mfma_32x32x16(i, x[p & 1], w, acc[p]);
      __builtin_amdgcn_sched_barrier(0);        // a position's reads stay with its MFMAs: hoisted together they do not fit the registers
    }
  }

  // ---- epilogue: lane (half = lane >> 5, channel = lane & 31) holds, per position, tiles 8 a4 + 4 half + r of its tile half: one tile
  // row, 4 consecutive tile columns -> Y = A^T M A per tile: 2 output rows x 8 consecutive columns
  // (the lane number is re-derived: nothing of the prologue's per-lane values has to stay in a register across the k loop)
  unsigned lane_e;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
  const int co = 32 * (2 * g + wc) + (int)(lane_e & 31);
  const float bv = a.bias ? a.bias[co] : 0.f;
  float* const oplane = a.out + ((size_t)n * a.out_ctot + a.out_c0 + co) * a.Hout * a.Wout;
#pragma unroll
  for (int a4 = 0; a4 < 4; ++a4) {
    const int t0 = wt * 32 + 8 * a4 + 4 * (int)(lane_e >> 5);
    const int oy = y0 + 2 * (t0 / K::TGX), ox = x0 + 2 * (t0 % K::TGX);
    float y[2][8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float t[2][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        t[0][k] = acc[k][4 * a4 + r] + acc[4 + k][4 * a4 + r] + acc[8 + k][4 * a4 + r];
        t[1][k] = acc[4 + k][4 * a4 + r] - acc[8 + k][4 * a4 + r] - acc[12 + k][4 * a4 + r];
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        y[h][2 * r] = t[h][0] + t[h][1] + t[h][2];
        y[h][2 * r + 1] = t[h][1] - t[h][2] - t[h][3];
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (oy + h >= a.Hout) continue;
      float* orow = oplane + (size_t)(oy + h) * a.Wout;
#pragma unroll
      for (int half = 0; half < 2; ++half)
        store_row4(orow, ox + 4 * half, a.Wout, f32x4{y[h][4 * half], y[h][4 * half + 1], y[h][4 * half + 2], y[h][4 * half + 3]}, bv, a.relu, a.slope);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <class K>
__global__ void __launch_bounds__(256, 1)
conv_wino_bf16x3(Args a) {
  unsigned t;
  if (!xcd_task(blockIdx.x, a.total, t)) return;
  const int bx = t % a.tx; t /= a.tx;
  const int by = t % a.ty; t /= a.ty;
  wino_body<K>(a, (int)(t / a.N), bx, by, (int)(t % a.N));
}

// U = G g G^T, the operations of conv_wino.hip's wino_u in its order
__device__ inline void wino_u(const float g[3][3], float U[4][4]) {
  float tmp[4][3];
  for (int k = 0; k < 3; ++k) {
    tmp[0][k] = g[0][k];
    tmp[1][k] = ((g[0][k] + g[1][k]) + g[2][k]) * 0.5f;
    tmp[2][k] = ((g[0][k] - g[1][k]) + g[2][k]) * 0.5f;
    tmp[3][k] = g[2][k];
  }
  for (int i = 0; i < 4; ++i) {
    U[i][0] = tmp[i][0];
    U[i][1] = ((tmp[i][0] + tmp[i][1]) + tmp[i][2]) * 0.5f;
    U[i][2] = ((tmp[i][0] - tmp[i][1]) + tmp[i][2]) * 0.5f;
    U[i][3] = tmp[i][2];
  }
}

// weight [Cout][Cin][3][3] -> packed [Cout / 32][kalloc][position][piece][lane][8 bf16]; one thread per (group, k-step, lane)
__global__ void __launch_bounds__(256) pack_weights(const float* __restrict__ wsrc, u32x4* __restrict__ up, int Cout, int Cin, int kalloc) {
  int lane, ks, grp;
  if (!pack_thread(Cout / 32, kalloc, lane, ks, grp)) return;
  const int co = 32 * grp + (lane & 31), c0 = kKC * ks + 8 * (lane >> 5);
  float U[8][4][4];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = c0 + j;
    float g[3][3];
    for (int r = 0; r < 3; ++r)
      for (int s = 0; s < 3; ++s) g[r][s] = (ks < kalloc - 1 && ci < Cin) ? wsrc[((size_t)co * Cin + ci) * 9 + r * 3 + s] : 0.f;
    wino_u(g, U[j]);
  }
  u32x4* dst = up + ((size_t)grp * kalloc + ks) * kStepVecs + lane;
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = U[j][p >> 2][p & 3];
    store_pieces(dst + 3 * p * kPieceVecs, kPieceVecs, v);
  }
}

constexpr int kstep_alloc(int Cin) { return cdiv(Cin, kKC) + 1; }      // + 1: the weight fetch runs ahead through the k-step boundary

template <class K>
static int launch(const Args& base, hipStream_t st) {
  Args a = base;
  a.tx = cdiv(a.Wout, K::TW); a.ty = cdiv(a.Hout, K::TH);
  a.ng = a.Cout / 64;
  a.nsteps = cdiv(a.Cin, kKC);
  return launch_tiles<&conv_wino_bf16x3<K>>(a, (long long)a.N * a.tx * a.ty * a.ng, K::THREADS, K::LDS_BYTES, "conv_wino_bf16x3", "conv_wino_bf16x3_forward", st);
}

struct Variant {
  int tgy, tgx;
  int (*fn)(const Args&, hipStream_t);
};

#define FN2_WX_ROW(TGY, TGX) {TGY, TGX, &launch<Cfg<TGY, TGX>>},
// 16x16- and 8x32-pixel tiles of 64 channels
static const Variant kVariants[] = {FN2_WX_ROW(8, 8) FN2_WX_ROW(4, 16)};
FN2_BF16X3_VARIANT_KNOBS(conv_wino_bf16x3)

// Cost model: rounds of workgroups over the 256 CUs (one workgroup per CU; tiles hanging over the image edge included); the square
// tile first among equals (it stages fewer window pixels per tile)
static double variant_cost(const Variant& v, const Args& a) {
  const long long wgs = (long long)a.N * cdiv(a.Wout, 2 * v.tgx) * cdiv(a.Hout, 2 * v.tgy) * (a.Cout / 64);
  return (double)((wgs + 255) / 256) * (v.tgy == v.tgx ? 1.0 : 1.02);
}

bool geometry_ok(int Cin, int Hin, int Win, int Cout, int kernel, int stride, int pad) {
  if (kernel != 3 || stride != 1 || pad != 1 || Cout <= 0 || Cout % 64 != 0) return false;
  return fn2_conv_wino_supported(Cin, Hin, Win, Cout, pad) != 0;       // Win % 4 == 0, the 32-bit offset limits of the exact kernel
}

}  // namespace wx

size_t conv_wino_bf16x3_packed_floats(int Cout, int Cin) {
  if (Cout <= 0 || Cout % 64 != 0 || Cin <= 0) return 0;
  return (size_t)(Cout / 32) * wx::kstep_alloc(Cin) * wx::kStepVecs * 4;
}

int conv_wino_bf16x3_pack_weights(const float* weight, float* packed, int Cout, int Cin, void* stream) {
  const int kalloc = wx::kstep_alloc(Cin);
  return bf16x3::pack_operand("conv_wino_bf16x3_pack_weights", weight, packed, conv_wino_bf16x3_packed_floats(Cout, Cin) != 0,
                              [&] { return fail(FN2_ERR_UNSUPPORTED, "conv_wino_bf16x3_pack_weights: needs Cout %% 64 == 0 (got %d)", Cout); },
                              Cout / 32, kalloc, stream, wx::pack_weights, Cout, Cin, kalloc);
}

int conv_wino_bf16x3_forward(const float* bottom, const float* packed_weight, const float* bias, float* top, int N, int Cin, int Hin, int Win,
                             int bottom_channels, int bottom_c0, int Cout, int top_channels, int top_c0, int kernel, int stride, int pad,
                             int relu, float negative_slope, void* stream) {
  if (N < 0) return fail(FN2_ERR_INVALID_ARG, "conv_wino_bf16x3: bad batch");
  if (N == 0) return FN2_OK;
  if (const int rc = mfma::check_conv_args("conv_wino_bf16x3", bottom, packed_weight, top, Cin, bottom_channels, bottom_c0, Cout, top_channels, top_c0, [&] {
        return wx::geometry_ok(Cin, Hin, Win, Cout, kernel, stride, pad) ? FN2_OK
            : fail(FN2_ERR_UNSUPPORTED, "conv_wino_bf16x3: unsupported geometry (Cin %d, %dx%d, Cout %d, k %d s %d p %d)", Cin, Hin, Win, Cout, kernel, stride, pad);
      }))
    return rc;
  wx::Args a{};
  a.in = bottom; a.up = reinterpret_cast<const wx::u32x4*>(packed_weight); a.bias = bias; a.out = top;
  a.N = N; a.Cin = Cin; a.Hin = Hin; a.Win = Win; a.in_ctot = bottom_channels; a.in_c0 = bottom_c0;
  a.Cout = Cout; a.Hout = Hin; a.Wout = Win; a.out_ctot = top_channels; a.out_c0 = top_c0;
  a.kalloc = wx::kstep_alloc(Cin);
  a.slope = negative_slope; a.relu = relu;
  hipStream_t st = as_stream(stream);
  static TuneCache cache("conv_wino_bf16x3", wx::kNumVariants);
  const TuneKey key{N, Cin, Hin, Win, Cout, kernel, stride, pad, bottom_channels == Cin, top_channels == Cout};
  return bf16x3::pick_and_run("conv_wino_bf16x3", wx::g_forced_variant, wx::kNumVariants, cache, key, st, [](int) { return true; },
                              [&](int i) { return wx::variant_cost(wx::kVariants[i], a); }, [&](int i) { return wx::kVariants[i].fn(a, st); });
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_conv_wino_bf16x3_supported(const fn2_conv_desc* d) {
  if (!d || d->N < 1 || d->Cin < 1 || d->Cout < 1 || d->Hin < 1 || d->Win < 1) return 0;
  return wx::geometry_ok(d->Cin, d->Hin, d->Win, d->Cout, d->kernel, d->stride, d->pad) ? 1 : 0;
}
