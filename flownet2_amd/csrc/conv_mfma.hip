// Direct convolution (Convolution{kernel_size KS, stride S, pad} + bias + ReLU{negative_slope}) of the FlowNet encoders on
// v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation in k order (bit-identical to an fmaf chain).
//
// Reference: ConvolutionLayer::Forward_gpu (src/caffe/layers/conv_layer.cu:8-23: per SAMPLE im2col_gpu + cublasSgemm, then
// forward_gpu_bias -- base_conv_layer.cpp:326-348) followed by the in-place ReLU layer (relu_layer.cu:8-27).  Here: one
// launch per layer for the whole mini-batch, no column matrix, NCHW in and out (no layout transposes), bias and activation in
// the epilogue, optional channel slices on both blobs (a consumer's concat blob can be written in place).
//
// GEMM view.  Output pixels are cut into 4x4 PATCHES (one MFMA M tile: 16 pixels), output channels into groups of 16 (one N
// tile); K = (channel quad cq, ky, kx) k-steps, the 4 k values of a k-step being the 4 channels of the quad -- so that the
// pixel operand of tap (ky, kx) for lane (pixel p, kq) is ONE ds_read_b32 at  lane_base + immediate  from a window of the
// input staged in its natural [channel][row][column] order:
//     address = [kq * CS + (py * S) * RS + px * S]  +  [cq * 4 * CS + ky * RS + kx + 4 * S * patch]
//   * pixel operand: the input window of a workgroup tile, CQ channel quads at a time, arrives by 16-byte LDS-DMA
//     (buffer_load_dwordx4 ... lds) straight from NCHW; rows / columns outside the image and channels beyond Cin are
//     out-of-range for the buffer descriptor and come back 0.0f = the zero padding.  Two window buffers, one barrier per chunk.
//     RS == 4 (mod 16) and CS == 16 (mod 32) make the stride-1 reads conflict-free (stride 2: 2-way, the odd banks idle).
//   * weight operand: pre-packed once per weight blob (fn2_conv_mfma_pack_weights) as [Cout/64][k-step][lane][4]: lane
//     (co, kq) holds W[64 g + 16 j + co][4 cq + kq][ky][kx] for j = 0..3, so a wave's operand for a k-step is ONE coalesced
//     global_load_dwordx{MW} per lane straight into registers, prefetched NBUFA - 1 k-steps ahead; no LDS for weights.
//   * wave tile = MW channel groups x NP patches (MW * NP accumulator tiles), workgroup = WM x WNX x WNY waves.
//   * epilogue: the MFMA result layout hands every lane 4 consecutive x of one output channel: bias + leaky ReLU + 16-byte store.
#include "mfma_tile.hpp"

namespace fn2 {
namespace cv {

using namespace mfma;

struct Args {
  const float* in; const float* wp; const float* bias; float* out;
  int N, Cin, Hin, Win, in_ctot, in_c0;
  int Cout, Hout, Wout, out_ctot, out_c0;
  int pad;
  int nchunks;        // chunks of CQ channel quads
  int kquads;         // live channel quads, cdiv(Cin, 4): the 1x1 tiles execute no k-step beyond them (the packed weights are padded to whole chunks)
  int ksteps;         // k-steps of the packed weights per 64-channel group (= quads * KS * KS), multiple of the chunk length
  int tx, ty;         // workgroup tiles per sample along x / y
  int ng;             // Cout / (16 * MW * WM)
  unsigned total;     // tiles (= workgroups of the plain launch)
  unsigned nbig;      // split-tail launch: tiles that run whole (a multiple of 256); the rest run as two half-channel workgroups
  float slope; int relu;
};

// P16 (1x1 kernels only): the M tile is 16 CONSECUTIVE pixels of one row instead of a 4x4 patch -- the launcher flattens every plane into
// one row of H * W pixels (a 1x1 convolution has no spatial window), so no tile hangs over an image edge: the plain-GEMM form.
template <int KS_, int S_, int MW_, int NP_, int WM_, int WNX_, int WNY_, int CQ_, int P16_ = 0, int PIN_ = 0>
struct Cfg : Window<((P16_ ? 1 : 4) * WNY_ - 1) * S_ + KS_,                  // window rows per channel: (TH - 1) * S + KS
                    ((P16_ ? 16 : 4) * NP_ * WNX_ - 1) * S_ + KS_ + 4,       // window columns incl. the left margin (pad <= PADL): (TW - 1) * S + KS + PADL
                    CQ_, WM_ * WNX_ * WNY_> {
  static constexpr int KS = KS_, S = S_, MW = MW_, NP = NP_, WM = WM_, WNX = WNX_, WNY = WNY_, CQ = CQ_, P16 = P16_;
  static constexpr int PIN = PIN_;      // 1: operand reads pinned one behind each patch's MFMAs, a k-step ahead (else the compiler's order)
  static constexpr int NW = WM * WNX * WNY, THREADS = 64 * NW;
  static constexpr int PADL = 4;                                     // window columns left of S * x0 (16-byte aligned start)
  static constexpr int TW = (P16 ? 16 : 4) * NP * WNX, TH = (P16 ? 1 : 4) * WNY;   // output pixels of a workgroup tile
  static_assert(!P16 || (KS == 1 && S == 1), "row tiles are for 1x1 kernels");
  static_assert(Cfg::WR == (TH - 1) * S + KS && Cfg::WC == (TW - 1) * S + KS + PADL, "window of the tile");
  static constexpr int KSC = CQ * KS * KS;                           // k-steps per chunk
  static constexpr int NBUFA = ring_depth(KSC);                      // weight-operand ring
  static_assert(KSC % NBUFA == 0, "ring phase must repeat per chunk");
  static_assert(2 * Cfg::BUF * 4 <= 160 * 1024, "LDS");
};

// ---- 1x1 tiles (a plain GEMM over the channels).  The packed weights pad K to whole chunks of 8 channel quads, but only cdiv(Cin, 4)
// quads are live: the k-steps behind them multiply zeros by zeros (7 of 104 for the 386 channels of deconv2) and are not executed.
//
// gemm_chunk: a whole chunk with another one behind it, whose window DMA was issued at the top of this one.  `ahead` = the k-steps the next
// chunk executes (>= 1): its k-step i is prefetched only when i < ahead.  Where ahead < R, the last k-steps have fewer loads behind their
// operand than R; they then wait as if only the next chunk's k-step 0 had been fetched -- never more than are in flight.
// ks is the counter of an unrolled loop in both functions: the ring phase and every wait immediate fold to constants.
template <class K>
__device__ __forceinline__ void gemm_chunk(f32x4 (&acc)[K::MW][K::NP], typename WVec<K::MW>::T (&wreg)[K::NBUFA], const float* win,
                                           const float* wk, unsigned wlane, int ahead) {
  static_assert(K::KS == 1 && K::S == 1, "1x1 tiles");
  constexpr int MW = K::MW, NP = K::NP, KSC = K::KSC, PW = K::P16 ? 16 : 4;
  constexpr int R = K::NBUFA - 1, DMA = K::NRUN / K::NW;
  using WV = typename WVec<MW>::T;
  auto weight_step = [&](int ks) -> WV {
    const float* wks = wk + (size_t)(ks + R) * 256;
    if (ks + R < KSC) wreg[(ks + R) % K::NBUFA] = weight_fetch<MW>(wks, wlane);
    else wreg[(ks + R) % K::NBUFA] = weight_fetch_unless_last<MW>(ahead, ks + R - KSC, wks, wlane);
    const int behind = ks < R ? R + DMA : R;      // loads younger than this k-step's weight when every prefetch was issued
    const int next = ks + R - KSC + 1;            // of them, the next chunk's
    if (next >= 2) ring_wait_either(ahead, R, behind - (next - 1), behind);
    else ring_wait(behind);
    weight_landed(wreg[ks % K::NBUFA]);
    return wreg[ks % K::NBUFA];
  };
  if constexpr (K::PIN) {      // (the two loop forms of conv_body)
    float b[2][NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) b[0][p] = win[PW * p];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < KSC; ++ks) {
      const WV w = weight_step(ks);
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int j = 0; j < MW; ++j) acc[j][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[ks & 1][p], wget<MW>(w, j), acc[j][p], 0, 0, 0);
        if (ks + 1 < KSC) b[(ks + 1) & 1][p] = win[(ks + 1 < KSC ? ks + 1 : ks) * 4 * K::CS + PW * p];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < KSC; ++ks) {
      const WV w = weight_step(ks);
      float b[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) b[p] = win[ks * 4 * K::CS + PW * p];
#pragma unroll
      for (int j = 0; j < MW; ++j)
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[j][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[p], wget<MW>(w, j), acc[j][p], 0, 0, 0);
    }
  }
}

// gemm_last_chunk: the last chunk, which executes its `live` k-steps (1 .. KSC) and leaves behind k-step live - 1.  ONE unrolled body with
// an exit behind every k-step, not a block per live count: the accumulators and the ring keep their registers (a switch over eight unrolled
// blocks doubled the VGPRs and copied ring registers whose loads were in flight on the way into the blocks).  It issues no window and no
// weight beyond k-step live - 1; min(live, R) of its weights were fetched ahead, so at most that many loads are younger than its window and
// that is what its top may leave in flight.  k-step ks leaves min(R, live - 1 - ks) loads in flight, the last one none: nothing of the ring
// or the window is in flight when the epilogue starts.  The operand reads run a k-step ahead in both loop forms (an exit ends a basic
// block: the compiler cannot lift them over it by itself); the read behind the last live k-step stays inside the window buffer.
template <class K>
__device__ __forceinline__ void gemm_last_chunk(f32x4 (&acc)[K::MW][K::NP], typename WVec<K::MW>::T (&wreg)[K::NBUFA], const float* win,
                                                const float* wk, unsigned wlane, int live) {
  static_assert(K::KS == 1 && K::S == 1, "1x1 tiles");
  constexpr int MW = K::MW, NP = K::NP, KSC = K::KSC, PW = K::P16 ? 16 : 4;
  constexpr int R = K::NBUFA - 1;
  using WV = typename WVec<MW>::T;
  const int last = live - 1;
  wait_vmcnt<R>();
#pragma unroll
  for (int j = R - 1; j >= 1; --j) ring_wait_if_le(live, j, j);
  __builtin_amdgcn_s_barrier();
  float b[2][NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) b[0][p] = win[PW * p];
  if constexpr (K::PIN) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ks = 0; ks < KSC; ++ks) {
    if (ks + R < KSC) wreg[(ks + R) % K::NBUFA] = weight_fetch_unless_last<MW>(live, ks + R, wk + (size_t)(ks + R) * 256, wlane);
    ring_wait(KSC - 1 - ks < R ? KSC - 1 - ks : R);
#pragma unroll
    for (int j = (KSC - 1 - ks < R ? KSC - 1 - ks : R) - 1; j >= 0; --j) ring_wait_if_le(last, ks + j, j);
    weight_landed(wreg[ks % K::NBUFA]);
    const WV w = wreg[ks % K::NBUFA];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
      for (int j = 0; j < MW; ++j) acc[j][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[ks & 1][p], wget<MW>(w, j), acc[j][p], 0, 0, 0);
      if (ks + 1 < KSC) b[(ks + 1) & 1][p] = win[(ks + 1 < KSC ? ks + 1 : ks) * 4 * K::CS + PW * p];
      if constexpr (K::PIN) __builtin_amdgcn_sched_barrier(0);
    }
    if (ks + 1 < KSC && last == ks) return;
  }
}

// One workgroup tile: channel group g (of 16 * MW * WM channels), pixel tile (bx, by) of sample n.
template <class K>
__device__ __forceinline__ void conv_body(const Args& a, int g, int bx, int by, int n) {
  static_assert(K::THREADS == 256, "launch bounds");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int KS = K::KS, S = K::S, MW = K::MW, NP = K::NP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % K::WM, wnx = (wave / K::WM) % K::WNX, wny = wave / (K::WM * K::WNX);
  const int x0 = bx * K::TW, y0 = by * K::TH;

  // ---- LDS-DMA plan: run r = i * NW + wave, slot s = 64 r + lane -> (channel, window row, group of 4 columns)
  const size_t plane = (size_t)a.Hin * a.Win;
  const __amdgpu_buffer_rsrc_t rs = nchw_rsrc(a.in, n, a.in_ctot, a.in_c0, a.Cin, plane);
  unsigned voff[K::RPW];
  window_plan<K>(voff, wave, lane, S * y0 - a.pad, S * x0 - K::PADL, a.Hin, a.Win, plane);
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)smem;
  const unsigned chunk_bytes = 4u * 4u * K::CQ * (unsigned)plane;
  auto stage = [&](int chunk, int buf) { stage_chunk<K>(rs, voff, lds_base + 4u * (unsigned)(buf * K::BUF), wave, (unsigned)chunk * chunk_bytes); };

  // ---- operands
  const int kq = lane >> 4, p16 = lane & 15, py = K::P16 ? 0 : p16 >> 2, px = K::P16 ? p16 : p16 & 3;
  constexpr int PW = K::P16 ? 16 : 4, PH = K::P16 ? 1 : 4;          // pixels of an M tile along x / y
  const int bbase = kq * K::CS + (S * (PH * wny + py)) * K::RS + S * (PW * NP * wnx + px) + K::PADL - a.pad;
  using WV = typename WVec<MW>::T;
  // packed weights: [Cout/64][ksteps][64 lanes][4]; this wave's channel groups: 16 * MW * (g * WM + wm) ...
  const int cg0 = (g * K::WM + wm) * MW;                      // first 16-channel group of this wave
  const float* wb = a.wp + (size_t)(cg0 / 4) * a.ksteps * 256 + (cg0 % 4);      // weight_lane, split for weight_fetch: the wave's base + the lane's bytes
  const unsigned wlane = 16u * (unsigned)lane;

  f32x4 acc[MW][NP];
#pragma unroll
  for (int j = 0; j < MW; ++j)
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[j][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  // The weight ring runs R k-steps ahead and waits by hand (weight_fetch / ring_wait* / weight_landed, mfma_tile.hpp).  Order of the loads in
  // flight at k-step ks of chunk c:  weights of k-steps ks .. R - 1 (issued before the chunk's top, only while ks < R) | the window DMA of
  // chunk c + 1 (issued at the top; every wave issues at least DMA instructions of it) | the weights issued since.  A use may therefore leave
  // R + DMA loads in flight while ks < R, and R from then on: the window has the ring's depth, R k-steps, to land before a wait reaches it
  // -- with one counter and in-order returns, the first weight issued behind it cannot be waited for without it.  The last chunk issues no
  // window and no weight beyond its own k-steps (nothing is in flight when the epilogue starts): its uses leave min(R, KSC - 1 - ks).
  constexpr int R = K::NBUFA - 1, DMA = K::NRUN / K::NW;
  static_assert(R + DMA <= 63, "vmcnt has 6 bits");
  WV wreg[K::NBUFA];
  stage(0, 0);
  if constexpr (KS == 1) {
    // whole chunks, then the last chunk with only its live k-steps (gemm_chunk, gemm_last_chunk above)
    const int nfull = a.nchunks - 1;                     // (nchunks >= 1: Cin >= 1)
    const int live = a.kquads - nfull * K::KSC;          // k-steps of the last chunk, 1 .. KSC
#pragma unroll
    for (int i = 0; i < R; ++i) wreg[i] = weight_fetch_unless_last<MW>(nfull ? K::KSC : live, i, wb + (size_t)i * 256, wlane);
    for (int c = 0; c < nfull; ++c) {
      const int buf = c & 1;
      wait_vmcnt<R>();      // as below: R or more weights were fetched behind the window of chunk c
      __builtin_amdgcn_s_barrier();
      stage(c + 1, buf ^ 1);
      gemm_chunk<K>(acc, wreg, smem + buf * K::BUF + bbase, wb + (size_t)c * K::KSC * 256, wlane, c + 1 < nfull ? K::KSC : live);
    }
    gemm_last_chunk<K>(acc, wreg, smem + (nfull & 1) * K::BUF + bbase, wb + (size_t)nfull * K::KSC * 256, wlane, live);
  } else {
    if (a.nchunks > 0) {
#pragma unroll
      for (int i = 0; i < R; ++i) wreg[i] = weight_fetch<MW>(wb + (size_t)i * 256, wlane);
    }
    // the k-step's weight: fetch the one R k-steps ahead, wait for this one
    auto weight_step = [&](int ks0, int ks, int rest) -> WV {
      const float* wks = wb + (size_t)(ks0 + ks + R) * 256;
      if (ks + R < K::KSC) wreg[(ks + R) % K::NBUFA] = weight_fetch<MW>(wks, wlane);
      else wreg[(ks + R) % K::NBUFA] = weight_fetch_unless_last<MW>(rest, 0, wks, wlane);
      const int left = K::KSC - 1 - ks < R ? K::KSC - 1 - ks : R;
      if (ks < R) ring_wait_either(rest, 1, left, R + DMA);
      else if (left < R) ring_wait_either(rest, 1, left, R);
      else ring_wait(R);
      weight_landed(wreg[ks % K::NBUFA]);
      return wreg[ks % K::NBUFA];
    };

    for (int c = 0; c < a.nchunks; ++c) {
      const int buf = c & 1;
      const int rest = a.nchunks - 1 - c;      // chunks still to come
      // in flight: the window of chunk c (issued at the top of the chunk before) and, younger than it, the weight prefetch of the last R
      // k-steps; loads retire in order, so the window has landed once at most R loads remain -- no need to drain the ring
      wait_vmcnt<R>();
      __builtin_amdgcn_s_barrier();
      if (rest) stage(c + 1, buf ^ 1);
      const float* win = smem + buf * K::BUF + bbase;
      const int ks0 = c * K::KSC;
      if constexpr (K::PIN) {
        // operand reads one k-step ahead, ONE read behind the MW MFMAs of every patch, order pinned (a block of NP reads in front of a
        // k-step's MFMAs leaves the matrix pipe a single queued instruction deep while it issues: csrc/conv_plane.hip, DESIGN 3.4 c).
        // A variant of its own: conv3 [16,128,80,112] gains (434 -> 412 us), conv2 [16,64,160,224] loses (428 -> 490): the autotuner
        // decides per layer, the bits are the same.
        float b[2][NP];
        auto tap_off = [](int ks) { const int cq = ks / (KS * KS), ky = (ks / KS) % KS, kx = ks % KS; return cq * 4 * K::CS + ky * K::RS + kx; };
#pragma unroll
        for (int p = 0; p < NP; ++p) b[0][p] = win[tap_off(0) + PW * S * p];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < K::KSC; ++ks) {
          const WV w = weight_step(ks0, ks, rest);
#pragma unroll
          for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int j = 0; j < MW; ++j) acc[j][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[ks & 1][p], wget<MW>(w, j), acc[j][p], 0, 0, 0);
            if (ks + 1 < K::KSC) b[(ks + 1) & 1][p] = win[tap_off(ks + 1 < K::KSC ? ks + 1 : ks) + PW * S * p];
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else {
#pragma unroll
      for (int ks = 0; ks < K::KSC; ++ks) {
        const WV w = weight_step(ks0, ks, rest);
        const int cq = ks / (KS * KS), ky = (ks / KS) % KS, kx = ks % KS;
        float b[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) b[p] = win[cq * 4 * K::CS + ky * K::RS + kx + PW * S * p];
#pragma unroll
        for (int j = 0; j < MW; ++j)
#pragma unroll
          for (int p = 0; p < NP; ++p) acc[j][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[p], wget<MW>(w, j), acc[j][p], 0, 0, 0);
      }
      }
    }

  }

  wait_vmcnt<0>();      // (nothing is in flight behind a last chunk)
  // ---- epilogue: lane (row block = lane >> 4, channel = lane & 15) holds 4 consecutive x of output row y0 + 4 wny + (lane >> 4)
  // (row tiles: pixels 4 (lane >> 4) .. + 3 of the 16-pixel tile, row y0 + wny)
  const int y = K::P16 ? y0 + wny : y0 + 4 * wny + (lane >> 4);
  if (y < a.Hout) {
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      const int co = 16 * (cg0 + j) + (lane & 15);
      const float bv = a.bias ? a.bias[co] : 0.f;
      float* orow = a.out + (((size_t)n * a.out_ctot + a.out_c0 + co) * a.Hout + y) * a.Wout;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int x = K::P16 ? x0 + 16 * (NP * wnx + p) + 4 * (lane >> 4) : x0 + 4 * (NP * wnx + p);
        store_row4(orow, x, a.Wout, acc[j][p], bv, a.relu, a.slope);
      }
    }
  }
}

// Task list: (sample, tile row, tile column, channel group), channel group fastest (the workgroups that share an input window are
// neighbours: xcd_task)
__device__ __forceinline__ void decode_tile(const Args& a, unsigned t, int& g, int& bx, int& by, int& n) {
  g = t % a.ng; t /= a.ng;
  bx = t % a.tx; t /= a.tx;
  by = t % a.ty;
  n = t / a.ty;
}

template <class K>
__global__ void __launch_bounds__(256, 2)
conv_mfma(Args a) {
  unsigned t;
  if (!xcd_task(blockIdx.x, a.total, t)) return;
  int g, bx, by, n;
  decode_tile(a, t, g, bx, by, n);
  conv_body<K>(a, g, bx, by, n);
}

// The same launch with a split tail.  With W tiles over 256 CUs the last, partial round (W mod 256 tiles) leaves most CUs idle for
// a whole tile time; here the first a.nbig tiles (whole rounds) run as they are and each remaining tile is cut into two
// workgroups of half the channels (MW / 2 channel groups per wave): if they are at most 256 the tail costs half a tile time.
// The arithmetic per output element is the same k-ordered chain: same bits.
template <class K>
__global__ void __launch_bounds__(256, 2)
conv_mfma_tail(Args a) {
  using KH = Cfg<K::KS, K::S, K::MW / 2, K::NP, K::WM, K::WNX, K::WNY, K::CQ, K::P16>;
  int g, bx, by, n;
  if (blockIdx.x < a.nbig) {
    const unsigned t = (blockIdx.x % 8) * (a.nbig / 8) + blockIdx.x / 8;
    decode_tile(a, t, g, bx, by, n);
    conv_body<K>(a, g, bx, by, n);
  } else {
    unsigned u;
    if (!xcd_task(blockIdx.x - a.nbig, 2 * (a.total - a.nbig), u)) return;
    decode_tile(a, a.nbig + u / 2, g, bx, by, n);
    conv_body<KH>(a, 2 * g + (int)(u & 1), bx, by, n);
  }
}

// weight [Cout][Cin][KS][KS] -> packed [Cout/64][ksteps + spare][64][4]
__global__ void pack_weights(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int KS, int ksteps, int kalloc) {
  const long long total = (long long)((Cout + 63) / 64) * kalloc * 256;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    long long r = i >> 8;
    const int ks = (int)(r % kalloc), grp = (int)(r / kalloc);
    const int co = 64 * grp + 16 * j + (lane & 15), kq = lane >> 4;
    const int cq = ks / (KS * KS), tap = ks % (KS * KS);
    const int ci = 4 * cq + kq;
    float v = 0.f;
    if (ks < ksteps && ci < Cin && co < Cout) v = w[((size_t)co * Cin + ci) * KS * KS + tap];
    wp[i] = v;
  }
}

// The same packing from a strided VIEW of a weight blob, through LDS: logical element (co, ci, tap) of a [Cout][Cin][KS][KS] operand is
//   src[co * s_co + ci * s_ci + (flip ? T - 1 - tap : tap)]   for co < src_co and ci < src_ci,   0 beyond (channel padding).
// That covers, without a layout pass in front: the blob as it is (s_co = Cin T, s_ci = T), its channel axes swapped (a Deconvolution's
// blob read as a Convolution's, the transposed convolutions of the data gradients: s_co = T, s_ci = src_co T), the 180-degree rotation of
// a 3x3 data gradient (flip), zero channels up to the kernels' group sizes, and the [Cout 16][Cin] GEMM operand of a Deconvolution
// (T = 1, s_co = 1, s_ci = Cout 16).  A training step repacks every weight after every update (39 M floats, two forms each): the
// gather form above reads 4 bytes per 64-byte line (17-56 us per blob, 0.53 ms per step plus 0.35 ms of torch transposes / cats / fills
// in front of it); here a workgroup reads runs of the source's fastest axis, turns them in LDS and writes whole 1 KiB k-steps.
// (KS and with it every divisor of the index decodes is a template parameter: with run-time divisors the kernel spent its time in
// 32-bit divisions -- 21 us per blob, slower than the gather it replaced.)
template <int KS> struct PackTile {
  static constexpr int T = KS * KS;
  static constexpr int QT = KS == 1 ? 8 : KS == 3 ? 3 : KS == 4 ? 2 : 1;      // channel quads per workgroup tile (<= 8192 floats; 7x7: 12544).  Twice the tile
                                                                                // (runs of 0.9-1.2 KB, 2 workgroups per CU) was 1.7x SLOWER: the kernel lives on workgroups in flight
  static constexpr int CIL = 4 * QT, ROW = CIL * T + 1;                          // + 1 float per output-channel row against bank conflicts
  static constexpr int LDS_FLOATS = 64 * ROW;
};

template <int KS, int ORDER>      // ORDER 0: source runs along (ci, tap) for a fixed co; 1: along (co, tap) for a fixed ci; 2: any strides
__global__ void __launch_bounds__(256) pack_weights_view(const float* __restrict__ w, float* __restrict__ wp, int ksteps, int kalloc,
                                                         int src_co, int src_ci, long long s_co, long long s_ci, int flip) {
  using P = PackTile<KS>;
  constexpr int T = P::T, QT = P::QT, CIL = P::CIL, ROW = P::ROW;
  __shared__ float tile[P::LDS_FLOATS];                   // [64][4 * QT][T]
  const int grp = blockIdx.x, cq0 = blockIdx.y * QT;
  const int co0 = 64 * grp, ci0 = 4 * cq0;
  const int nquads = ksteps / T;                          // channel quads of the packed operand (incl. zero padding quads)
  constexpr int TOTAL = 64 * CIL * T;
  if constexpr (ORDER == 0) {
    const float* src = w + (size_t)co0 * s_co + (size_t)ci0 * T;
#pragma unroll
    for (int i = threadIdx.x; i < TOTAL; i += 256) {      // (all loads of the thread in flight at once: TOTAL / 256 <= 49)
      const int col = i / (CIL * T), e = i - col * (CIL * T), c = e / T;
      tile[col * ROW + e] = (co0 + col < src_co && ci0 + c < src_ci) ? src[(size_t)col * s_co + e] : 0.f;
    }
  } else if constexpr (ORDER == 1) {
    const float* src = w + (size_t)ci0 * s_ci + (size_t)co0 * T;
#pragma unroll
    for (int i = threadIdx.x; i < TOTAL; i += 256) {      // (all loads of the thread in flight at once: TOTAL / 256 <= 49)
      const int c = i / (64 * T), e = i - c * (64 * T), col = e / T, t = e - col * T;
      tile[col * ROW + c * T + t] = (co0 + col < src_co && ci0 + c < src_ci) ? src[(size_t)c * s_ci + e] : 0.f;
    }
  } else {
#pragma unroll
    for (int i = threadIdx.x; i < TOTAL; i += 256) {      // (all loads of the thread in flight at once: TOTAL / 256 <= 49)
      const int col = i / (CIL * T), e = i - col * (CIL * T), c = e / T, t = e - c * T;
      tile[col * ROW + e] = (co0 + col < src_co && ci0 + c < src_ci) ? w[(size_t)(co0 + col) * s_co + (size_t)(ci0 + c) * s_ci + t] : 0.f;
    }
  }
  __syncthreads();
  // k-step ks = cq * T + tap: 256 floats [lane = kq * 16 + co % 16][j = co / 16]
  const int nq = min(QT, nquads - cq0);
  float* dst = wp + ((size_t)grp * kalloc + (size_t)cq0 * T) * 256;
  const int j = threadIdx.x & 3, lane = threadIdx.x >> 2;
  const float* trow = tile + (16 * j + (lane & 15)) * ROW + (lane >> 4) * T;
#pragma unroll
  for (int ks = 0; ks < QT * T; ++ks) {
    const int cq = ks / T, tap = ks - cq * T;
    if (cq < nq) dst[ks * 256 + threadIdx.x] = trow[4 * cq * T + (flip ? T - 1 - tap : tap)];
  }
  if (cq0 + QT >= nquads)                                 // the spare k-steps behind the group
    for (int i = threadIdx.x; i < (kalloc - ksteps) * 256; i += 256) wp[((size_t)grp * kalloc + ksteps) * 256 + i] = 0.f;
}

template <int KS>
static void launch_pack_view(const float* w, float* wp, int Cout, int ksteps, int kalloc, int src_co, int src_ci, long long s_co, long long s_ci, int flip,
                             hipStream_t st) {
  using P = PackTile<KS>;
  const dim3 grid((unsigned)((Cout + 63) / 64), (unsigned)cdiv(ksteps / P::T, P::QT));
  if (s_ci == (long long)P::T) hipLaunchKernelGGL((pack_weights_view<KS, 0>), grid, dim3(256), 0, st, w, wp, ksteps, kalloc, src_co, src_ci, s_co, s_ci, flip);
  else if (s_co == (long long)P::T) hipLaunchKernelGGL((pack_weights_view<KS, 1>), grid, dim3(256), 0, st, w, wp, ksteps, kalloc, src_co, src_ci, s_co, s_ci, flip);
  else hipLaunchKernelGGL((pack_weights_view<KS, 2>), grid, dim3(256), 0, st, w, wp, ksteps, kalloc, src_co, src_ci, s_co, s_ci, flip);
}

constexpr int kSpare = 8;          // spare (zero) k-steps behind every group: the weight prefetch runs NBUFA - 1 k-steps ahead
constexpr int kChunkQuads = 2;     // k-steps are padded to a whole number of chunks of at most this many channel quads (8 for 1x1 kernels)

inline int chunk_quads(int KS) { return KS == 1 ? 8 : kChunkQuads; }
inline int ksteps_for(int Cin, int KS) { return cdiv(cdiv(Cin, 4), chunk_quads(KS)) * chunk_quads(KS) * KS * KS; }

template <class K>
static void set_geometry(Args& a) {
  if constexpr (K::P16) {                 // every plane as ONE row of H * W pixels (contiguous in NCHW; a 1x1 kernel has no spatial window)
    a.Win *= a.Hin; a.Hin = 1; a.Wout *= a.Hout; a.Hout = 1;
  }
  a.tx = cdiv(a.Wout, K::TW); a.ty = cdiv(a.Hout, K::TH);
  a.ng = a.Cout / (16 * K::MW * K::WM);
  a.kquads = cdiv(a.Cin, 4);
  a.nchunks = cdiv(a.kquads, K::CQ);
}

inline long long tiles_of(const Args& a) { return (long long)a.N * a.tx * a.ty * a.ng; }

template <class K>
static int launch(const Args& base, hipStream_t st) {
  Args a = base;
  set_geometry<K>(a);
  a.nbig = (unsigned)tiles_of(a);          // (every tile is a whole one)
  return launch_tiles<&conv_mfma<K>>(a, tiles_of(a), K::THREADS, (int)(sizeof(float) * 2 * K::BUF), "conv_mfma", "conv_mfma_forward", st);
}

// whole rounds of tiles, then the remainder as half-channel workgroups (conv_mfma_tail)
inline unsigned whole_rounds(long long tiles) { return (unsigned)(tiles / 256 * 256); }

template <class K>
static int launch_tail(const Args& base, hipStream_t st) {
  if constexpr (K::MW < 2) {
    return fail(FN2_ERR_UNSUPPORTED, "conv_mfma: variant has no split tail");
  } else {
    Args a = base;
    set_geometry<K>(a);
    if (tiles_of(a) > 0x1fffff00ll) return fail(FN2_ERR_UNSUPPORTED, "conv_mfma: grid too large");
    a.total = (unsigned)tiles_of(a); a.nbig = whole_rounds(a.total);
    const unsigned nsm = 2 * (a.total - a.nbig);
    const unsigned grid = a.nbig + 8 * ((nsm + 7) / 8);
    constexpr size_t lds = sizeof(float) * 2 * K::BUF;
    set_dynamic_lds_once<&conv_mfma_tail<K>>((int)lds);
    hipLaunchKernelGGL((conv_mfma_tail<K>), dim3(grid), dim3(K::THREADS), lds, st, a);
    return check_launch("conv_mfma_forward");
  }
}

struct Variant {
  int ks, s, mw, np, wm, wnx, wny, p16;
  int (*fn)(const Args&, hipStream_t);
  int (*fn_tail)(const Args&, hipStream_t);     // nullptr: no split-tail form
};

// X-macro list of the tile variants: (KS, S, MW, NP, WM, WNX, WNY, CQ, split-tail form instantiated)
#define FN2_CV_LIST(X) \
  /* 1x1 stride 1: a plain GEMM over the channels (conv_redir; the weight^T x bottom product of the Deconvolution layers), 8 quads per chunk */ \
  X(1, 1, 2, 7, 2, 2, 1, 8, 1) X(1, 1, 2, 7, 2, 1, 2, 8, 1) X(1, 1, 4, 7, 1, 2, 2, 8, 0) X(1, 1, 4, 7, 1, 1, 4, 8, 0) X(1, 1, 2, 6, 2, 2, 1, 8, 1) \
  X(1, 1, 2, 4, 2, 2, 1, 8, 1) X(1, 1, 2, 7, 1, 2, 2, 8, 0) X(1, 1, 2, 7, 1, 4, 1, 8, 0) X(1, 1, 2, 4, 1, 2, 2, 8, 0) X(1, 1, 4, 4, 1, 2, 2, 8, 0) \
  /* 3x3 stride 1 */ \
  X(3, 1, 2, 7, 2, 2, 1, 2, 1) X(3, 1, 2, 7, 2, 1, 2, 2, 1) X(3, 1, 4, 7, 1, 2, 2, 2, 0) X(3, 1, 4, 7, 1, 1, 4, 2, 0) \
  X(3, 1, 2, 6, 2, 2, 1, 2, 1) X(3, 1, 4, 6, 1, 2, 2, 2, 0) X(3, 1, 4, 4, 1, 2, 2, 2, 0) X(3, 1, 2, 4, 2, 2, 1, 2, 1) \
  /* 3x3 stride 2 */ \
  X(3, 2, 2, 7, 2, 1, 2, 2, 1) X(3, 2, 4, 7, 1, 1, 4, 2, 0) X(3, 2, 2, 6, 2, 2, 1, 2, 1) X(3, 2, 4, 6, 1, 2, 2, 2, 0) X(3, 2, 2, 4, 2, 2, 1, 2, 1) \
  /* 4x4 stride 2 (the data gradient of the Deconvolution{4, 2, 1} layers: a convolution of top_diff with the weight blob as it is) */ \
  X(4, 2, 2, 7, 2, 2, 1, 2, 1) X(4, 2, 2, 7, 2, 1, 2, 2, 1) X(4, 2, 4, 7, 1, 2, 2, 2, 0) X(4, 2, 2, 6, 2, 2, 1, 2, 1) X(4, 2, 4, 4, 1, 2, 2, 2, 0) X(4, 2, 2, 4, 2, 2, 1, 2, 1) \
  /* 5x5 stride 2 */ \
  X(5, 2, 2, 7, 2, 2, 1, 1, 1) X(5, 2, 2, 7, 2, 1, 2, 1, 1) X(5, 2, 4, 7, 1, 2, 2, 1, 0) X(5, 2, 4, 7, 1, 1, 4, 1, 0) \
  X(5, 2, 2, 6, 2, 2, 1, 1, 1) X(5, 2, 4, 6, 1, 2, 2, 1, 0) X(5, 2, 4, 4, 1, 2, 2, 1, 0) \
  /* 7x7 stride 2 (the 12-channel stems of FlowNet2's stacked nets: whole channel quads) */ \
  X(7, 2, 2, 6, 2, 2, 1, 1, 1) X(7, 2, 2, 7, 2, 2, 1, 1, 1) X(7, 2, 4, 4, 1, 2, 2, 1, 0) X(7, 2, 4, 6, 1, 2, 2, 1, 0) X(7, 2, 2, 4, 2, 2, 1, 1, 1)

template <class K, int TAIL> struct TailFn { static constexpr int (*fn)(const Args&, hipStream_t) = nullptr; };
template <class K> struct TailFn<K, 1> { static constexpr int (*fn)(const Args&, hipStream_t) = &launch_tail<K>; };

#define FN2_CV_ROW(KS, S, MW, NP, WM, WNX, WNY, CQ, TAIL) \
  {KS, S, MW, NP, WM, WNX, WNY, 0, &launch<Cfg<KS, S, MW, NP, WM, WNX, WNY, CQ>>, TailFn<Cfg<KS, S, MW, NP, WM, WNX, WNY, CQ>, TAIL>::fn},
#define FN2_CV_ROW16(MW, NP, WM, WNX, WNY, TAIL) \
  {1, 1, MW, NP, WM, WNX, WNY, 1, &launch<Cfg<1, 1, MW, NP, WM, WNX, WNY, 8, 1>>, TailFn<Cfg<1, 1, MW, NP, WM, WNX, WNY, 8, 1>, TAIL>::fn},
#define FN2_CV_PIN(KS, S, MW, NP, WM, WNX, WNY, CQ, P16, TAIL) \
  {KS, S, MW, NP, WM, WNX, WNY, P16, &launch<Cfg<KS, S, MW, NP, WM, WNX, WNY, CQ, P16, 1>>, TailFn<Cfg<KS, S, MW, NP, WM, WNX, WNY, CQ, P16, 1>, TAIL>::fn},
static const Variant kVariants[] = {FN2_CV_LIST(FN2_CV_ROW)
  /* 1x1 on flattened planes (16-pixel row tiles): TW = 16 NP WNX pixels */
  /* (WNY = 1: a flattened plane has one row) */
  FN2_CV_ROW16(2, 7, 2, 2, 1, 1) FN2_CV_ROW16(2, 7, 4, 1, 1, 1) FN2_CV_ROW16(4, 7, 1, 4, 1, 0) FN2_CV_ROW16(4, 7, 2, 2, 1, 0) FN2_CV_ROW16(2, 5, 2, 2, 1, 1)
  FN2_CV_ROW16(2, 4, 2, 2, 1, 1) FN2_CV_ROW16(2, 7, 1, 4, 1, 0) FN2_CV_ROW16(2, 5, 1, 4, 1, 0) FN2_CV_ROW16(4, 5, 1, 4, 1, 0) FN2_CV_ROW16(2, 4, 1, 4, 1, 0)
  FN2_CV_ROW16(4, 5, 2, 2, 1, 0) FN2_CV_ROW16(4, 4, 2, 2, 1, 0)
  /* planes of 140 (10x14) / 288 (12x24) pixels: 9 x 16 = 144 */
  FN2_CV_ROW16(2, 9, 4, 1, 1, 1) FN2_CV_ROW16(2, 9, 2, 2, 1, 1) FN2_CV_ROW16(2, 3, 2, 2, 1, 1) FN2_CV_ROW16(4, 3, 1, 4, 1, 0)
  /* 256-channel workgroup tiles (36 / 28 accumulator tiles per wave): fewer re-reads of the pixel operand by the big-M deconvolution GEMMs */
  FN2_CV_ROW16(4, 9, 4, 1, 1, 0) FN2_CV_ROW16(4, 9, 2, 2, 1, 0) FN2_CV_ROW16(4, 7, 4, 1, 1, 0)
  /* pinned issue order (Cfg::PIN): the 5x5 / 2 tiles the encoders pick and the GEMM tiles of the deconvolutions */
  FN2_CV_PIN(5, 2, 2, 7, 2, 2, 1, 1, 0, 1) FN2_CV_PIN(5, 2, 2, 7, 2, 1, 2, 1, 0, 1)
  FN2_CV_PIN(1, 1, 4, 9, 4, 1, 1, 8, 1, 0) FN2_CV_PIN(1, 1, 2, 9, 4, 1, 1, 8, 1, 1) FN2_CV_PIN(1, 1, 2, 5, 2, 2, 1, 8, 1, 1) FN2_CV_PIN(1, 1, 4, 7, 4, 1, 1, 8, 1, 0)
  FN2_CV_PIN(1, 1, 2, 7, 2, 2, 1, 8, 1, 1) FN2_CV_PIN(1, 1, 2, 3, 2, 2, 1, 8, 1, 1)
  FN2_CV_PIN(3, 1, 2, 7, 2, 2, 1, 2, 0, 1) FN2_CV_PIN(3, 1, 2, 6, 2, 2, 1, 2, 0, 1) FN2_CV_PIN(3, 2, 2, 7, 2, 1, 2, 2, 0, 1) FN2_CV_PIN(3, 2, 2, 6, 2, 2, 1, 2, 0, 1)
  FN2_CV_PIN(4, 2, 2, 7, 2, 2, 1, 2, 0, 1) FN2_CV_PIN(4, 2, 2, 6, 2, 2, 1, 2, 0, 1) FN2_CV_PIN(5, 2, 2, 6, 2, 2, 1, 1, 0, 1)
  FN2_CV_PIN(7, 2, 2, 6, 2, 2, 1, 1, 0, 1) FN2_CV_PIN(7, 2, 4, 6, 1, 2, 2, 1, 0, 0)
  /* 32-channel GEMMs on planes too small to fill the chip with the tiles above (conv_redir, [8,256,40,56] -> 32: 72 workgroups of 256
     pixels): 64- and 128-pixel tiles, 280 / 144 workgroups there.  (New variants go to the end: the forced-variant numbers stay.) */
  FN2_CV_ROW16(2, 1, 1, 4, 1, 0) FN2_CV_ROW16(2, 2, 1, 4, 1, 0) FN2_CV_PIN(1, 1, 2, 1, 1, 4, 1, 8, 1, 0) FN2_CV_PIN(1, 1, 2, 2, 1, 4, 1, 8, 1, 0)};
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

int g_forced_variant = -1;       // >= 0: plain launch of that variant; >= 1000: its split-tail launch

// Cost model: tile times of the busiest CU x accumulator tiles of a wave (tiles hanging over the image edge included), with a
// mild penalty for small wave tiles (more operand traffic per MFMA).  tail: the last partial round as half tiles.
static double variant_cost(const Variant& v, const Args& a, bool tail) {
  const int tw = (v.p16 ? 16 : 4) * v.np * v.wnx, th = (v.p16 ? 1 : 4) * v.wny;
  const long long wgs = v.p16 ? (long long)a.N * cdiv(a.Wout * a.Hout, tw) * (a.Cout / (16 * v.mw * v.wm))
                              : (long long)a.N * cdiv(a.Wout, tw) * cdiv(a.Hout, th) * (a.Cout / (16 * v.mw * v.wm));
  double rounds = (double)((wgs + 255) / 256);
  if (tail) {
    const long long r = wgs % 256;
    if (wgs < 256 || r == 0 || r > 128) return 1e30;               // nothing to gain
    rounds = (double)(wgs / 256) + 0.5 * 1.12;                      // half tiles run MW / 2: less efficient
  }
  const double eff = 1.0 / (1.0 + 0.08 * (4.0 / v.mw - 1.0) + 0.02 * (7.0 / v.np - 1.0));
  return rounds * v.mw * v.np / eff;
}

static bool variant_applies(const Variant& v, const Args& a, int KS, int S) {
  if (!v.p16 && a.Win % 4 != 0) return false;          // 4x4-patch tiles stage 16-byte pieces of image rows; row tiles only need H * W % 4 == 0
  return v.ks == KS && v.s == S && a.Cout % (16 * v.mw * v.wm) == 0;
}

}  // namespace cv
}  // namespace fn2

using namespace fn2;

FN2_API size_t fn2_conv_mfma_packed_floats(int Cout, int Cin, int kernel) {
  if (Cout <= 0 || Cout % 32 != 0 || Cin <= 0 || kernel <= 0) return 0;
  return (size_t)((Cout + 63) / 64) * (cv::ksteps_for(Cin, kernel) + cv::kSpare) * 256;
}

FN2_API int fn2_conv_mfma_pack_weights_view(const float* weight, float* packed, int Cout, int Cin, int kernel, int src_cout, int src_cin,
                                            long long stride_cout, long long stride_cin, int flip, void* stream);

FN2_API int fn2_conv_mfma_pack_weights(const float* weight, float* packed, int Cout, int Cin, int kernel, void* stream) {
  if (!weight || !packed) return fail(FN2_ERR_INVALID_ARG, "conv_mfma_pack_weights: null blob");
  if (Cout <= 0 || Cout % 32 != 0 || Cin <= 0 || (kernel != 1 && kernel != 3 && kernel != 4 && kernel != 5 && kernel != 7))
    return fail(FN2_ERR_UNSUPPORTED, "conv_mfma_pack_weights: needs Cout %% 32 == 0 and kernel_size 1, 3, 4, 5 or 7 (got Cout %d, kernel %d)", Cout, kernel);
  return fn2_conv_mfma_pack_weights_view(weight, packed, Cout, Cin, kernel, Cout, Cin, (long long)Cin * kernel * kernel, (long long)kernel * kernel, 0, stream);
}

FN2_API int fn2_conv_mfma_pack_weights_view(const float* weight, float* packed, int Cout, int Cin, int kernel, int src_cout, int src_cin,
                                            long long stride_cout, long long stride_cin, int flip, void* stream) {
  if (!weight || !packed) return fail(FN2_ERR_INVALID_ARG, "conv_mfma_pack_weights_view: null blob");
  if (Cout <= 0 || Cout % 32 != 0 || Cin <= 0 || (kernel != 1 && kernel != 3 && kernel != 4 && kernel != 5 && kernel != 7))
    return fail(FN2_ERR_UNSUPPORTED, "conv_mfma_pack_weights_view: needs Cout %% 32 == 0 and kernel_size 1, 3, 4, 5 or 7 (got Cout %d, kernel %d)", Cout, kernel);
  if (src_cout < 1 || src_cout > Cout || src_cin < 1 || src_cin > Cin || stride_cout < 1 || stride_cin < 1)
    return fail(FN2_ERR_INVALID_ARG, "conv_mfma_pack_weights_view: bad source view (%d of %d, %d of %d channels, strides %lld / %lld)", src_cout, Cout,
                src_cin, Cin, stride_cout, stride_cin);
  const int ksteps = cv::ksteps_for(Cin, kernel), kalloc = ksteps + cv::kSpare;
  hipStream_t st = as_stream(stream);
  switch (kernel) {
    case 1: cv::launch_pack_view<1>(weight, packed, Cout, ksteps, kalloc, src_cout, src_cin, stride_cout, stride_cin, flip ? 1 : 0, st); break;
    case 3: cv::launch_pack_view<3>(weight, packed, Cout, ksteps, kalloc, src_cout, src_cin, stride_cout, stride_cin, flip ? 1 : 0, st); break;
    case 4: cv::launch_pack_view<4>(weight, packed, Cout, ksteps, kalloc, src_cout, src_cin, stride_cout, stride_cin, flip ? 1 : 0, st); break;
    case 5: cv::launch_pack_view<5>(weight, packed, Cout, ksteps, kalloc, src_cout, src_cin, stride_cout, stride_cin, flip ? 1 : 0, st); break;
    default: cv::launch_pack_view<7>(weight, packed, Cout, ksteps, kalloc, src_cout, src_cin, stride_cout, stride_cin, flip ? 1 : 0, st); break;
  }
  return check_launch("conv_mfma_pack_weights_view");
}

FN2_API int fn2_conv_mfma_supported(int Cin, int Hin, int Win, int Cout, int kernel, int stride, int pad) {
  if (Cin <= 0 || Hin <= 0 || Win <= 0 || Cout <= 0 || Cout % 32 != 0) return 0;
  if (kernel == 1 ? ((long long)Hin * Win) % 4 != 0 : Win % 4 != 0) return 0;      // (1x1: the planes are flattened, only their size matters)
  if (!((kernel == 1 && stride == 1) || (kernel == 3 && (stride == 1 || stride == 2)) || (kernel == 4 && stride == 2) || (kernel == 5 && stride == 2) || (kernel == 7 && stride == 2))) return 0;
  if (pad < 0 || pad > 4 || pad > kernel - 1) return 0;
  if ((long long)Cin * Hin * Win >= (1ll << 28)) return 0;
  const int Hout = (Hin + 2 * pad - kernel) / stride + 1, Wout = (Win + 2 * pad - kernel) / stride + 1;
  if (Hout < 1 || Wout < 1) return 0;
  // and a tile variant that takes it: only the 1x1 tiles block Cout by 32, the others by 64 (a Convolution{5, 2, 2} with 96 outputs
  // used to be routed DIRECT by fn2_conv_route and then failed at launch with "no kernel variant")
  cv::Args a{};
  a.Win = Win; a.Cout = Cout;
  for (int i = 0; i < cv::kNumVariants; ++i)
    if (cv::variant_applies(cv::kVariants[i], a, kernel, stride)) return 1;
  return 0;
}

FN2_API int fn2_debug_set_conv_variant(int v) { cv::g_forced_variant = v; return FN2_OK; }
FN2_API int fn2_conv_mfma_num_variants(void) { return cv::kNumVariants; }

FN2_API int fn2_conv_mfma_forward(const float* bottom, const float* packed_weight, const float* bias, float* top,
                                  int N, int Cin, int Hin, int Win, int bottom_channels, int bottom_c0,
                                  int Cout, int top_channels, int top_c0, int kernel, int stride, int pad,
                                  int relu, float negative_slope, void* stream) {
  if (N < 0) return fail(FN2_ERR_INVALID_ARG, "conv_mfma: bad batch");
  if (N == 0) return FN2_OK;
  if (const int rc = mfma::check_conv_args("conv_mfma", bottom, packed_weight, top, Cin, bottom_channels, bottom_c0, Cout, top_channels, top_c0, [&] {
        return fn2_conv_mfma_supported(Cin, Hin, Win, Cout, kernel, stride, pad) ? FN2_OK
            : fail(FN2_ERR_UNSUPPORTED, "conv_mfma: unsupported geometry (Cin %d, %dx%d, Cout %d, k %d s %d p %d)", Cin, Hin, Win, Cout, kernel, stride, pad);
      }))
    return rc;
  cv::Args a{};
  a.in = bottom; a.wp = packed_weight; a.bias = bias; a.out = top;
  a.N = N; a.Cin = Cin; a.Hin = Hin; a.Win = Win; a.in_ctot = bottom_channels; a.in_c0 = bottom_c0;
  a.Cout = Cout; a.Hout = (Hin + 2 * pad - kernel) / stride + 1; a.Wout = (Win + 2 * pad - kernel) / stride + 1;
  a.out_ctot = top_channels; a.out_c0 = top_c0; a.pad = pad;
  a.ksteps = cv::ksteps_for(Cin, kernel) + cv::kSpare;
  a.slope = negative_slope; a.relu = relu;
  hipStream_t st = as_stream(stream);
  static TuneCache cache("conv_mfma", cv::kNumVariants);
  const TuneKey key{N, Cin, Hin, Win, Cout, kernel, stride, pad, bottom_channels == Cin, top_channels == Cout};
  mfma::Pick p;
  if (const int rc = mfma::pick_variant(p, "conv_mfma", cv::g_forced_variant, cv::kNumVariants, true, cache, key, st,
                                        [&](int i) { return cv::variant_applies(cv::kVariants[i], a, kernel, stride); },
                                        [&](int i, bool tail) { return cv::variant_cost(cv::kVariants[i], a, tail); },
                                        [&](int i, bool tail) { return tail ? cv::kVariants[i].fn_tail(a, st) : cv::kVariants[i].fn(a, st); },
                                        [&](int i) { return cv::kVariants[i].fn_tail != nullptr; }))
    return rc;
  return p.tail ? cv::kVariants[p.variant].fn_tail(a, st) : cv::kVariants[p.variant].fn(a, st);
}
