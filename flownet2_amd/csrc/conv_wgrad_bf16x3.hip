// Weight gradient of a Convolution{5, 2, 2} (the quantity of csrc/conv_wgrad.hip) in SPLIT-bf16 ("bf16x3") arithmetic on
// v_mfma_f32_16x16x32_bf16: an opt-in second arithmetic for conv2 / conv3 of the encoders,
//
//     dw[ca][cb][ky][kx] (+)= sum_{n, y, x}  a[n][a_c0 + ca][y][x] * b[n][b_c0 + cb][2 y + ky - 2][2 x + kx - 2]        (zero outside b)
//
// a = top_diff, b = bottom, dw = weight_diff [Cout][Cin][5][5].  As conv_wgrad.hip: NCHW blobs and channel slices on both, zero padding by
// out-of-range buffer loads, a deterministic ordered K split into slab parts which fn2::wgrad_finalize_parts (conv_wgrad.hip's two finalize
// kernels, through the same SlabMap) adds in part order, accumulate != 0 adds into dw, workspace from the caller, no pre-split copy in
// global memory.
//
// Arithmetic (split_bf16.hpp).  Every fp32 value v of BOTH operands is cut into three bf16 pieces h = rne(v), m = rne(v - h),
// l = rne(v - h - m); of the nine piece products of a * b the six leading ones are formed -- each exact in fp32 -- and summed in fp32:
//     a * b ~ mm + lh + hl + mh + hm + hh          (first letter: the piece of a = top_diff; the dropped ml, lm, ll are < 2^-24 |a b|)
//
// GEMM view: M = 16 `a` channels, N = 16 `b` channels, K = pixels; one k-step = 4 rows x 8 pixels of the `a` map: lane (channel = lane & 15,
// k-group g = lane >> 4) holds, for j = 0 .. 7, pixel (row g, column 8 xb + j) of the chunk.  A wave owns MA x 1 channel-group pairs x all
// 25 taps (one accumulator tile each); a workgroup (4 waves, 2 x 2) walks the rows of its K part in chunks of (up to) 4 rows x 8 pixels.
// Per chunk: the fp32 `a` pixels [CA][4][8] and the `b` window [32][11 rows][24 columns] (window column wc <-> column 2 x0 - 4 + wc, window
// row wr <-> row 2 y0 - 2 + wr) arrive by 16-byte LDS-DMA, then the workgroup splits them ONCE into bf16 images:
//     barrier -> split -> barrier -> (DMA of the next chunk into the stage) + 150 MA MFMAs from the images.
//   * `a` image [piece][row][channel][8 pixels]: the operand is one aligned ds_read_b128 per piece (channels 16 bytes apart, rows
//     16 CA = 0 (mod 256) bytes apart: conflict-free over the four 16-lane groups of the instruction).
//   * `b` image, parity-deinterleaved: tap kx of pixel j reads window column 2 j + kx + 2, i.e. element j - 1 / j / j + 1 (kx = 0 / 2 / 4)
//     of the even plane P_e[i] = column 2 i + 4, or element j - 1 / j (kx = 1 / 3) of the odd plane P_o[i] = column 2 i + 5.
//     THE ALIGNMENT CHOICE: aligned read plus neighbour dwords, shifted in registers.  Per window row, parity and piece the image keeps the
//     aligned 16 bytes P[0 .. 7] ([piece][row][parity][channel], as the `a` image) and, in a second array, 8 bytes (P[8], P[9] | P[-2], P[-1]).
//     A lane reads ds_read_b128 + ds_read_b64 (even) and ds_read_b128 + ds_read_b32 (odd) per window row and piece -- 12 reads for the 5 taps
//     of a ky -- and builds the operands of kx = 0, 1, 4 with __builtin_amdgcn_alignbit (hipcc emits v_perm_b32): 8 distinct shifts + 2 masks per piece, 30 VALU
//     instructions
//     beside the 30 MA MFMAs of a ky.  (Per-kx aligned copies of the planes would take 2.5 x the LDS of the image.)
//   * K padding.  Rows of a chunk beyond its valid rows (the end of the part or of the sample): `a` is zero (not loaded) and the lanes of
//     those k-groups read the `b` rows of the chunk's LAST VALID row -- a pixel of the element's own window against a zero.  Pixels beyond the
//     row end (Wa % 8 == 4, last x block): `a` is zero; of `b` only element j = 4 of kx = 0 / 1 (columns Wb - 2, Wb - 1) is not already zero
//     padding, and that element is masked to zero in the operand.  So a non-finite `b` value reaches exactly the taps the exact kernel
//     gives it to, and a non-finite `a` value exactly its own `a` channel (Inf splits into (inf, nan, nan): NaN where the exact kernel may
//     give Inf).
//
// Summation order per weight element -- a function of the layer geometry only: K is cut into ksplit parts of whole rows
// (wgx::ksplit_for_split: conv_wgrad_geom.hpp's ksplit_for capped to at least 4 rows per part; rows [p U / ksplit, (p + 1) U / ksplit) of the
// flattened (n, y), U = N Ha); within a part the k-steps ascend over (groups of up to 4 rows that stay inside the sample and the part,
// x blocks of 8 pixels); within a k-step the six MFMAs mm, lh, hl, mh, hm, hh on ONE fp32 accumulator; the parts are added in part order.
// It does not depend on the tile variant or the run: every variant writes the same bits.  NOT the exact kernel's bits; within its fp64
// bound (tests/test_wgrad_bf16x3.py).
//
// Build figures (hipcc -O3 --save-temps, gfx950), no spills, no scratch, one workgroup per CU (by LDS):
//   variant 0 (MA = 2: 64 x 32 channels per workgroup)  168 VGPRs + 200 AGPRs (accumulators), 107,008 bytes of LDS
//   variant 1 (MA = 1: 32 x 32 channels per workgroup)  156 VGPRs + 100 AGPRs, 96,768 bytes of LDS
#include "conv_internal.hpp"
#include "conv_wgrad_geom.hpp"
#include "mfma_tile.hpp"
#include "split_bf16.hpp"

namespace fn2 {
namespace wgx {

using namespace mfma;
using namespace bf16x3;
using wg::SlabMap;
using wg::part_begin;

using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

struct Args {
  const float* a; const float* b; float* slab;
  int N, Ca, Ha, Wa, a_ctot, a_c0;
  int Cb, Hb, Wb, b_ctot, b_c0;
  int ksplit, nblk_a, nblk_b, nxb, U;
  unsigned total;            // workgroups: nblk_a * nblk_b * ksplit
  long long slab_part;       // floats per part
};

struct Chunk { int n, y, rvalid, x0; };

template <int MA_>
struct Cfg {
  static constexpr int MA = MA_, NB = 1, WM = 2, WN = 2, NW = 4, THREADS = 256, T = 25, KS = 5;
  static constexpr int CA = 16 * MA * WM, CB = 16 * NB * WN, TILES = MA * NB * T;
  static constexpr int R = 4, XT = 8;                          // the chunk = one k-step: 4 rows x 8 pixels
  // fp32 stage, `a`: [CA][R][XT], channel stride 36 dwords (36 c mod 64 distinct multiples of 4 for 16 channels: the split's b128 reads)
  static constexpr int CSA = 36, SLOTS_CA = CSA / 4, SLOTS_A = CA * SLOTS_CA, NRUN_A = cdiv(SLOTS_A, 64), A_DW = NRUN_A * 256;
  // fp32 stage, `b`: [CB][WR][RSB], channel stride 268 dwords (== 12 mod 64, the same property)
  static constexpr int WR = 2 * (R - 1) + KS, RSB = 24, CSB = 268, SLOTS_CB = CSB / 4, SLOTS_B = CB * SLOTS_CB, NRUN_B = cdiv(SLOTS_B, 64);
  static constexpr int B_DW = NRUN_B * 256;
  static constexpr int RPW_A = cdiv(NRUN_A, NW), RPW_B = cdiv(NRUN_B, NW);
  static constexpr int STAGE_BYTES = 4 * (A_DW + B_DW);
  // bf16 images (bytes)
  static constexpr int PA = R * CA * 16;                       // `a`, per piece: [row][channel] x 16
  static constexpr int BM = WR * 2 * CB * 16, BX = WR * 2 * CB * 8, PB = BM + BX;      // `b`, per piece: main [wr][parity][channel] x 16, then extra x 8
  static constexpr int IMG_A = STAGE_BYTES, IMG_B = IMG_A + 3 * PA;
  static constexpr int LDS_BYTES = IMG_B + 3 * PB;
  static_assert(WR * RSB <= CSB && R * XT <= CSA, "images inside their channel strides");
  static_assert((CA * 16) % 256 == 0 && (2 * 2 * CB * 16) % 256 == 0, "k-groups a whole bank row apart");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// LDS-DMA of one chunk into the stage at LDS byte address `dst`.  Slot s (16 bytes) of the `a` stage: channel s / 9, dword 4 (s % 9) of
// [4 rows][8 pixels]; of the `b` stage: channel s / 67, dword 4 (s % 67) of [11 rows][24 columns].  pa_rc / pb_rc: the slot's (row, column),
// rows 255 / 0x7fff for slots outside the image or the blob.
template <class K>
__device__ __forceinline__ void stage_chunk(const Args& a, const Chunk& c, int ca0, int cb0, unsigned dst, int wave,
                                            const unsigned (&pa_off)[K::RPW_A], const unsigned (&pa_rc)[K::RPW_A],
                                            const unsigned (&pb_off)[K::RPW_B], const unsigned (&pb_rc)[K::RPW_B]) {
  const size_t planeA = (size_t)a.Ha * a.Wa, planeB = (size_t)a.Hb * a.Wb;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.a + ((size_t)c.n * a.a_ctot + a.a_c0 + ca0) * planeA), 0, (unsigned)(4u * K::CA * planeA), kRsrcWord3);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.b + ((size_t)c.n * a.b_ctot + a.b_c0 + cb0) * planeB), 0, (unsigned)(4u * K::CB * planeB), kRsrcWord3);
  const unsigned originA = (unsigned)(c.y * a.Wa + c.x0);
#pragma unroll
  for (int i = 0; i < K::RPW_A; ++i) {
    const int run = i * K::NW + wave;
    if (run < K::NRUN_A) {
      const unsigned r = pa_rc[i] & 0xffu, x = pa_rc[i] >> 8;
      const bool ok = (int)r < c.rvalid && c.x0 + (int)x < a.Wa;
      const unsigned voff = ok ? 4u * (pa_off[i] + originA) : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(uintptr_t)(dst + 1024u * (unsigned)run), 16, voff, 0, 0, 0);
    }
  }
  const int gy0 = 2 * c.y - 2, gx0 = 2 * c.x0 - 4, wr_end = 2 * (c.rvalid - 1) + K::KS;      // (the rows of the valid `a` rows only)
#pragma unroll
  for (int i = 0; i < K::RPW_B; ++i) {
    const int run = i * K::NW + wave;
    if (run < K::NRUN_B) {
      const int wr = (int)(pb_rc[i] & 0xffffu);
      const int gy = gy0 + wr, gx = gx0 + (int)(pb_rc[i] >> 16);
      const bool ok = wr < wr_end && (unsigned)gy < (unsigned)a.Hb && (unsigned)gx < (unsigned)a.Wb;
      const unsigned voff = ok ? 4u * (pb_off[i] + (unsigned)(gy * a.Wb + gx)) : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(uintptr_t)(dst + 4u * K::A_DW + 1024u * (unsigned)run), 16, voff, 0, 0, 0);
    }
  }
}

// 8 consecutive window columns c0 .. c0 + 7 -> per piece (d0, d1, d2, d3) = (columns c0, c0 + 2 | c0 + 1, c0 + 3 | c0 + 4, c0 + 6 | c0 + 5, c0 + 7):
// the even-plane pairs in dwords 0 and 2, the odd-plane pairs in dwords 1 and 3
__device__ __forceinline__ void split8_planes(const float* s, u32x4& h, u32x4& m, u32x4& l) {
  const f32x4 lo = *reinterpret_cast<const f32x4*>(s), hi = *reinterpret_cast<const f32x4*>(s + 4);
  float v[8] = {lo[0], lo[2], lo[1], lo[3], hi[0], hi[2], hi[1], hi[3]};
  split8(v, h, m, l);
}

// The stage -> the bf16 images.  `a`: one (channel, row) = 8 pixels per thread.  `b`: one (channel, window row) = 24 columns per thread.
template <class K>
__device__ __forceinline__ void split_stage(float* smem, int tid) {
  char* const base = reinterpret_cast<char*>(smem);
  if (tid < K::R * K::CA) {
    const int ch = tid % K::CA, r = tid / K::CA;
    const float* s = smem + ch * K::CSA + r * K::XT;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(s), hi = *reinterpret_cast<const f32x4*>(s + 4);
    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    u32x4 p[3];
    split8(v, p[0], p[1], p[2]);
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x4*>(base + K::IMG_A + q * K::PA + (r * K::CA + ch) * 16) = p[q];
  }
#pragma unroll
  for (int it = 0; it < cdiv(K::WR * K::CB, 256); ++it) {
    const int i = it * 256 + tid;
    if (i < K::WR * K::CB) {
      const int ch = i % K::CB, wr = i / K::CB;
      const float* s = smem + K::A_DW + ch * K::CSB + wr * K::RSB;
      u32x4 p[3][3];                                         // [8-column group][piece]
#pragma unroll
      for (int k = 0; k < 3; ++k) split8_planes(s + 8 * k, p[k][0], p[k][1], p[k][2]);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        char* const pm = base + K::IMG_B + q * K::PB + ((wr * 2) * K::CB + ch) * 16;
        char* const px = base + K::IMG_B + q * K::PB + K::BM + ((wr * 2) * K::CB + ch) * 8;
        // even plane: P[-2], P[-1] = columns 0, 2; P[0 .. 7] = columns 4 .. 18; P[8], P[9] = columns 20, 22.  Odd plane: the columns + 1
        *reinterpret_cast<u32x4*>(pm) = u32x4{p[0][q][2], p[1][q][0], p[1][q][2], p[2][q][0]};
        *reinterpret_cast<u32x4*>(pm + K::CB * 16) = u32x4{p[0][q][3], p[1][q][1], p[1][q][3], p[2][q][1]};
        *reinterpret_cast<u32x2*>(px) = u32x2{p[2][q][2], p[0][q][0]};                       // (next | previous)
        *reinterpret_cast<u32x2*>(px + K::CB * 8) = u32x2{p[2][q][3], p[0][q][1]};
      }
    }
  }
}

// what a lane reads of one window row: per piece the aligned 8 elements of both planes and their neighbour dwords
struct RowB { u32x4 e[3], o[3]; unsigned en[3], ep[3], op[3]; };

template <class K>
__device__ __forceinline__ void load_row(RowB& r, const char* bm, const char* bx, int ky) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const char* m = bm + q * K::PB + ky * (2 * K::CB * 16);
    const char* x = bx + q * K::PB + ky * (2 * K::CB * 8);
    r.e[q] = *reinterpret_cast<const u32x4*>(m);
    r.o[q] = *reinterpret_cast<const u32x4*>(m + K::CB * 16);
    const u32x2 t = *reinterpret_cast<const u32x2*>(x);
    r.en[q] = t[0]; r.ep[q] = t[1];
    r.op[q] = *reinterpret_cast<const unsigned*>(x + K::CB * 8 + 4);
  }
}

__device__ __forceinline__ unsigned ab16(unsigned hi, unsigned lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }

// The chunk's k-step: 25 taps x MA channel groups x 6 products.  am: the lane's address in the `a` image (piece 0, group 0); bm / bx: in
// the main / extra `b` image (piece 0, window row 2 * (its k-group's row), even plane); mask4: 0xffff0000 where pixel j = 4 lies beyond the
// row end, else all ones.  The reads of window row ky + 1 are issued in front of the MFMAs of ky.
template <class K>
__device__ __forceinline__ void compute_chunk(const char* am, const char* bm, const char* bx, unsigned mask4, f32x4 (&acc)[K::TILES]) {
  constexpr int MA = K::MA;
  u32x4 av[MA][3];
#pragma unroll
  for (int ma = 0; ma < MA; ++ma)
#pragma unroll
    for (int q = 0; q < 3; ++q) av[ma][q] = *reinterpret_cast<const u32x4*>(am + q * K::PA + ma * 256);
  RowB row[2];
  load_row<K>(row[0], bm, bx, 0);
#pragma unroll
  for (int ky = 0; ky < 5; ++ky) {
    if (ky + 1 < 5) load_row<K>(row[(ky + 1) & 1], bm, bx, ky + 1);
    __builtin_amdgcn_sched_barrier(0);
    const RowB& r = row[ky & 1];
    u32x4 bop[5][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const u32x4 E = r.e[q], O = r.o[q];
      const unsigned e10 = ab16(E[1], E[0]), e21 = ab16(E[2], E[1]), e32 = ab16(E[3], E[2]);
      bop[0][q] = u32x4{ab16(E[0], r.ep[q]), e10, e21 & mask4, e32};
      bop[1][q] = u32x4{ab16(O[0], r.op[q]), ab16(O[1], O[0]), ab16(O[2], O[1]) & mask4, ab16(O[3], O[2])};
      bop[2][q] = E;
      bop[3][q] = O;
      bop[4][q] = u32x4{e10, e21, e32, ab16(r.en[q], E[3])};
    }
    // small terms first: (a piece, b piece) = mm, lh, hl, mh, hm, hh; the 5 MA accumulators of the row between two MFMAs on the same one
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int kx = 0; kx < 5; ++kx)
#pragma unroll
        for (int ma = 0; ma < MA; ++ma) {
          const int ti = ma * K::T + ky * 5 + kx;
          acc[ti] = piece_mfma_16x16x32(i, av[ma], bop[kx], acc[ti]);
        }
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <class K>
__global__ void __launch_bounds__(256, 1) conv_wgrad_bf16x3(Args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % K::WM, wn = wave / K::WM;

  // ---- task: (K part, channel block), as conv_wgrad
  unsigned t;
  if (!xcd_task(blockIdx.x, a.total, t)) return;
  const int nblk = a.nblk_a * a.nblk_b;
  const int part = (int)(t / (unsigned)nblk), blk = (int)(t % (unsigned)nblk);
  const int ca0 = (blk / a.nblk_b) * K::CA, cb0 = (blk % a.nblk_b) * K::CB;
  const int u0 = part_begin(part, a.ksplit, a.U), u1 = part_begin(part + 1, a.ksplit, a.U);

  // ---- LDS-DMA plan: run = i * NW + wave, slot = 64 * run + lane
  const unsigned planeA = (unsigned)(a.Ha * a.Wa), planeB = (unsigned)(a.Hb * a.Wb);
  unsigned pa_off[K::RPW_A], pa_rc[K::RPW_A], pb_off[K::RPW_B], pb_rc[K::RPW_B];
#pragma unroll
  for (int i = 0; i < K::RPW_A; ++i) {
    const int s = (i * K::NW + wave) * 64 + lane;
    const int ch = s / K::SLOTS_CA, d = (s % K::SLOTS_CA) * 4, r = d / K::XT, x = d % K::XT;
    const bool ok = s < K::SLOTS_A && d < K::R * K::XT && ca0 + ch < a.Ca;
    pa_off[i] = ok ? (unsigned)ch * planeA + (unsigned)(r * a.Wa + x) : 0u;
    pa_rc[i] = ok ? ((unsigned)r | ((unsigned)x << 8)) : 0xffffffffu;
  }
#pragma unroll
  for (int i = 0; i < K::RPW_B; ++i) {
    const int s = (i * K::NW + wave) * 64 + lane;
    const int ch = s / K::SLOTS_CB, d = (s % K::SLOTS_CB) * 4, wr = d / K::RSB, wc = d % K::RSB;
    const bool ok = s < K::SLOTS_B && d < K::WR * K::RSB && cb0 + ch < a.Cb;
    pb_off[i] = ok ? (unsigned)ch * planeB : 0u;
    pb_rc[i] = ok ? ((unsigned)wr | ((unsigned)wc << 16)) : 0x7fffu;
  }
  const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)smem;

  auto chunk_at = [&](int u, int xb) -> Chunk {
    const int n = u / a.Ha, y = u - n * a.Ha;
    int rv = a.Ha - y;
    if (rv > u1 - u) rv = u1 - u;
    if (rv > K::R) rv = K::R;
    return Chunk{n, y, rv, xb * K::XT};
  };

  f32x4 acc[K::TILES];
#pragma unroll
  for (int i = 0; i < K::TILES; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int g = lane >> 4, n16 = lane & 15;
  const char* const base = reinterpret_cast<const char*>(smem);
  const char* const am = base + K::IMG_A + (g * K::CA + (wm * K::MA) * 16 + n16) * 16;
  int u = u0, xb = 0;
  Chunk c = chunk_at(u, xb);
  stage_chunk<K>(a, c, ca0, cb0, lds_base, wave, pa_off, pa_rc, pb_off, pb_rc);
  while (true) {
    int un = u, xbn = xb + 1;
    if (xbn >= a.nxb) { xbn = 0; un = u + c.rvalid; }
    const bool has_next = un < u1;
    wait_vmcnt<0>();                     // this wave's part of the stage has landed
    __syncthreads();                     // ... everyone's; and every wave is done with the images of the chunk before
    split_stage<K>(smem, tid);
    __syncthreads();                     // the images are whole, the stage is free
    const int gr = g < c.rvalid ? g : c.rvalid - 1;      // k-groups beyond the valid rows: the window of the last valid row, against zeros
    const unsigned mask4 = (c.x0 + 4 >= a.Wa) ? 0xffff0000u : 0xffffffffu;
    if (has_next) {
      c = chunk_at(un, xbn);
      stage_chunk<K>(a, c, ca0, cb0, lds_base, wave, pa_off, pa_rc, pb_off, pb_rc);
    }
    const int bsel = (2 * gr * 2) * K::CB + wn * 16 + n16;
    compute_chunk<K>(am, base + K::IMG_B + bsel * 16, base + K::IMG_B + K::BM + bsel * 8, mask4, acc);
    if (!has_next) break;
    u = un; xb = xbn;
  }

  // ---- epilogue: the accumulator tiles as they are (lane l holds D[4 (l >> 4) + j][l & 15], j = 0..3), 16-byte stores
  float* dst = a.slab + (size_t)part * (size_t)a.slab_part + (((size_t)blk * 4 + wave) * K::TILES) * 256 + lane * 4;
#pragma unroll
  for (int i = 0; i < K::TILES; ++i) *reinterpret_cast<f32x4*>(dst + (size_t)i * 256) = acc[i];
}

template <class K>
static int launch(const Args& base, hipStream_t st) {
  Args a = base;             // (total: set by the caller, within the limit by make_plan)
  return launch_tiles<&conv_wgrad_bf16x3<K>>(a, a.total, K::THREADS, K::LDS_BYTES, "conv_wgrad_bf16x3", "conv_wgrad_bf16x3", st);
}

struct Variant {
  int ca, cb, tiles;
  SlabMap map;
  int (*fn)(const Args&, hipStream_t);
};

#define FN2_WX_ROW(MA) {Cfg<MA>::CA, Cfg<MA>::CB, Cfg<MA>::TILES, SlabMap{MA, 1, 2, 2, 25, Cfg<MA>::CA, Cfg<MA>::CB, Cfg<MA>::TILES}, &launch<Cfg<MA>>},
static const Variant kVariants[] = {FN2_WX_ROW(2) FN2_WX_ROW(1)};
FN2_BF16X3_VARIANT_KNOBS(conv_wgrad_bf16x3)

// The K split of a layer in this arithmetic: the exact kernel's (a function of the geometry only), with at least 4 rows -- one k-step -- per part
inline int ksplit_for_split(int N, int Ca, int Ha, int Wa, int Cb) {
  const int k = wg::ksplit_for(N, Ca, Ha, Wa, Cb, 5), cap = N * Ha / 4;
  return k < cap ? k : (cap < 1 ? 1 : cap);
}

struct Plan { int ksplit; size_t slab_floats[kNumVariants], slab_max; };

// a [N, Ca, Ha, Wa] = top_diff, b [N, Cb, Hb, Wb] = bottom of a Convolution{5, 2, 2}
static bool make_plan(Plan& p, int N, int Ca, int Ha, int Wa, int Cb, int Hb, int Wb) {
  if (N <= 0 || Ca < 16 || Cb < 16 || Ha <= 0 || Wa <= 0 || Hb <= 0 || Wb <= 0) return false;
  if (Wa % 4 != 0 || Wb % 4 != 0) return false;
  if (Ha != (Hb - 1) / 2 + 1 || Wa != (Wb - 1) / 2 + 1) return false;                    // the maps of one 5 / 2 / 2 layer
  if (64ll * Ha * Wa >= (1ll << 28) || 32ll * Hb * Wb >= (1ll << 28) || (long long)N * Ha >= (1ll << 30)) return false;      // descriptor range
  p.ksplit = ksplit_for_split(N, Ca, Ha, Wa, Cb);
  p.slab_max = 0;
  for (int i = 0; i < kNumVariants; ++i) {
    const Variant& v = kVariants[i];
    p.slab_floats[i] = (size_t)wg::cdiv_c(Ca, v.ca) * wg::cdiv_c(Cb, v.cb) * 4 * v.tiles * 256;
    if ((long long)wg::cdiv_c(Ca, v.ca) * wg::cdiv_c(Cb, v.cb) * p.ksplit > 0x3fffff00ll) return false;
    if (p.slab_floats[i] > p.slab_max) p.slab_max = p.slab_floats[i];
  }
  return true;
}

static bool plan_of(Plan& p, const fn2_conv_desc* d, int transposed) {
  if (transposed || !d || d->N < 1 || d->Cin < 1 || d->Cout < 1 || d->Hin < 1 || d->Win < 1 || d->kernel != 5 || d->stride != 2 || d->pad != 2) return false;
  return make_plan(p, d->N, d->Cout, (d->Hin - 1) / 2 + 1, (d->Win - 1) / 2 + 1, d->Cin, d->Hin, d->Win);
}

}  // namespace wgx

size_t conv_wgrad_bf16x3_workspace_bytes(const fn2_conv_desc* d, int transposed) {
  wgx::Plan p;
  return wgx::plan_of(p, d, transposed) ? sizeof(float) * (size_t)p.ksplit * p.slab_max : 0;
}

int conv_wgrad_bf16x3(const fn2_conv_desc* d, int transposed, const float* bottom, int bottom_channels, int bottom_c0, const float* top_diff,
                      int top_channels, int top_c0, float* weight_diff, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  wgx::Plan p;
  if (!wgx::plan_of(p, d, transposed)) return fail(FN2_ERR_UNSUPPORTED, "conv_wgrad_bf16x3: the split-bf16 weight gradient does not take this layer");
  if (!bottom || !top_diff || !weight_diff) return fail(FN2_ERR_INVALID_ARG, "conv_wgrad_bf16x3: null blob");
  if (top_c0 < 0 || top_c0 + d->Cout > top_channels || bottom_c0 < 0 || bottom_c0 + d->Cin > bottom_channels)
    return fail(FN2_ERR_INVALID_ARG, "conv_wgrad_bf16x3: channel slice outside the blob");
  const int v = wgx::g_forced_variant < 0 ? 0 : wgx::g_forced_variant;
  if (v >= wgx::kNumVariants) return fail(FN2_ERR_UNSUPPORTED, "conv_wgrad_bf16x3: forced variant %d does not exist", v);
  const size_t need = sizeof(float) * (size_t)p.ksplit * p.slab_max;
  if (!workspace || workspace_bytes < need) return fail(FN2_ERR_WORKSPACE, "conv_wgrad_bf16x3: workspace of %zu bytes needed", need);
  if (((reinterpret_cast<uintptr_t>(bottom) | reinterpret_cast<uintptr_t>(top_diff) | reinterpret_cast<uintptr_t>(workspace)) & 15) != 0)
    return fail(FN2_ERR_UNSUPPORTED, "conv_wgrad_bf16x3: blobs and workspace must be 16-byte aligned");
  const wgx::Variant& var = wgx::kVariants[v];
  hipStream_t st = as_stream(stream);
  wgx::Args g{};
  g.a = top_diff; g.b = bottom; g.slab = static_cast<float*>(workspace);
  g.N = d->N; g.Ca = d->Cout; g.Ha = (d->Hin - 1) / 2 + 1; g.Wa = (d->Win - 1) / 2 + 1; g.a_ctot = top_channels; g.a_c0 = top_c0;
  g.Cb = d->Cin; g.Hb = d->Hin; g.Wb = d->Win; g.b_ctot = bottom_channels; g.b_c0 = bottom_c0;
  g.ksplit = p.ksplit; g.nblk_a = wg::cdiv_c(g.Ca, var.ca); g.nblk_b = wg::cdiv_c(g.Cb, var.cb);
  g.nxb = wg::cdiv_c(g.Wa, 8); g.U = g.N * g.Ha;
  g.total = (unsigned)((long long)g.nblk_a * g.nblk_b * p.ksplit);
  g.slab_part = (long long)p.slab_floats[v];
  if (const int rc = var.fn(g, st)) return rc;
  return wgrad_finalize_parts(g.slab, weight_diff, var.map, g.Ca, g.Cb, g.nblk_a, g.nblk_b, p.ksplit, g.slab_part, accumulate, stream);
}

}  // namespace fn2

using namespace fn2;

// the layers this kernel takes: Convolution{5, 2, 2}, not transposed, both map widths multiples of 4, at least 16 channels on both sides
FN2_API int fn2_conv_wgrad_bf16x3_supported(const fn2_conv_desc* d, int transposed) {
  wgx::Plan p;
  return wgx::plan_of(p, d, transposed) ? 1 : 0;
}

FN2_API int fn2_conv_wgrad_bf16x3_ksplit(const fn2_conv_desc* d, int transposed) {
  wgx::Plan p;
  return wgx::plan_of(p, d, transposed) ? p.ksplit : 0;
}
