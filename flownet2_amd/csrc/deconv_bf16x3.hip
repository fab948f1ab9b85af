// The GEMM of the Deconvolution{4, 2, 1} (FN2_DECONV_ROUTE_GEMM: weight^T x bottom into the column matrix, then col2im + bias + ReLU) in
// SPLIT-bf16 ("bf16x3") arithmetic on v_mfma_f32_16x16x32_bf16: an opt-in second arithmetic for the 1x1 form of csrc/conv_mfma.hip.  Per
// sample  col[M = 16 Cout][P = Hin Win] = A[M][K = Cin] . B[K][P];  B is the layer's channel slice of the bottom blob (NCHW: pixels
// contiguous, channel stride P), row m = (co, ky, kx) of A is weight[.][co][ky][kx] of Caffe's [Cin][Cout][4][4] blob, and col has the
// layout fn2_col2im_bias_relu_forward_into reads.  One launch per mini-batch, no workspace of its own, no pre-split copy of the activations.
//
// Arithmetic: that of csrc/conv_bf16x3.hip (FN2_CONV_ARITH_BF16X3, include/flownet2_hip.h).  Every fp32 value is cut into three bf16
// pieces  h = rne(v), m = rne(v - h), l = rne(v - h - m);  the six leading piece products are summed in fp32 on ONE accumulator in the
// order mm, lh, hl, mh, hm, hh (first letter: the activation's piece).  The k-steps are blocks of 32 input channels in ascending channel
// order; there is no K split, and a k-step beyond the layer's last one is skipped, not run on zeros.  So the summation order of an
// output depends on neither the tile variant nor the batch nor the run: every variant writes the same bits.
// Ragged last k-step: channels >= Cin carry zero weights AND zero activations (the loads are not issued: nothing of a wider bottom blob's
// neighbouring channels enters, NaN x 0 cannot arise); pixels >= P of a tile hanging over the plane are zeros too and are never stored.
//
// Operands.
//   * weights: split once when packed (fn2::deconv_bf16x3_pack_weights), [M / 16][k-step (+ 1 spare)][piece][lane][8 bf16]: lane
//     (row = lane & 15, kq = lane >> 4) holds channels 32 ks + 8 kq + j of row 16 g + (lane & 15) -- one global_load_dwordx4 per lane,
//     piece and row group.  The spare k-step (zeros, never read) makes the operand's length differ from the exact GEMM operand's for
//     every layer -- without it the two are equally long at 33 .. 64 input channels -- so that a length check tells the two apart.
//   * activations: a workgroup tile is TP pixels x a chunk of KS k-steps with TP / 4 x 4 KS == 256 (128 pixels x 64 channels, or 64 pixels
//     x 128 channels).  Each thread fetches one pixel quad of 8 channels (8 x global_load_dwordx4, a chunk ahead of its use), splits the four
//     pixels in registers (split8) and writes three 16-byte entries per pixel into the LDS image [piece][channel octet][pixel]; a lane's
//     operand is one ds_read_b128 per piece.  Octet o lies at (o >> 1) (2 TP + 1) + (o & 1) TP entries: the odd octet of a pair a multiple
//     of 16 entries on, so the 16-lane groups of a ds_read_b128 (8 pixels of an even octet, the 8 OTHER pixels of its odd neighbour) fill
//     the 256-byte bank row exactly; and pairs an odd number of entries apart, so the 8 lanes of a ds_write_b128 (4 octet pairs x 2
//     neighbouring quads, or 8 octet pairs) take 8 different slots of the 128-byte row.  One image: barrier -> split -> barrier ->
//     (fetch of the next chunk) + MFMAs; the other workgroups of the CU compute meanwhile.
//   * 4 waves; wave tile 4 or 2 row groups x 4 pixel groups; workgroup tiles of 128 x 128, 64 x 128 and 128 x 64 (rows x pixels).  A tile
//     may hang over the M edge (whole 16-row groups idle: they re-read the last group and store nothing) and over the pixel edge
//     (P % 4 == 0: whole 16-byte stores).  The 64-pixel tile wastes less of a plane just over a multiple of 64 pixels (deconv4: 140).
// Build figures (hipcc -O3, gfx950, from -Rpass-analysis=kernel-resource-usage), variant 0 / 1 / 2 = 128 x 128 / 64 x 128 / 128 x 64 tiles:
// 236 / 158 / 160 VGPRs, 49,344 / 49,344 / 49,536 bytes of LDS, no spills, no scratch; 2 / 3 / 3 workgroups per CU (__launch_bounds__).
// Measured on an MI355X at deconv4 / 3 / 2 of FlowNetC, batch 8 @448x320 (profiles/deconv_bf16x3_bench.md): the whole deconvolution takes
// 0.80 / 0.81 / 0.75 of the exact route's time (the GEMM alone 0.78 / 0.80 / 0.72; the arithmetic floor is 6/16 = 0.375); the 128 x 64 tile is the fastest at all three.
#include "conv_internal.hpp"
#include "mfma_tile.hpp"
#include "split_bf16.hpp"

namespace fn2 {
namespace dx {

using namespace mfma;
using namespace bf16x3;

struct Args {
  const float* in; const u32x4* wp; float* col;
  int N, Cin, P, in_ctot, in_c0;
  int M;              // 16 Cout
  int ksteps;         // blocks of 32 channels
  int kalloc;         // k-steps of the packed weights per 16-row group, the spare one included
  int nchunks;        // chunks of KS k-steps
  int mt, pt;         // workgroup tiles along M / P
  unsigned total;     // tiles = workgroups
};

template <int MW_, int WM_, int WN_, int KS_, int WGS_>
struct Cfg {
  static constexpr int MW = MW_, NPW = 4, WM = WM_, WN = WN_, WGS = WGS_;      // WGS: workgroups per CU the registers must allow
  static constexpr int THREADS = 64 * WM * WN;
  static constexpr int TM = 16 * MW * WM, TP = 16 * NPW * WN;        // rows / pixels of a workgroup tile
  static constexpr int KS = KS_, OCT = 4 * KS;                       // k-steps and channel octets of a chunk
  static constexpr int S2 = 2 * TP + 1, PS = (OCT / 2) * S2;         // image: entries between octet pairs / pieces
  static constexpr int LDS_BYTES = 3 * PS * 16;
  // k-steps whose weight operands are fetched ahead = what the registers hold (two of them in the 128-channel chunks: 59 VGPRs spilled)
  static constexpr int EARLY = MW <= 2 && KS <= 2 ? 2 : 1;
  static_assert(THREADS == 256 && (TP / 4) * OCT == THREADS, "one (octet, pixel quad) per thread");
  static_assert(TP % 16 == 0 && S2 % 8 == 1, "bank rules of the 16-byte LDS accesses");
};

template <class K>
__device__ __forceinline__ void fetch_chunk(const Args& a, const float* src, bool pix_ok, int ch0, f32x4 (&xr)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ch = ch0 + j;
    xr[j] = (pix_ok && ch < a.Cin) ? *reinterpret_cast<const f32x4*>(src + (size_t)ch * a.P) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

template <class K>
__device__ __forceinline__ void split_chunk(u32x4* img, int widx, const f32x4 (&xr)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = xr[j][i];
    store_pieces(img + widx + i, K::PS, v);
  }
}

template <class K>
__device__ __forceinline__ void load_weights(const u32x4* const (&wl)[K::MW], int ks, u32x4 (&w)[K::MW][3]) {
#pragma unroll
  for (int j = 0; j < K::MW; ++j) load_pieces(wl[j], (size_t)ks, w[j]);
}

template <class K>
__device__ __forceinline__ void gemm_body(const Args& a, int mtile, int ptile, int n) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int MW = K::MW, NPW = K::NPW;
  u32x4* const img = reinterpret_cast<u32x4*>(smem);                // [piece][octet pair][octet & 1][pixel]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % K::WM, wn = wave / K::WM;
  const int p0 = ptile * K::TP;

  // ---- staging task of this thread: octet 2 so2 + so1 of the chunk, pixel quad squad of the tile
  const int so2 = tid % (K::OCT / 2), squad = (tid / (K::OCT / 2)) % (K::TP / 4), so1 = tid / (K::THREADS / 2);
  const int spix = p0 + 4 * squad;
  const bool pix_ok = spix < a.P;                                    // (P % 4 == 0: a quad is inside the plane or outside it)
  const float* src = a.in + ((size_t)n * a.in_ctot + a.in_c0) * a.P + (pix_ok ? spix : 0);
  const int soct8 = 8 * (2 * so2 + so1);
  const int widx = so2 * K::S2 + so1 * K::TP + 4 * squad;

  // ---- operands of this lane
  const int cg0 = (mtile * K::WM + wm) * MW;                         // first 16-row group of this wave
  const u32x4* wl[MW];                                               // group cg0 + j, k-step ks: load_pieces(wl[j], ks, ..)
#pragma unroll
  for (int j = 0; j < MW; ++j)                                       // (a group outside the matrix re-reads the last one and stores nothing)
    wl[j] = packed_lane(a.wp, min(cg0 + j, a.M / 16 - 1), a.kalloc, lane);
  const int kq = lane >> 4;
  const int ridx = (kq >> 1) * K::S2 + (kq & 1) * K::TP + 16 * NPW * wn + (lane & 15);

  f32x4 acc[MW][NPW];
#pragma unroll
  for (int j = 0; j < MW; ++j)
#pragma unroll
    for (int p = 0; p < NPW; ++p) acc[j][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 xr[8];
  fetch_chunk<K>(a, src, pix_ok, soct8, xr);
  for (int c = 0; c < a.nchunks; ++c) {
    // the weight operands of this chunk's k-steps: in flight through the split and the barriers
    u32x4 w[K::KS][MW][3];
#pragma unroll
    for (int s = 0; s < K::EARLY; ++s)
      if (K::KS * c + s < a.ksteps) load_weights<K>(wl, K::KS * c + s, w[s]);
    __syncthreads();                     // every wave is done with the image of chunk c - 1
    split_chunk<K>(img, widx, xr);
    __syncthreads();                     // the image is whole
    if (c + 1 < a.nchunks) fetch_chunk<K>(a, src, pix_ok, 8 * K::OCT * (c + 1) + soct8, xr);
#pragma unroll
    for (int s = 0; s < K::KS; ++s) {
      if (K::KS * c + s < a.ksteps) {
        // (the operands of k-step s - 1 are spent: their registers take the k-step EARLY - 1 ahead)
        if (s > 0 && s - 1 + K::EARLY < K::KS && K::KS * c + s - 1 + K::EARLY < a.ksteps) load_weights<K>(wl, K::KS * c + s - 1 + K::EARLY, w[s - 1 + K::EARLY]);
        u32x4 x[NPW][3];
#pragma unroll
        for (int p = 0; p < NPW; ++p)
#pragma unroll
          for (int q = 0; q < 3; ++q) x[p][q] = img[q * K::PS + 2 * s * K::S2 + ridx + 16 * p];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < MW; ++j)
#pragma unroll
            for (int p = 0; p < NPW; ++p)
              acc[j][p] = piece_mfma_16x16x32(i, x[p], w[s][j], acc[j][p]);
      }
    }
  }

  // ---- epilogue: lane (pixel quad = lane >> 4, row = lane & 15) holds 4 consecutive pixels of row 16 (cg0 + j) + (lane & 15)
#pragma unroll
  for (int j = 0; j < MW; ++j) {
    if (16 * (cg0 + j) < a.M) {
      float* crow = a.col + ((size_t)n * a.M + 16 * (cg0 + j) + (lane & 15)) * a.P;
#pragma unroll
      for (int p = 0; p < NPW; ++p) {
        const int pix = p0 + 16 * (NPW * wn + p) + 4 * (lane >> 4);
        if (pix < a.P) *reinterpret_cast<f32x4*>(crow + pix) = acc[j][p];
      }
    }
  }
}

// Task list: (sample, pixel tile, row tile), row tile fastest (xcd_task: neighbours share the activation tile)
template <class K>
__global__ void __launch_bounds__(256, K::WGS)
deconv_bf16x3_gemm(Args a) {
  unsigned t;
  if (!xcd_task(blockIdx.x, a.total, t)) return;
  const int mtile = t % a.mt; t /= a.mt;
  gemm_body<K>(a, mtile, (int)(t % a.pt), (int)(t / a.pt));
}

// weight [Cin][Cout][4][4] = [Cin][M] -> the packed layout of split_bf16.hpp, groups of 16 rows of M
__global__ void __launch_bounds__(256) pack_weights(const float* __restrict__ wsrc, u32x4* __restrict__ wp, int M, int Cin, int ksteps) {      // ksteps: kalloc
  int lane, ks, grp;
  if (!pack_thread(M / 16, ksteps, lane, ks, grp)) return;
  const int m = 16 * grp + (lane & 15);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = 32 * ks + 8 * (lane >> 4) + j;
    v[j] = ci < Cin ? wsrc[(size_t)ci * M + m] : 0.f;
  }
  u32x4 h, mm, l;                    // (store_pieces, written out: through the helper this kernel allocates other registers)
  split8(v, h, mm, l);
  u32x4* dst = wp + ((size_t)grp * ksteps + ks) * kStepVecs + lane;
  dst[0] = h; dst[kPieceVecs] = mm; dst[2 * kPieceVecs] = l;
}

template <class K>
static int launch(const Args& base, hipStream_t st) {
  Args a = base;
  a.mt = cdiv(a.M, K::TM); a.pt = cdiv(a.P, K::TP);
  a.nchunks = cdiv(a.ksteps, K::KS);
  return launch_tiles<&deconv_bf16x3_gemm<K>>(a, (long long)a.N * a.mt * a.pt, K::THREADS, K::LDS_BYTES, "deconv_bf16x3", "deconv_bf16x3_gemm", st);
}

struct Variant {
  int tm, tp, wgs;
  int (*fn)(const Args&, hipStream_t);
};

#define FN2_DX_ROW(MW, WM, WN, KS, WGS) {Cfg<MW, WM, WN, KS, WGS>::TM, Cfg<MW, WM, WN, KS, WGS>::TP, WGS, &launch<Cfg<MW, WM, WN, KS, WGS>>},
// rows x pixels of the workgroup tile: 128 x 128 and 64 x 128 (2 x 2 waves, chunks of 64 channels), 128 x 64 (4 x 1 waves, chunks of 128
// channels: planes just over a multiple of 64 pixels -- deconv4's 140 -- waste less of it)
static const Variant kVariants[] = {FN2_DX_ROW(4, 2, 2, 2, 2) FN2_DX_ROW(2, 2, 2, 2, 3) FN2_DX_ROW(2, 4, 1, 4, 3)};
FN2_BF16X3_VARIANT_KNOBS(deconv_bf16x3)

constexpr int kstep_alloc(int Cin) { return cdiv(Cin, 32) + 1; }

// Cost model: rounds of workgroups over the chip's slots (256 CUs x workgroups per CU) x the tile's area (what hangs over the edges
// included) x workgroups sharing a CU; the 128-channel chunks first among equals (half the barriers per product)
static double variant_cost(const Variant& v, const Args& a) {
  const long long wgs = (long long)a.N * cdiv(a.M, v.tm) * cdiv(a.P, v.tp), slots = 256 * v.wgs;
  return (double)((wgs + slots - 1) / slots) * v.tm * v.tp * v.wgs * (v.tp == 64 ? 1.0 : 1.1);      // (128 x 64: the fastest at all three FlowNetC shapes)
}

bool geometry_ok(int Cin, int Hin, int Win, int Cout) {
  if (Cin < 1 || Hin < 1 || Win < 1 || Cout < 1) return false;
  const long long P = (long long)Hin * Win, M = 16ll * Cout;
  // whole waves of 32 rows, whole 16-byte pixel quads; every in-sample offset fits 31 bits
  return M % 32 == 0 && P % 4 == 0 && M * P < (1ll << 31) && (long long)Cin * P < (1ll << 31);
}

}  // namespace dx

size_t deconv_bf16x3_packed_floats(int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0 || (16 * (long long)Cout) % 32 != 0) return 0;
  return bf16x3::packed_floats(Cout, dx::kstep_alloc(Cin));
}

int deconv_bf16x3_pack_weights(const float* weight, float* packed, int Cin, int Cout, void* stream) {
  const int kalloc = dx::kstep_alloc(Cin);          // (channels >= Cin, the spare k-step among them: zeros)
  return bf16x3::pack_operand("deconv_bf16x3_pack_weights", weight, packed, deconv_bf16x3_packed_floats(Cin, Cout) != 0,
                              [&] { return fail(FN2_ERR_UNSUPPORTED, "deconv_bf16x3_pack_weights: needs Cout %% 2 == 0 (got %d)", Cout); },
                              Cout, kalloc, stream, dx::pack_weights, 16 * Cout, Cin, kalloc);
}

int deconv_bf16x3_gemm(const float* bottom, const float* packed_weight, float* col, int N, int Cin, int Hin, int Win, int bottom_channels,
                       int bottom_c0, int Cout, void* stream) {
  if (N < 0) return fail(FN2_ERR_INVALID_ARG, "deconv_bf16x3: bad batch");
  if (N == 0) return FN2_OK;
  if (const int rc = mfma::check_conv_args("deconv_bf16x3", bottom, packed_weight, col, Cin, bottom_channels, bottom_c0, Cout, Cout, 0, [&] {
        return dx::geometry_ok(Cin, Hin, Win, Cout) ? FN2_OK
            : fail(FN2_ERR_UNSUPPORTED, "deconv_bf16x3: unsupported geometry (Cin %d, %dx%d, Cout %d)", Cin, Hin, Win, Cout);
      }))
    return rc;
  dx::Args a{};
  a.in = bottom; a.wp = reinterpret_cast<const dx::u32x4*>(packed_weight); a.col = col;
  a.N = N; a.Cin = Cin; a.P = Hin * Win; a.in_ctot = bottom_channels; a.in_c0 = bottom_c0;
  a.M = 16 * Cout; a.ksteps = mfma::cdiv(Cin, 32); a.kalloc = dx::kstep_alloc(Cin);
  hipStream_t st = as_stream(stream);
  static TuneCache cache("deconv_bf16x3", dx::kNumVariants);
  const TuneKey key{N, Cin, Hin, Win, Cout, bottom_channels == Cin, 0, 0, 0, 0};
  return bf16x3::pick_and_run("deconv_bf16x3", dx::g_forced_variant, dx::kNumVariants, cache, key, st, [](int) { return true; },
                              [&](int i) { return dx::variant_cost(dx::kVariants[i], a); }, [&](int i) { return dx::kVariants[i].fn(a, st); });
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_deconv_bf16x3_supported(const fn2_conv_desc* d) {
  if (!d || d->N < 1 || d->kernel != 4 || d->stride != 2 || d->pad != 1) return 0;
  return dx::geometry_ok(d->Cin, d->Hin, d->Win, d->Cout) ? 1 : 0;
}
