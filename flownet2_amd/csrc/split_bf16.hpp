// The split-bf16 ("bf16x3") toolkit: what the six kernels of that arithmetic share.
//   serves   conv_bf16x3.hip (direct 5x5 / 2), deconv_bf16x3.hip (deconvolution GEMM), correlation_bf16x3.hip, tconv_bf16x3.hip (stride-2 data
//            gradient), conv_wino_bf16x3.hip (Winograd 3x3), conv_wgrad_bf16x3.hip (5x5 / 2 weight gradient)
//   holds    the cut     piece2 / split8: fp32 values -> three bf16 pieces  h = rne(v), m = rne(v - h), l = rne(v - h - m)  in MFMA operand order;
//                        store_pieces: split8 and the three stores, one piece plane apart
//            the sum     kXPiece / kWPiece and piece_mfma_16x16x32 / piece_mfma_32x32x16: product i of the six leading piece products on one accumulator
//            the operand the packed layout [group][k-step][piece][lane] of conv, tconv and deconv (kPieceVecs, kStepVecs, packed_floats, packed_lane,
//                        load_pieces), the thread of a pack kernel (pack_thread) and the host entry of one (pack_operand)
//            the knobs   pick_and_run (pick_variant, then the pick's launch) and FN2_BF16X3_VARIANT_KNOBS (variant count, forced variant, their two
//                        C functions)
// The k loops, the images in LDS, the variants and their cost models stay with the kernels ("split-bf16 toolkit").
#pragma once

#include "mfma_tile.hpp"

namespace fn2 {
namespace bf16x3 {

using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// ------------------------------------------------------------------------------------------------ the cut
// (a, b) -> the bf16 pieces of both, packed (a in the low half), and what is left of a and b
__device__ __forceinline__ unsigned piece2(float& a, float& b) {
  const bf16x2 h = __builtin_convertvector(mfma::f32x2{a, b}, bf16x2);     // v_cvt_pk_bf16_f32: round to nearest even
  const unsigned u = __builtin_bit_cast(unsigned, h);
  a -= __builtin_bit_cast(float, u << 16);
  b -= __builtin_bit_cast(float, u & 0xffff0000u);
  return u;
}

// 8 fp32 values -> three 16-byte operands (h, m, l), element j in bits 16 (j % 2) of dword j / 2
__device__ __forceinline__ void split8(float (&v)[8], u32x4& h, u32x4& m, u32x4& l) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = piece2(v[2 * i], v[2 * i + 1]);
    m[i] = piece2(v[2 * i], v[2 * i + 1]);
    l[i] = piece2(v[2 * i], v[2 * i + 1]);
  }
}

// split8, then h / m / l to dst, dst + stride, dst + 2 stride (stride: the 16-byte vectors between two piece planes)
__device__ __forceinline__ void store_pieces(u32x4* dst, int stride, float (&v)[8]) {
  u32x4 h, m, l;
  split8(v, h, m, l);
  dst[0] = h; dst[stride] = m; dst[2 * stride] = l;
}

// ------------------------------------------------------------------------------------------------ the sum
// one k-step of the arithmetic on one accumulator: the six leading piece products, small terms first --
// (activation piece, weight piece) = mm, lh, hl, mh, hm, hh; x / w: the (h, m, l) operands of the lane
constexpr int kXPiece[6] = {1, 2, 0, 1, 0, 0}, kWPiece[6] = {1, 0, 2, 0, 1, 0};

// product i of the six on acc (i: the counter of an unrolled loop)
__device__ __forceinline__ mfma::f32x4 piece_mfma_16x16x32(int i, const u32x4 (&x)[3], const u32x4 (&w)[3], mfma::f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x[kXPiece[i]]), __builtin_bit_cast(bf16x8, w[kWPiece[i]]), acc, 0, 0, 0);
}

__device__ __forceinline__ f32x16 piece_mfma_32x32x16(int i, const u32x4 (&x)[3], const u32x4 (&w)[3], f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x[kXPiece[i]]), __builtin_bit_cast(bf16x8, w[kWPiece[i]]), acc, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ the packed operand
// The weight operand of conv, tconv and deconv, split once when packed:  [group of 16 rows][kalloc k-steps][piece h, m, l][64 lanes][8 bf16].
// A lane's operand of a k-step and piece is one 16-byte vector (one global_load_dwordx4), the pieces kPieceVecs apart, the k-steps
// kStepVecs.  kalloc = the layer's k-steps + 1: the kernels fetch a k-step ahead, so every group ends in a spare k-step of zeros.
// (conv_wino_bf16x3 keeps the pieces of its 16 positions together: [group of 32][kalloc][position][piece][lane], 16 kStepVecs per k-step.)
constexpr int kPieceVecs = 64;                  // 16-byte vectors of one piece of a k-step: one per lane
constexpr int kStepVecs = 3 * kPieceVecs;       // ... of a k-step

constexpr size_t packed_floats(size_t groups, size_t kalloc) { return groups * kalloc * kStepVecs * 4; }

// this lane's vector of (k-step 0, piece h) of `group`
__device__ __forceinline__ const u32x4* packed_lane(const u32x4* wp, int group, int kalloc, int lane) {
  return wp + (size_t)group * kalloc * kStepVecs + lane;
}

// the three pieces of k-step ks, from packed_lane's pointer
__device__ __forceinline__ void load_pieces(const u32x4* wl, size_t ks, u32x4 (&w)[3]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) w[q] = wl[ks * kStepVecs + kPieceVecs * q];
}

// A pack kernel runs one thread per (group, k-step, lane) in blocks of 256: this thread's three.  false: it is past the last one
__device__ __forceinline__ bool pack_thread(int groups, int kalloc, int& lane, int& ks, int& grp) {
  const long long total = (long long)groups * kalloc * 64;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return false;
  lane = (int)(i & 63), ks = (int)((i >> 6) % kalloc), grp = (int)((i >> 6) / kalloc);
  return true;
}

// The host entry of a pack kernel: both blobs present, the layer has a layout (else `refuse()`, the kernel's own refusal), the operand
// 16-byte aligned; then kernel(weight, packed, args...) on groups x kalloc x 64 threads.  what: "<kernel>_pack_weights"
template <class Refuse, class Kernel, class... A>
int pack_operand(const char* what, const float* weight, float* packed, bool has_layout, Refuse refuse, int groups, int kalloc, void* stream,
                 Kernel kernel, A... args) {
  if (!weight || !packed) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (!has_layout) return refuse();
  if ((reinterpret_cast<uintptr_t>(packed) & 15) != 0) return fail(FN2_ERR_UNSUPPORTED, "%s: the operand must be 16-byte aligned", what);
  const long long total = (long long)groups * kalloc * 64;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), weight, reinterpret_cast<u32x4*>(packed), args...);
  return check_launch(what);
}

// ------------------------------------------------------------------------------------------------ the knobs
// mfma::pick_variant among a family's variants (none has a split tail), then the launch of the pick.
//   applies(i), cost(i): as pick_variant's;  run(i): launches variant i
template <class Applies, class Cost, class Run>
int pick_and_run(const char* what, int forced, int nvariants, TuneCache& cache, const TuneKey& key, hipStream_t st, Applies applies, Cost cost, Run run) {
  mfma::Pick p;
  if (const int rc = mfma::pick_variant(p, what, forced, nvariants, false, cache, key, st, applies, [&](int i, bool) { return cost(i); },
                                        [&](int i, bool) { return run(i); }, [](int) { return false; }))
    return rc;
  return run(p.variant);
}

// Behind a family's kVariants, inside its namespace: the variant count, the forced variant (a debug knob, -1 = none) and the two C
// functions fn2_<NAME>_num_variants / fn2_debug_set_<NAME>_variant of include/flownet2_hip.h
#define FN2_BF16X3_VARIANT_KNOBS(NAME)                                            \
  constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);          \
  int g_forced_variant = -1;                                                      \
  FN2_API int fn2_##NAME##_num_variants(void) { return kNumVariants; }            \
  FN2_API int fn2_debug_set_##NAME##_variant(int v) { g_forced_variant = v; return FN2_OK; }

}  // namespace bf16x3
}  // namespace fn2
