// The split-bf16 ("bf16x3") pieces shared by the kernels of that arithmetic (conv_bf16x3.hip, deconv_bf16x3.hip): the bf16 vector types
// and the cut of fp32 values into three bf16 pieces  h = rne(v), m = rne(v - h), l = rne(v - h - m)  in MFMA operand order.
#pragma once

#include "mfma_tile.hpp"

namespace fn2 {
namespace bf16x3 {

using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

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

// one k-step of the arithmetic on one accumulator: the six leading piece products, small terms first --
// (activation piece, weight piece) = mm, lh, hl, mh, hm, hh; x / w: the (h, m, l) operands of the lane
constexpr int kXPiece[6] = {1, 2, 0, 1, 0, 0}, kWPiece[6] = {1, 0, 2, 0, 1, 0};

}  // namespace bf16x3
}  // namespace fn2
