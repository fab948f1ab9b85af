// Entry points shared between translation units of the library that are not part of include/flownet2_hip.h.
#pragma once

#include <cstddef>

#include "../../include/flownet2_hip.h"

namespace fn2 {

namespace wg { struct SlabMap; }

// csrc/tconv_mfma.hip: fn2_tconv_forward with the output multiplied by the leaky-ReLU derivative of `mask` (NULL: no mask)
int tconv_forward_masked(const float* bottom, const float* packed_weight, const float* bias, float* top,
                         int N, int Cin, int Hin, int Win, int bottom_channels, int bottom_c0,
                         int Cout, int Hout, int Wout, int top_channels, int top_c0, int kernel, int pad,
                         int relu, float negative_slope, const float* mask, int mask_channels, int mask_c0, float mask_slope, void* stream);

// csrc/conv_stem_wgrad.hip: fn2_conv_k7s2_wgrad; bias_diff != NULL: the bias gradient of the same layer comes out of the same pass
int conv_k7s2_wgrad_bias(const float* top_diff, const float* bottom, float* weight_diff, float* bias_diff, int N, int Cin, int Hin, int Win, int Cout,
                         int accumulate, void* workspace, size_t workspace_bytes, void* stream);

// csrc/conv_bf16x3.hip: the direct convolution in split-bf16 arithmetic (FN2_CONV_ARITH_BF16X3 beside FN2_CONV_ROUTE_DIRECT); which layers
// it takes: fn2_conv_bf16x3_supported.  The operand holds the three bf16 planes of the weights (0 floats: no operand for these channels).
size_t conv_bf16x3_packed_floats(int Cout, int Cin, int kernel);
int conv_bf16x3_pack_weights(const float* weight, float* packed, int Cout, int Cin, int kernel, void* stream);
int conv_bf16x3_forward(const float* bottom, const float* packed_weight, const float* bias, float* top, int N, int Cin, int Hin, int Win,
                        int bottom_channels, int bottom_c0, int Cout, int top_channels, int top_c0, int kernel, int stride, int pad,
                        int relu, float negative_slope, void* stream);

// csrc/conv_wino_bf16x3.hip: the Winograd F(2x2, 3x3) convolution in split-bf16 arithmetic (FN2_CONV_ARITH_BF16X3 beside
// FN2_CONV_ROUTE_WINOGRAD); which layers it takes: fn2_conv_wino_bf16x3_supported.  The operand holds the three bf16 planes of U = G g G^T:
// (Cout / 32) x (ceil(Cin / 16) + 1) x 12288 floats (0: no operand for these channels).
size_t conv_wino_bf16x3_packed_floats(int Cout, int Cin);
int conv_wino_bf16x3_pack_weights(const float* weight, float* packed, int Cout, int Cin, void* stream);
int conv_wino_bf16x3_forward(const float* bottom, const float* packed_weight, const float* bias, float* top, int N, int Cin, int Hin, int Win,
                             int bottom_channels, int bottom_c0, int Cout, int top_channels, int top_c0, int kernel, int stride, int pad,
                             int relu, float negative_slope, void* stream);

// csrc/deconv_bf16x3.hip: the GEMM of the Deconvolution{4, 2, 1} in split-bf16 arithmetic (FN2_CONV_ARITH_BF16X3 beside
// FN2_DECONV_ROUTE_GEMM); which layers it takes: fn2_deconv_bf16x3_supported.  weight: Caffe's [Cin][Cout][4][4] blob; the operand holds
// the three bf16 planes of weight^T; col: the column matrix [N][16 Cout][Hin Win] fn2_col2im_bias_relu_forward_into reads.
size_t deconv_bf16x3_packed_floats(int Cin, int Cout);
int deconv_bf16x3_pack_weights(const float* weight, float* packed, int Cin, int Cout, void* stream);
int deconv_bf16x3_gemm(const float* bottom, const float* packed_weight, float* col, int N, int Cin, int Hin, int Win, int bottom_channels,
                       int bottom_c0, int Cout, void* stream);

// csrc/tconv_bf16x3.hip: the data gradient of a Convolution{5, 2, 2} in split-bf16 arithmetic (FN2_CONV_ARITH_BF16X3 beside
// FN2_BWD_ROUTE_TCONV); which layers it takes: fn2_tconv_bf16x3_supported.  weight: the Convolution's own blob [Ct][Cb][k][k] (Ct = top_diff
// channels, Cb = bottom_diff channels); the operand holds its three bf16 planes in k-step order.  mask: NULL, or the activated output of the
// layer in front (bottom_diff is multiplied by its leaky-ReLU derivative on the way out).
size_t tconv_bf16x3_packed_floats(int Cb, int Ct, int kernel, int pad);
int tconv_bf16x3_pack_weights(const float* weight, float* packed, int Cb, int Ct, int kernel, int pad, void* stream);
int tconv_bf16x3_masked(const float* top_diff, const float* packed_weight, float* bottom_diff, int N, int Ct, int Ht, int Wt, int top_channels, int top_c0,
                        int Cb, int Hb, int Wb, int bottom_channels, int bottom_c0, int kernel, int pad,
                        const float* mask, int mask_channels, int mask_c0, float mask_slope, void* stream);

// csrc/conv_wgrad.hip: the finalize pass of the weight-gradient kernels (wgrad_finalize / wgrad_finalize_tiled) over a slab of `ksplit` parts of
// `slab_part` floats in the tile layout `map` (conv_wgrad_geom.hpp): the parts added in part order, scattered into dw [Ca][Cb][T]
int wgrad_finalize_parts(const float* slab, float* dw, const wg::SlabMap& map, int Ca, int Cb, int nblk_a, int nblk_b, int ksplit, long long slab_part,
                         int accumulate, void* stream);

// csrc/conv_wgrad_bf16x3.hip: the weight gradient of a Convolution{5, 2, 2} in split-bf16 arithmetic (FN2_CONV_ARITH_BF16X3 of
// fn2_conv_backward_weights_arith); which layers it takes: fn2_conv_wgrad_bf16x3_supported (0 bytes: not this layer).  Arguments as
// fn2_conv_backward_weights.
size_t conv_wgrad_bf16x3_workspace_bytes(const fn2_conv_desc* desc, int transposed);
int conv_wgrad_bf16x3(const fn2_conv_desc* desc, int transposed, const float* bottom, int bottom_channels, int bottom_c0, const float* top_diff,
                      int top_channels, int top_c0, float* weight_diff, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

}  // namespace fn2
