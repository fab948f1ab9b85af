/* General-geometry Convolution / Deconvolution (csrc/conv_general.hip): the last resort for every geometry fn2_conv_desc can state and the
 * specialised families (fn2_conv_route, fn2_deconv_route, fn2_conv_backward_data_route, fn2_conv_backward_weights_supported) do not take.
 * A header of its own, includable on its own; it adds no structure, enumerator or constant.
 *
 *   replaces  ConvolutionLayer / DeconvolutionLayer::{Forward_gpu, Backward_gpu}   conv_layer.cu:8-57, deconv_layer.cu:8-56
 *             BaseConvolutionLayer::{forward,backward,weight}_gpu_gemm, *_gpu_bias base_conv_layer.cpp:255-393 (im2col + GEMM per sample)
 *             output extents                                                        conv_layer.cpp:8-23, deconv_layer.cpp:8-24
 *
 * Scope: N, Cin, Cout, kernel, stride >= 1, pad >= 0, square taps, no dilation, no groups; `transposed` = 0 a Convolution (weight blob
 * [Cout][Cin][k][k], top extent (Hin + 2 pad - kernel) / stride + 1, which needs Hin + 2 pad >= kernel), 1 a Deconvolution (weight blob
 * [Cin][Cout][k][k] as Caffe stores it, top extent stride (Hin - 1) + kernel - 2 pad >= 1).  Every blob (bottom, top, weights, packed
 * operand) below 2^31 elements.  Pointers need 4-byte alignment only; channel slices of wider blobs on both sides, of any plane size.
 *
 * Two gather kernels on v_mfma_f32_16x16x4_f32 (exact fp32 products, one fp32 accumulation per output value in ascending k order), both an
 * implicit GEMM out[M x pixels] = Wp[M x K] x col[K x pixels] whose col tile (16 k-rows x 64 pixels of one sample) is gathered into LDS
 * straight from the input blob, zeros outside the image; no column buffer, no workspace:
 *   forward gather     col[(c, ky, kx)][(y, x)] = in[c][y stride - pad + ky][x stride - pad + kx]
 *                      -> Convolution forward (K = Cin k k), Deconvolution data gradient (K = Cout k k)
 *   transposed gather  col[(c, ky, kx)][(y, x)] = in[c][(y + pad - ky) / stride][(x + pad - kx) / stride] where both divisions are exact
 *                      -> Convolution data gradient (K = Cout k k), Deconvolution forward (K = Cin k k)
 * The packed operand Wp (fn2_conv_general_pack_weights, once per weight version and pass): [ceil(M / 16)][Kpad / 4][64 lanes], lane l of
 * k-step ks of group g holding Wp[16 g + (l & 15)][4 ks + (l >> 4)], zero beyond M and K, Kpad = K rounded up to 16 (whole chunks of four
 * k-steps): neither the K loop nor the M direction has a tail; the pixel tail is masked at the store.  pass 0 = forward, 1 = data
 * gradient, 2 = weight gradient (no operand: 0 floats, packing is a no-op).
 * Weight gradient: dW[A x K] = X[A x P] x col^T[P x K] with the forward gather of the larger map, tiles of 64 channels x 16 k-columns,
 * the N x ceil(P / 64) pixel chunks cut into a number of parts fixed by the descriptor alone; each part is one accumulation chain per
 * value into the workspace, a second kernel adds the parts in part order (and into weight_diff when accumulate != 0).  Bias gradient: one
 * workgroup per channel, a fixed strided sum and tree.  No floating-point atomics anywhere.
 * Bits: the same from run to run, and for forward / data gradient the same for a sample whatever its batch (a tile never spans samples,
 * nothing depends on N).  The gather kernels come in three instantiations -- 1, 2 or 4 groups of 16 output channels per workgroup, chosen by
 * the channel count alone (up to 16, up to 32, more), no autotuning -- that run the same accumulation chain per value, so the same bits
 * (fn2_debug_set_conv_general_groups forces one: 0 = by geometry, 1, 2, 4; the weight gradient has one form).  fn2_set_batch_invariant
 * does not reach this family; the split-bf16 switches do not either.
 *
 * _supported and _sizes are host-only (no GPU needed).  _supported: 1 / 0.  The other functions return FN2_OK or refuse on the host
 * before any launch: FN2_ERR_UNSUPPORTED what _supported refuses, FN2_ERR_INVALID_ARG a null blob, a channel slice outside its blob, a
 * misaligned pointer or an unknown pass, FN2_ERR_WORKSPACE a workspace that is null or too small. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
int fn2_conv_general_supported(const fn2_conv_desc* desc, int transposed);
int fn2_debug_set_conv_general_groups(int groups);
/* floats of the packed operand of each pass and bytes of the weight-gradient workspace; any out-pointer may be NULL */
int fn2_conv_general_sizes(const fn2_conv_desc* desc, int transposed, size_t* forward_packed, size_t* backward_data_packed,
                           size_t* backward_weights_packed, size_t* backward_weights_workspace);
int fn2_conv_general_pack_weights(const fn2_conv_desc* desc, int transposed, int pass, const float* weight, float* packed, void* stream);
/* top = act(bias + layer(bottom)); bias may be NULL; relu != 0: leaky ReLU with negative_slope */
int fn2_conv_general_forward(const fn2_conv_desc* desc, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                             const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                             int relu, float negative_slope, void* stream);
/* bottom_diff is OVERWRITTEN (exactly Cin channels from bottom_c0 on) */
int fn2_conv_general_backward_data(const fn2_conv_desc* desc, int transposed, const float* top_diff, int top_channels, int top_c0,
                                   const float* packed_weight, float* bottom_diff, int bottom_channels, int bottom_c0, void* stream);
/* weight_diff in the layer's own blob layout; bias_diff [Cout] or NULL; accumulate != 0 adds into both (Caffe's beta = 1) */
int fn2_conv_general_backward_weights(const fn2_conv_desc* desc, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                      const float* top_diff, int top_channels, int top_c0, float* weight_diff, float* bias_diff,
                                      int accumulate, void* workspace, size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
