/* General-geometry Convolution / Deconvolution with rectangular taps, per-axis stride, pad and dilation, and groups: the kernels of
 * include/flownet2_hip_conv_general.h (csrc/conv_general.hip) widened in place, for every ConvolutionParameter with two spatial axes that
 * fn2_conv_desc cannot state.  A header of its own, includable on its own; it adds no structure, enumerator or constant.
 *
 *   replaces  BaseConvolutionLayer::LayerSetUp (kernel_h / kernel_w, stride, pad, dilation, group)  base_conv_layer.cpp:36-139
 *             ConvolutionLayer / DeconvolutionLayer::compute_output_shape                             conv_layer.cpp:8-23, deconv_layer.cpp:8-24
 *             ConvolutionLayer / DeconvolutionLayer::{Forward_gpu, Backward_gpu}                      conv_layer.cu:8-57, deconv_layer.cu:8-56
 *             the per-group GEMMs of {forward,backward,weight}_gpu_gemm                               base_conv_layer.cpp:255-393
 *
 * The geometry travels as one array of 14 ints, `geom`:
 *   {N, Cin, Hin, Win, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group}
 * Scope: N, Cin, Cout, kernel, stride, dilation, group >= 1, pad >= 0, Cin % group == 0 and Cout % group == 0.  With ext = dilation
 * (kernel - 1) + 1 per axis, `transposed` = 0 is a Convolution (weight blob [Cout][Cin / group][kh][kw], top extent (Hin + 2 pad - ext) /
 * stride + 1, which needs Hin + 2 pad >= ext), 1 a Deconvolution (weight blob [Cin][Cout / group][kh][kw] as Caffe stores it, top extent
 * stride (Hin - 1) + ext - 2 pad >= 1).  Every blob (bottom, top, weights, packed operand) below 2^31 elements, the padded extents
 * below 2^31.  Pointers need 4-byte alignment only; channel slices of wider blobs on both sides, of any plane size: the group offsets are
 * added to the caller's bottom_c0 / top_c0.
 *
 * Group g of `group` is the layer of Cin / group -> Cout / group channels on the channel slices [g Cin / group, ...) of bottom and
 * [g Cout / group, ...) of top with the rows [g Cs / group, ...) of the weight blob [Cs][Cl / group][kh][kw] (Cs: Cout of a Convolution,
 * Cin of a Deconvolution).  It is a grid factor of the kernels; a row group of 16 output channels and a 64-channel tile of the weight
 * gradient never span two groups.  The gathers, per axis:
 *   forward gather     col[(c, ky, kx)][(y, x)] = in[c][y stride_h - pad_h + ky dilation_h][x stride_w - pad_w + kx dilation_w]
 *   transposed gather  col[(c, ky, kx)][(y, x)] = in[c][(y + pad_h - ky dilation_h) / stride_h][(x + pad_w - kx dilation_w) / stride_w]
 *                      where both divisions are exact and inside the map
 * The packed operand (fn2_conv_geometry_pack_weights): [group][ceil(Mg / 16)][Kpad_g / 4][64 lanes], Mg the pass's output channels per
 * group, K_g = (reduction channels per group) kh kw with the taps fastest, ky before kx, Kpad_g = K_g rounded up to 16; lane l of k-step ks
 * of row group r holds Wp[16 r + (l & 15)][4 ks + (l >> 4)], zero beyond Mg and K_g.  With group 1 and square taps this is byte for byte
 * the operand of fn2_conv_general_pack_weights.  pass 0 = forward, 1 = data gradient, 2 = weight gradient (no operand).
 * Weight gradient: as in flownet2_hip_conv_general.h per group (the plan -- at most 64 parts -- is a function of the geometry alone, an
 * ordered finalize pass, no floating-point atomics); the workspace is [parts][group][16 ceil(Csg / 16)][Kpad_g] floats.  The bias gradient
 * is per channel.
 * Bits: one fp32 accumulation chain per output value in ascending k; the same from run to run, for a sample whatever its batch, and from
 * the 1-, 2- and 4-row-group instantiations (fn2_debug_set_conv_general_groups).  A geometry fn2_conv_desc can state -- (k, k, s, s, p, p,
 * 1, 1, 1) -- runs the very kernels fn2_conv_general_* run and gives their bits; every other geometry runs instantiations that read the
 * per-axis values.  fn2_set_batch_invariant and the split-bf16 switches do not reach this family.
 *
 * _supported, _out_shape and _sizes are host-only (no GPU needed).  _supported: 1 / 0.  The other functions return FN2_OK or refuse on the
 * host before any launch: FN2_ERR_UNSUPPORTED what _supported refuses (a null geom, a value out of range, group < 1, dilation < 1, a
 * channel count not divisible by group, an empty output, a blob beyond the 32-bit limits), FN2_ERR_INVALID_ARG a null blob, a channel
 * slice outside its blob, a misaligned pointer or an unknown pass, FN2_ERR_WORKSPACE a workspace that is null or too small. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
int fn2_conv_geometry_supported(const int* geom, int transposed);
/* the top extent (conv_layer.cpp:8-23, deconv_layer.cpp:8-24 with the dilated extent); either out-pointer may be NULL */
int fn2_conv_geometry_out_shape(const int* geom, int transposed, int* out_h, int* out_w);
/* floats of the packed operand of each pass and bytes of the weight-gradient workspace; any out-pointer may be NULL */
int fn2_conv_geometry_sizes(const int* geom, int transposed, size_t* forward_packed, size_t* backward_data_packed,
                            size_t* backward_weights_packed, size_t* backward_weights_workspace);
int fn2_conv_geometry_pack_weights(const int* geom, int transposed, int pass, const float* weight, float* packed, void* stream);
/* top = act(bias + layer(bottom)); bias may be NULL; relu != 0: leaky ReLU with negative_slope   (forward_gpu_gemm + forward_gpu_bias) */
int fn2_conv_geometry_forward(const int* geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                              const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                              int relu, float negative_slope, void* stream);
/* bottom_diff is OVERWRITTEN (exactly Cin channels from bottom_c0 on)   (backward_gpu_gemm) */
int fn2_conv_geometry_backward_data(const int* geom, int transposed, const float* top_diff, int top_channels, int top_c0,
                                    const float* packed_weight, float* bottom_diff, int bottom_channels, int bottom_c0, void* stream);
/* weight_diff in the layer's own blob layout; bias_diff [Cout] or NULL; accumulate != 0 adds into both   (weight_gpu_gemm, backward_gpu_bias) */
int fn2_conv_geometry_backward_weights(const int* geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                       const float* top_diff, int top_channels, int top_c0, float* weight_diff, float* bias_diff,
                                       int accumulate, void* workspace, size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
