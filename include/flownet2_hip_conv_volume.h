/* General-geometry Convolution / Deconvolution over 0, 1, 2 or 3 spatial axes: the kernels of include/flownet2_hip_conv_geometry.h
 * (csrc/conv_general.hip) with a depth axis in front of the two.  A header of its own, includable on its own; it adds no structure,
 * enumerator or constant.
 *
 *   replaces  BaseConvolutionLayer::LayerSetUp / Reshape with num_spatial_axes_ != 2 (axis, force_nd_im2col)   base_conv_layer.cpp:15-254
 *             im2col_nd_gpu / col2im_nd_gpu                                                                     util/im2col.cu
 *             ConvolutionLayer / DeconvolutionLayer::compute_output_shape, Forward_gpu, Backward_gpu           as in flownet2_hip_conv_geometry.h
 *
 * The geometry travels as one array of 19 ints, `geom`:
 *   {N, Cin, Din, Hin, Win, Cout, kernel_d, kernel_h, kernel_w, stride_d, stride_h, stride_w, pad_d, pad_h, pad_w,
 *    dilation_d, dilation_h, dilation_w, group}
 * N is the folded batch: count(0, channel_axis) of the bottom blob, whatever its leading axes.  Fewer than three spatial axes are stated
 * with the leading ones trivial (extent 1, kernel 1, stride 1, pad 0, dilation 1): one axis [N, C, L] is Din = Hin = 1, Win = L; none is a
 * 1x1x1 layer on a 1x1x1 map.  A geometry whose depth axis is trivial runs the very kernels fn2_conv_geometry_* run on the other fourteen
 * ints and gives their bits; only a depth axis that is not trivial runs the depth instantiations.  Four or more spatial axes cannot be
 * stated and are refused by the callers (the Caffe plug-in and flownet2_amd.ops.conv_volume) by name.
 * Scope, per axis, as in flownet2_hip_conv_geometry.h: N, Cin, Cout, extents, kernel, stride, dilation, group >= 1, pad >= 0, Cin % group ==
 * 0 and Cout % group == 0; ext = dilation (kernel - 1) + 1; `transposed` = 0 a Convolution (weight blob [Cout][Cin / group][kd][kh][kw], top
 * extent (in + 2 pad - ext) / stride + 1), 1 a Deconvolution (weight blob [Cin][Cout / group][kd][kh][kw], top extent stride (in - 1) + ext
 * - 2 pad >= 1).  Every blob (bottom, top, weights, packed operand) below 2^31 elements, the padded extents below 2^31.  Channel slices of
 * wider blobs on both sides, groups as there.  The gathers, per axis, with pixels (z, y, x) and k-rows (c, kz, ky, kx), the taps fastest,
 * kz before ky before kx:
 *   forward gather     col[(c, kz, ky, kx)][(z, y, x)] = in[c][z stride_d - pad_d + kz dilation_d][y ...][x ...]
 *   transposed gather  col[(c, kz, ky, kx)][(z, y, x)] = in[c][(z + pad_d - kz dilation_d) / stride_d][...][...]
 *                      where all three divisions are exact and inside the volume
 * A tap outside the volume contributes 0 and is not read.  The packed operand: [group][ceil(Mg / 16)][Kpad_g / 4][64 lanes] with K_g =
 * (reduction channels per group) kd kh kw, laid out as in flownet2_hip_conv_geometry.h.  Weight gradient: the same plan (at most 64
 * parts, a function of the geometry alone, an ordered finalize pass, no floating-point atomics) over N Dt Ht Wt pixels; the workspace is
 * [parts][group][16 ceil(Csg / 16)][Kpad_g] floats.  Bits: one fp32 accumulation chain per output value in ascending k; the same from run
 * to run, for a sample whatever its batch, and from the 1-, 2- and 4-row-group instantiations (fn2_debug_set_conv_general_groups).
 *
 * _supported, _out_shape and _sizes are host-only (no GPU needed).  _supported: 1 / 0.  The other functions return FN2_OK or refuse on the
 * host before any launch, with the codes of flownet2_hip_conv_geometry.h: FN2_ERR_UNSUPPORTED what _supported refuses (a null geom, a
 * value out of range, a channel count not divisible by group, an empty output, a blob beyond the 32-bit limits), FN2_ERR_INVALID_ARG a
 * null blob, a channel slice outside its blob, a misaligned pointer or an unknown pass, FN2_ERR_WORKSPACE a workspace that is null or too
 * small.  After `geom` the argument lists are those of fn2_conv_geometry_*. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
int fn2_conv_volume_supported(const int* geom, int transposed);
/* the top extents; any out-pointer may be NULL */
int fn2_conv_volume_out_shape(const int* geom, int transposed, int* out_d, int* out_h, int* out_w);
/* floats of the packed operand of each pass and bytes of the weight-gradient workspace; any out-pointer may be NULL */
int fn2_conv_volume_sizes(const int* geom, int transposed, size_t* forward_packed, size_t* backward_data_packed,
                          size_t* backward_weights_packed, size_t* backward_weights_workspace);
int fn2_conv_volume_pack_weights(const int* geom, int transposed, int pass, const float* weight, float* packed, void* stream);
/* top = act(bias + layer(bottom)); bias may be NULL; relu != 0: leaky ReLU with negative_slope */
int fn2_conv_volume_forward(const int* geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                            const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                            int relu, float negative_slope, void* stream);
/* bottom_diff is OVERWRITTEN (exactly Cin channels from bottom_c0 on) */
int fn2_conv_volume_backward_data(const int* geom, int transposed, const float* top_diff, int top_channels, int top_c0,
                                  const float* packed_weight, float* bottom_diff, int bottom_channels, int bottom_c0, void* stream);
/* weight_diff in the layer's own blob layout; bias_diff [Cout] or NULL; accumulate != 0 adds into both */
int fn2_conv_volume_backward_weights(const int* geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                     const float* top_diff, int top_channels, int top_c0, float* weight_diff, float* bias_diff,
                                     int accumulate, void* workspace, size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
