// Entry points shared between translation units of the library that are not part of include/flownet2_hip.h.
#pragma once

#include <cstddef>

namespace fn2 {

// csrc/tconv_mfma.hip: fn2_tconv_forward with the output multiplied by the leaky-ReLU derivative of `mask` (NULL: no mask)
int tconv_forward_masked(const float* bottom, const float* packed_weight, const float* bias, float* top,
                         int N, int Cin, int Hin, int Win, int bottom_channels, int bottom_c0,
                         int Cout, int Hout, int Wout, int top_channels, int top_c0, int kernel, int pad,
                         int relu, float negative_slope, const float* mask, int mask_channels, int mask_c0, float mask_slope, void* stream);

// csrc/conv_stem_wgrad.hip: fn2_conv_k7s2_wgrad; bias_diff != NULL: the bias gradient of the same layer comes out of the same pass
int conv_k7s2_wgrad_bias(const float* top_diff, const float* bottom, float* weight_diff, float* bias_diff, int N, int Cin, int Hin, int Win, int Cout,
                         int accumulate, void* workspace, size_t workspace_bytes, void* stream);

}  // namespace fn2
