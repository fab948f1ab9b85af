/* The flow heads of a refinement stage with one launch less (csrc/flow_head.hip).  A header of its own, includable on its own.
 *
 * predict_flow (Convolution{3, 1, 1} C -> 2) and the upsample_flow (Deconvolution{4, 2, 1} 2 -> 2) that reads it, for a forward without
 * autograd: the per-tap pass of fn2_predict_flow_conv_forward as it is (same splits, same workspace), then ONE launch whose blocks gather
 * a tile of the flow (and a border of one pixel) into LDS and up-sample it from there into channels [top_c0, top_c0 + 2) of
 * top [N, top_channels, 2H, 2W] -- instead of a gather launch and an up-sampling launch with the flow's trip through memory between them.
 * flow [N, 2, H, W] and the slice have the bits of fn2_predict_flow_conv_forward followed by fn2_upsample_flow_deconv_forward_into
 * (flownet2_hip.h): the same expressions in the same order.  No other channel of top is written.  bias / up_bias may be NULL.
 *   in [N, C, H, W], weight [2, C, 3, 3], bias [2]; up_weight [2, 2, 4, 4], up_bias [2]
 *   workspace: fn2_predict_flow_conv_workspace_bytes(N, C, H, W)
 * fn2_predict_upsample_flow_supported: 0 for a geometry this form declines; the caller then makes the two calls. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
int fn2_predict_upsample_flow_supported(int N, int C, int H, int W);
int fn2_predict_upsample_flow_forward_into(const float* in, const float* weight, const float* bias, float* flow,
                                           const float* up_weight, const float* up_bias, float* top,
                                           int N, int C, int H, int W, int top_channels, int top_c0,
                                           void* workspace, size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
