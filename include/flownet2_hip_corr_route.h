/* Correlation: route query and routed forward (csrc/correlation.hip).  Part of include/flownet2_hip.h, which includes this file after
 * fn2_corr_params and the FN2_ROUTE_* / FN2_CONV_ARITH_* enums; do not include it on its own.  The convention is the convolutions': the
 * arithmetic (FN2_CONV_ARITH_BF16X3) is a bit beside the route, not a route of its own; the comment above the include describes both. */
#ifndef FLOWNET2_HIP_CORR_ROUTE_H_
#define FLOWNET2_HIP_CORR_ROUTE_H_
enum { FN2_CORR_ROUTE_NONE = 0, FN2_CORR_ROUTE_OWN = 1 };
/* NONE for parameters fn2_correlation_out_shape refuses; OWN | FN2_CONV_ARITH_BF16X3 when flags & FN2_ROUTE_BF16X3 and
 * fn2_correlation_bf16x3_supported; OWN otherwise.  Independent of N beyond the supported check and of batch-invariant mode. */
int fn2_correlation_route(const fn2_corr_params* p, int N, int C, int H, int W, int flags);
/* route OWN: exactly fn2_correlation_forward_fused.  OWN | FN2_CONV_ARITH_BF16X3: the split-bf16 kernel, FN2_ERR_UNSUPPORTED where it does not
 * take the layer or a blob is not 16-byte aligned.  Any other route: FN2_ERR_INVALID_ARG.  NULL blobs and a slice outside the top blob are
 * refused on the host with nothing launched; N == 0 is FN2_OK. */
int fn2_correlation_forward_routed(const fn2_corr_params* p, int route,
                                   const float* bottom0, const float* bottom1, float* top,
                                   int N, int C, int H, int W, int top_channels, int top_c0, int relu, float negative_slope,
                                   void* workspace, size_t workspace_bytes, void* stream);
#endif
