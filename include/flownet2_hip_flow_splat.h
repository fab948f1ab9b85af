/* Forward warping ("splatting", csrc/flow_splat.hip): every source pixel of a map is carried along its flow and its value is spread over
 * the four cells around the point where it lands -- summation, average, linear and softmax splatting of Niklaus and Liu, "Softmax
 * Splatting for Video Frame Interpolation" (CVPR 2020).  A header of its own, includable on its own.  A library call with a gradient, not
 * a Caffe layer: the reference tree has no counterpart.  With importance NONE, normalize 0 and t = 1 the forward is the image gradient of
 * FlowWarp (fn2_flow_warp_backward), whose arithmetic it repeats; its `weight` plane is then the range map of Wang et al., "Occlusion
 * Aware Unsupervised Learning of Optical Flow" (CVPR 2018).
 *
 * Inputs, contiguous float, 4-byte alignment: values [N,C,H,W] what is carried; flow [N,2,H,W] (u plane, then v plane); metric [N,1,H,W]
 * z, the importance (NULL allowed with importance NONE only, where it is never read); src_valid [N,1,H,W], non-zero (NaN included: it
 * compares unequal to 0): the source takes part, NULL = all ones, bit for bit.  t: a source moves by t * flow.  results and the workspace
 * hold doubles and ints (8-byte alignment).
 *
 * Arithmetic per source pixel s = (x, y), fp32, every operation rounded on its own (no contraction) except the one fmaf named below,
 * division correctly rounded.
 * ok(a) means |a| <= 1e9, false for NaN and +-Inf.
 *   1. src_valid[s] == 0: status MASKED, the source does nothing.
 *   2. (u, v) = flow[s].  !ok(u) || !ok(v): status NONFINITE.
 *   3. e: NONE e = 1 (metric is not read); LINEAR e = z, NONFINITE where !ok(z) or z < 0; SOFTMAX e = expf(z), NONFINITE where !ok(z) or
 *      e is +Inf.
 *   4. x2 = float(x) + t*u, y2 = float(y) + t*v.
 *   5. inside: x2 >= 0 && y2 >= 0 && x2 < W && y2 < H (FlowWarp's rule); otherwise status OUTSIDE.
 *   6. status SPLATTED.  ixL = (int)x2, ixR = min(ixL + 1, W - 1), iyT = (int)y2, iyB = min(iyT + 1, H - 1), al = x2 - ixL, be = y2 - iyT;
 *      the taps TL, TR, BL, BR are the cells (iyT,ixL), (iyT,ixR), (iyB,ixL), (iyB,ixR) with the weights (1-al)*(1-be), al*(1-be),
 *      (1-al)*be, al*be.
 * No tap index is formed before these tests have passed, so nothing outside the sample's own planes is ever addressed.
 *
 * Per target cell p, over the SPLATTED sources that reach it, in ASCENDING SOURCE INDEX (y * W + x), num_c = den = 0.0f at the start:
 *   w  = the sum, from 0.0f, of the source's tap weights whose cell is p, in the order TL, TR, BL, BR;
 *   ws = w for NONE, w * e otherwise;
 *   num_c = fmaf(values_c(s), ws, num_c) -- ONE rounding: fn2_flow_warp_backward's gather is compiled with contraction and adds its
 *   products this way, and NONE with t = 1 repeats it bit for bit;  den += ws;
 *   and, where more than one tap of the source is p and one of those has weight 0 (a clamped tap on the last column / row):
 *   num_c = fmaf(values_c(s), 0.0f, num_c) (FlowWarp's backward adds that tap as a product of its own: an infinite value makes the cell
 *   NaN).
 *
 * Outputs, each optional (NULL = absent); asking for one changes no bit of another:
 *   out     float [N,C,H,W]: num where normalize == 0; otherwise num / den where den > 0 and the fill value elsewhere (FN2_FILL_ZERO: 0,
 *           FN2_FILL_NAN: the NaN of FlowWarp)
 *   weight  float [N,1,H,W]: den
 *   hole    float [N,1,H,W]: 1.0 where den == 0, else 0.0
 *   status  unsigned char [N,1,H,W]: FN2_FLOW_SPLAT_STATUS_* of every source
 * results: DEVICE double [(N + 1) * FN2_FLOW_SPLAT_K]: one row per sample, then a totals row (sums in sample order from 0, max for
 * WEIGHT_MAX); columns as the first enum below; counts are exact integers held in doubles.
 *   PIXELS H W;  MASKED, NONFINITE, OUTSIDE, SPLATTED: sources with that status;  HOLES: cells where den == 0;
 *   WEIGHT_SUM, WEIGHT_MAX: fp64 sum and the largest of the fp32 den over the cells where it is not NaN (0 if none).
 *
 * Order.  The sum at a cell is a function of the sample's own (values, flow, metric, src_valid, t) alone: not of the batch, the run, the
 * alignment of a pointer or of how the atomics of the link pass were served, for ANY number of sources on a cell.  Three launches and a
 * memset: (1) link: a thread per source writes its status and, where SPLATTED, hangs itself on the list of its top-left tap's cell -- one
 * integer atomic exchange, the only atomic; (2) gather: a thread per (cell, group of up to 8 channels) walks the lists of its own cell and
 * of the cells left, above and above-left.  Up to 16 candidates are sorted in LDS and added in ascending order; where there are more the
 * thread makes selection passes over the lists instead: each pass takes the smallest index greater than the last one taken -- the same
 * ascending order, quadratic only at such sinks.  The row sums are kept by channel group 0: a sample is cut into B =
 * min(ceil(H W / 1024), 128) workgroups of 256 threads, thread i of workgroup b takes the cells b * 256 + i, then every B * 256 further
 * on, in ascending order; a wave64 shuffle tree and the four waves in order give the workgroup's partial row; (3) the shared
 * one-workgroup finalise adds a sample's B partial rows in index order.  All of it is fixed by (H, W) alone.  No floating-point atomics,
 * no host readback.
 *
 * Backward: ONE gather launch, a thread per source pixel, scattering nothing.  Inputs: out_diff [N,C,H,W] (g), weight_diff [N,1,H,W] or
 * NULL, the forward's inputs, and the forward's saved `out` (read where normalize == 1 only; may be NULL otherwise) and `weight` (den).
 * Per tap cell p:  normalize == 1: gn_c(p) = g_c(p) / den(p) where den(p) > 0, else 0;  gd(p) = -(sum_c g_c(p) * out_c(p)) / den(p)
 * where den(p) > 0, else 0, the sum over c ascending from 0.0f;  normalize == 0: gn = g, gd = 0;  then gd += weight_diff(p) where given.
 * Per SPLATTED source, taps k in the order TL, TR, BL, BR, channels c ascending, every sum from 0.0f:
 *   A_k       = (sum_c gn_c(p_k) * values_c(s)) + gd(p_k)
 *   dvalues_c = e * (sum_k w_k * gn_c(p_k))
 *   de        = sum_k w_k * A_k;   dmetric = de for LINEAR, de * e for SOFTMAX (0 for NONE)
 *   dx2       = e * (sum_k A_k * dwx_k),  dwx = -(1-be), (1-be), -be, be;   dy2 = e * (sum_k A_k * dwy_k),  dwy = -(1-al), -al, (1-al), al
 *   du = t * dx2, dv = t * dy2
 * Clamped taps that coincide cancel in dx2 / dy2 as they do in the forward.  A source that is not SPLATTED gets zeros.  For NONE e = 1 and
 * the products by e are not formed.  Outputs values_diff [N,C,H,W], flow_diff [N,2,H,W], metric_diff [N,1,H,W], each optional.
 *
 * fn2_flow_splat_sizes is host-only: the workspace bytes for (N, H, W) and K.  _forward and _backward return FN2_OK or refuse on the host
 * before any launch, writing nothing: FN2_ERR_INVALID_ARG a NULL values, flow or results (backward: values, flow, out_diff, weight; out
 * with normalize 1; metric_diff asked for with importance NONE), a non-positive extent, a blob of 2^31 elements or more (N max(C,2) H W),
 * a NaN or infinite t, an importance, normalize or fill that is not one of the values named, metric == NULL with an importance other than
 * NONE; FN2_ERR_WORKSPACE a workspace that is NULL or too small.  _sizes refuses the same extents and then writes nothing. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
enum {
  FN2_FLOW_SPLAT_PIXELS = 0,
  FN2_FLOW_SPLAT_MASKED,
  FN2_FLOW_SPLAT_NONFINITE,
  FN2_FLOW_SPLAT_OUTSIDE,
  FN2_FLOW_SPLAT_SPLATTED,
  FN2_FLOW_SPLAT_HOLES,
  FN2_FLOW_SPLAT_WEIGHT_SUM,
  FN2_FLOW_SPLAT_WEIGHT_MAX,
  FN2_FLOW_SPLAT_K
};
enum {
  FN2_FLOW_SPLAT_IMPORTANCE_NONE = 0,
  FN2_FLOW_SPLAT_IMPORTANCE_LINEAR,
  FN2_FLOW_SPLAT_IMPORTANCE_SOFTMAX
};
enum {
  FN2_FLOW_SPLAT_STATUS_MASKED = 0,
  FN2_FLOW_SPLAT_STATUS_NONFINITE,
  FN2_FLOW_SPLAT_STATUS_OUTSIDE,
  FN2_FLOW_SPLAT_STATUS_SPLATTED
};
/* either out-pointer may be NULL */
int fn2_flow_splat_sizes(int N, int C, int H, int W, size_t* workspace_bytes, int* K);
/* metric, src_valid, out, weight, hole, status: NULL = absent; results: DEVICE double [(N + 1) * FN2_FLOW_SPLAT_K] */
int fn2_flow_splat_forward(const float* values, const float* flow, const float* metric, const float* src_valid, int N, int C, int H, int W,
                           float t, int importance, int normalize, int fill, double* results, float* out, float* weight, float* hole,
                           unsigned char* status, void* workspace, size_t workspace_bytes, void* stream);
/* out, weight: the forward's; weight_diff, metric, src_valid, values_diff, flow_diff, metric_diff: NULL = absent */
int fn2_flow_splat_backward(const float* out_diff, const float* weight_diff, const float* values, const float* flow, const float* metric,
                            const float* src_valid, const float* out, const float* weight, int N, int C, int H, int W, float t,
                            int importance, int normalize, float* values_diff, float* flow_diff, float* metric_diff, void* stream);
#ifdef __cplusplus
}
#endif
