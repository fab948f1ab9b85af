/* Forward-backward flow consistency (csrc/flow_consistency.hip): the occlusion masks of a pair of flows, both directions in one launch.
 * A header of its own, includable on its own.  A library call, not a Caffe layer, and not differentiable: the reference tree has no
 * counterpart.  The thresholds are those of Sundaram, Brox and Keutzer, "Dense point trajectories by GPU-accelerated large displacement
 * optical flow" (ECCV 2010): a pixel is occluded where the flow there and the other flow at its target do not cancel, and is not trusted
 * on a motion boundary.
 *
 * Inputs: fw, bw contiguous float [N,2,H,W] (u plane, then v plane); fw maps frame 0 to frame 1, bw frame 1 to frame 0.  The float
 * pointers need 4-byte alignment only; results and the workspace hold doubles (8-byte alignment).
 * Direction 0 checks a = fw against o = bw, direction 1 checks a = bw against o = fw.
 *
 * Arithmetic per pixel (x, y), fp32, every operation rounded on its own (no contraction).  ok(t) means |t| <= 1e9, which is false for NaN
 * and +-Inf (1e9: the .flo unknown-flow convention, as in flownet2_hip_flow_metrics.h); "not finite" below means !ok.
 *   1. (au, av) = a[y, x].  !ok(au) || !ok(av): flag NONFINITE, err = NaN, and nothing else is computed for the pixel (no conversion to
 *      int, no tap address).
 *   2. motion boundary: ux = 0.5f * (u[y, min(x+1, W-1)] - u[y, max(x-1, 0)]), uy likewise along y, vx, vy likewise on the v plane;
 *      g = ((ux*ux + uy*uy) + vx*vx) + vy*vy; flag BOUNDARY when g > beta1 * (au*au + av*av) + beta2.  Where one of the eight neighbour
 *      values is not finite there is no BOUNDARY flag.
 *   3. x2 = float(x) + au, y2 = float(y) + av; inside: x2 >= 0 && y2 >= 0 && x2 < W && y2 < H (FlowWarp's rule).  Otherwise flag OUTSIDE,
 *      err = NaN, stop.
 *   4. ixL = (int)x2, ixR = min(ixL + 1, W - 1), iyT = (int)y2, iyB = min(iyT + 1, H - 1), al = x2 - ixL, be = y2 - iyT  (FlowWarp's taps).
 *   5. per channel of o, with TL = o[iyT, ixL], TR = o[iyT, ixR], BL = o[iyB, ixL], BR = o[iyB, ixR]:
 *      b = ((((1-al)*(1-be))*TL + (al*(1-be))*TR) + ((1-al)*be)*BL) + (al*be)*BR.  !ok(bu) || !ok(bv): flag NONFINITE, err = NaN, stop.
 *   6. su = au + bu, sv = av + bv, s = su*su + sv*sv, m = (au*au + av*av) + (bu*bu + bv*bv);
 *      flag INCONSISTENT when s > alpha1 * m + alpha2; err = sqrtf(s).
 * The published constants are alpha = (0.01, 0.5), beta = (0.01, 0.002).
 * No tap index is formed before the inside test and the finite test have passed, and every one is clamped as in 4: nothing outside
 * [0,W) x [0,H) of the pixel's own sample is ever read, whatever the flows hold.
 *
 * Outputs per direction, each optional (NULL = absent); asking for one changes no bit of another:
 *   flags   unsigned char [N,1,H,W]: the bit set of FN2_FLOW_CONSISTENCY_FLAG_*
 *   occ     float [N,1,H,W]: 1.0 where OUTSIDE, INCONSISTENT or NONFINITE is set, else 0.0 -- the `occ` plane of fn2_flow_metrics; its
 *           complement is a `valid` plane
 *   err     float [N,1,H,W]
 *   warped  float [N,2,H,W]: (bu, bv) of step 5, NaN where the pixel stopped before step 5 -- o warped by a, as
 *           fn2_flow_warp_forward(o, a, FN2_FILL_NAN) computes it in another association
 *
 * results: DEVICE double [2][(N + 1) * FN2_FLOW_CONSISTENCY_K]: per direction one row per sample, then a totals row; columns as the first
 * enum below.  Counts are exact integers held in doubles.
 *   PIXELS                                  H W
 *   NONFINITE, OUTSIDE, INCONSISTENT, BOUNDARY   pixels that carry the flag
 *   OCCLUDED                                pixels where occ is 1.0
 *   ERR_SUM, ERR_MAX                        fp64 sum of the fp32 err over the pixels where it is not NaN; the largest such err (0 if none)
 * The totals row is the fp64 sum of the sample rows in sample order (starting from 0), the max for ERR_MAX.
 *
 * Order of the sums: fixed by (H, W) alone.  A (direction, sample) is cut into B = min(ceil(H W / 1024), 128) workgroups of 256 threads;
 * where W is a multiple of 4 a thread owns four neighbouring pixels of a row per step (16-byte loads and stores where every pointer given
 * is 16-byte aligned, 4-byte ones otherwise: same values, same order, same bits), one pixel per step otherwise; a thread adds its pixels
 * in ascending order, a wave64 shuffle tree and the four waves in order give the workgroup's partial row in the workspace; one finalise
 * workgroup adds a sample's B partial rows in index order.  So a sample's row has the same bits alone or in any batch, from run to run and
 * for any allocation.  Two launches, no floating-point atomics, no host synchronisation.
 *
 * fn2_flow_consistency_sizes is host-only: the workspace bytes for (N, H, W) and K.  fn2_flow_consistency returns FN2_OK or refuses on the
 * host before any launch, writing nothing: FN2_ERR_INVALID_ARG a NULL fw, bw or results, a non-positive extent, a blob of 2^31 elements
 * or more (N 2 H W), a NaN or negative alpha1, alpha2, beta1 or beta2; FN2_ERR_WORKSPACE a workspace that is NULL or too small.  _sizes
 * refuses the same extents and then writes nothing. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
enum {
  FN2_FLOW_CONSISTENCY_PIXELS = 0,
  FN2_FLOW_CONSISTENCY_NONFINITE,
  FN2_FLOW_CONSISTENCY_OUTSIDE,
  FN2_FLOW_CONSISTENCY_INCONSISTENT,
  FN2_FLOW_CONSISTENCY_OCCLUDED,
  FN2_FLOW_CONSISTENCY_BOUNDARY,
  FN2_FLOW_CONSISTENCY_ERR_SUM,
  FN2_FLOW_CONSISTENCY_ERR_MAX,
  FN2_FLOW_CONSISTENCY_K
};
enum {
  FN2_FLOW_CONSISTENCY_FLAG_NONFINITE = 1,
  FN2_FLOW_CONSISTENCY_FLAG_OUTSIDE = 2,
  FN2_FLOW_CONSISTENCY_FLAG_INCONSISTENT = 4,
  FN2_FLOW_CONSISTENCY_FLAG_BOUNDARY = 8
};
/* either out-pointer may be NULL */
int fn2_flow_consistency_sizes(int N, int H, int W, size_t* workspace_bytes, int* K);
/* flags_*, occ_*, err_*, warped_*: NULL = absent; results: DEVICE double [2][(N + 1) * FN2_FLOW_CONSISTENCY_K] */
int fn2_flow_consistency(const float* fw, const float* bw, int N, int H, int W, float alpha1, float alpha2, float beta1, float beta2,
                         double* results, unsigned char* flags_fw, unsigned char* flags_bw, float* occ_fw, float* occ_bw, float* err_fw,
                         float* err_bw, float* warped_fw, float* warped_bw, void* workspace, size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
