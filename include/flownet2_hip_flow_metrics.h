/* Flow error metrics (csrc/flow_metrics.hip): what a FlowNet user quotes -- end-point error, KITTI's Fl outliers, Sintel's speed bands and
 * matched / unmatched split, Middlebury's angular error -- of a prediction against ground truth, in one streaming pass.
 * A header of its own, includable on its own.  A library call, not a Caffe layer: the reference tree has no counterpart (its numbers come
 * from the L1Loss test nets, which add sqrt(eps) at masked pixels and carry the loss weights).
 *
 * Inputs: pred, gt contiguous float [N,2,H,W] (u plane, then v plane); valid (optional, NULL = absent) float [N,1,H,W], non-zero = use the
 * pixel; occ (optional) float [N,1,H,W], non-zero = occluded / unmatched.  The float pointers need 4-byte alignment only; results and the
 * workspace hold doubles (8-byte alignment).
 *
 * Arithmetic per pixel, fp32, every operation rounded on its own (no contraction), (pu, pv) the prediction, (gu, gv) the ground truth:
 *   valid pixel:      gu == gu && gv == gv (NaN marks missing ground truth: custom_data_layer.cpp, l1loss_layer.cu)
 *                     && |gu| <= 1e9 && |gv| <= 1e9 (the .flo unknown-flow convention) && (valid absent || valid != 0)
 *   non-finite pixel: a valid pixel whose pu or pv is NaN or +-Inf: counted in NONFINITE, left out of everything else
 *   counted pixel:    valid and not non-finite; VALID is the number of counted pixels, the denominator of every mean
 *   du = pu - gu; dv = pv - gv; s = du*du + dv*dv; epe = sqrtf(s); mag = sqrtf(gu*gu + gv*gv)
 *   outlier:  epe > outlier_abs && epe > outlier_rel * mag                      (KITTI: 3 px and 5 %)
 *   band:     0 when mag < band0, 1 when mag < band1, else 2                    (Sintel: 10 and 40 px)
 *   angular error (radians) between (pu, pv, 1) and (gu, gv, 1):
 *     cx = pv - gv; cy = gu - pu; cz = pu*gv - pv*gu; ae = atan2f(sqrtf((cx*cx + cy*cy) + cz*cz), (1 + pu*gu) + pv*gv)
 *     (|a x b| over a . b; the acos form of the same angle loses half its digits where the flows agree)
 *   occluded: occ given and occ != 0
 *
 * results: DEVICE double [(N + 1) * FN2_FLOW_METRICS_K]: one row per sample, then a totals row; columns as the enum below.  Counts are
 * exact integers held in doubles; sums are fp64 sums of the fp32 per-pixel values; nothing is divided (means are the caller's).
 *   VALID, NONFINITE                 counts as above
 *   EPE_SUM, EPE_SQ_SUM, EPE_MAX     sum of epe, sum of s, largest epe (0 without a counted pixel)
 *   OUTLIERS, AE_SUM                 number of outliers, sum of ae
 *   BAND_COUNT0..2, BAND_EPE_SUM0..2 counted pixels and sum of epe per band
 *   OCC_COUNT, OCC_EPE_SUM           counted occluded pixels and their sum of epe (0 without occ)
 * The totals row is the fp64 sum of the sample rows in sample order (starting from 0), the max for EPE_MAX.
 * epe_map (optional) float [N,1,H,W] receives epe, NaN where the pixel is not counted; asking for it changes no bit of the results.
 *
 * Order of the sums: fixed by (H, W) alone.  A sample is cut into B = min(ceil(H W / 1024), 128) workgroups of 256 threads; where H W is a
 * multiple of 4 a thread owns four neighbouring pixels per step (one 16-byte load per plane where every pointer given is 16-byte aligned,
 * four 4-byte loads otherwise: same values, same order, same bits), one pixel per step otherwise; a thread adds its pixels in ascending
 * order, a wave64 shuffle tree and the four waves in order give the workgroup's partial row in the workspace; one finalise workgroup adds a
 * sample's B partial rows in index order.  So a sample's row has the same bits alone or in any batch, from run to run and for any
 * allocation.  Two launches, no floating-point atomics, no host synchronisation.
 *
 * fn2_flow_metrics_sizes is host-only: the workspace bytes for (N, H, W) -- N times a per-sample size that grows with H W -- and K.
 * fn2_flow_metrics returns FN2_OK or refuses on the host before any launch, writing nothing: FN2_ERR_INVALID_ARG a NULL pred, gt or
 * results, a non-positive extent, a blob of 2^31 elements or more (N 2 H W), a NaN or negative outlier_abs, outlier_rel, band0 or band1,
 * band0 >= band1; FN2_ERR_WORKSPACE a workspace that is NULL or too small.  _sizes refuses the same extents and then writes nothing. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
enum {
  FN2_FLOW_METRICS_VALID = 0,
  FN2_FLOW_METRICS_NONFINITE,
  FN2_FLOW_METRICS_EPE_SUM,
  FN2_FLOW_METRICS_EPE_SQ_SUM,
  FN2_FLOW_METRICS_EPE_MAX,
  FN2_FLOW_METRICS_OUTLIERS,
  FN2_FLOW_METRICS_AE_SUM,
  FN2_FLOW_METRICS_BAND_COUNT0,
  FN2_FLOW_METRICS_BAND_COUNT1,
  FN2_FLOW_METRICS_BAND_COUNT2,
  FN2_FLOW_METRICS_BAND_EPE_SUM0,
  FN2_FLOW_METRICS_BAND_EPE_SUM1,
  FN2_FLOW_METRICS_BAND_EPE_SUM2,
  FN2_FLOW_METRICS_OCC_COUNT,
  FN2_FLOW_METRICS_OCC_EPE_SUM,
  FN2_FLOW_METRICS_K
};
/* either out-pointer may be NULL */
int fn2_flow_metrics_sizes(int N, int H, int W, size_t* workspace_bytes, int* K);
/* valid, occ, epe_map: NULL = absent; results: DEVICE double [(N + 1) * FN2_FLOW_METRICS_K] */
int fn2_flow_metrics(const float* pred, const float* gt, const float* valid, const float* occ, int N, int H, int W, float outlier_abs,
                     float outlier_rel, float band0, float band1, double* results, float* epe_map, void* workspace, size_t workspace_bytes,
                     void* stream);
#ifdef __cplusplus
}
#endif
