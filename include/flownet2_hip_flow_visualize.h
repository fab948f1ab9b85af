/* Flow visualisation (csrc/flow_visualize.hip): the two pictures of a flow field -- the Middlebury colour coding, and the KITTI-style error
 * image, the picture form of the Fl outlier criterion that fn2_flow_metrics counts.  A header of its own, includable on its own.  Library
 * calls, not Caffe layers, and not differentiable: the reference tree has no counterpart.
 *
 * Blobs: flow, pred, gt contiguous float [N,2,H,W] (u plane, then v plane); valid, occ contiguous float [N,1,H,W] or NULL, the planes of
 * fn2_flow_metrics with the same meaning (non-zero = use the pixel / occluded); rgb unsigned char [N,H,W,3], interleaved, in PNG row
 * order.  The float pointers need 4-byte alignment only, rgb none.
 *
 * All arithmetic is fp32 and every operation is rounded on its own (no contraction, no fast-math).  ok(t) means |t| <= 1e9, which is
 * false for NaN and +-Inf (1e9: the .flo unknown-flow convention, as in flownet2_hip_flow_metrics.h and flownet2_hip_flow_consistency.h).
 *
 * fn2_flow_color -- the colour coding of Baker et al., "A Database and Evaluation Methodology for Optical Flow" (IJCV 2011), written
 * from that published definition.
 *   The wheel: 55 entries (R,G,B) of integers from the segment lengths RY = 15, YG = 6, GC = 4, CB = 11, BM = 13, MR = 6, with integer
 *   division, for i = 0 .. length - 1 of each segment in this order:
 *     RY (255, 255*i/15, 0)   YG (255 - 255*i/6, 255, 0)    GC (0, 255, 255*i/4)
 *     CB (0, 255 - 255*i/11, 255)   BM (255*i/13, 0, 255)   MR (255, 0, 255 - 255*i/6)
 *   Per pixel, with (u, v) its flow:
 *   1. !ok(u) || !ok(v): the three bytes are 0 (unknown flow is black) and nothing else is computed for the pixel.
 *   2. rad = sqrtf(u*u + v*v); rn = rad / maxrad.
 *   3. a = atan2f(-v, -u) / PI_F (PI_F = 3.14159265358979323846f); fk = ((a + 1.0f) * 0.5f) * 54.0f; k0 = min((int)fk, 54);
 *      k1 = (k0 + 1) % 55; f = fk - (float)k0.  Signed zeros go to atan2f as they are.
 *   4. per channel, with w0, w1 the wheel integers of k0, k1 as floats: c = w0 + f * (w1 - w0);
 *      rn <= 1: out = 255.0f - rn * (255.0f - c); otherwise out = 0.75f * c (the out-of-range convention);
 *      byte = (unsigned char)(int)out  (truncation: the original's rule).
 *   maxrad, by `norm`:
 *     FN2_FLOW_COLOR_NORM_SAMPLE   the largest rad over the sample's known pixels
 *     FN2_FLOW_COLOR_NORM_BATCH    the largest rad over the known pixels of all samples
 *     FN2_FLOW_COLOR_NORM_FIXED    the argument max_flow (> 0)
 *   In the first two modes a maximum of 0 (no known pixel included) is replaced by 1.  maxrad_out: optional DEVICE float [N], the maxrad
 *   used for each sample; asking for it changes no byte of rgb.
 *   Where this differs from the original tool (color_flow / colorcode.cpp), on purpose:
 *     - the original divides u and v by maxrad and takes the radius of the quotients, which can round the very pixel that holds the
 *       maximum to a radius above 1 and onto the out-of-range branch.  Here rn is formed from the unnormalised radius, so that pixel has
 *       rn == 1.0f exactly (x / x is 1 in IEEE arithmetic).
 *     - the original computes 1 - rad * (1 - c / 255) and multiplies by 255; here the factor 255 is multiplied through, which is the same
 *       real function and keeps the exact cases exact: c is exactly w0 where w0 == w1, so a saturated channel stays 255 for every rn, and
 *       rn == 0 (zero flow) gives 255 in every channel: white, bit for bit.
 *     - the original picks maxrad per image on the host (and lets the caller scale it); here the three rules above, on the device.
 *   What is kept: the coding has a seam of one wheel step at v = +-0, u > 0, since atan2f(-0.0f, -u) = -pi gives wheel entry 0 and
 *   atan2f(+0.0f, -u) = +pi gives entry 54.  That seam is Middlebury's.
 *
 * fn2_flow_error_map -- the error image.  Per pixel, with (pu, pv) the prediction and (gu, gv) the ground truth:
 *   1. !ok(gu) || !ok(gv), or valid present and 0 there: the bytes are 0.
 *   2. otherwise, !ok(pu) || !ok(pv): the colour of the last bin.
 *   3. otherwise du = pu - gu; dv = pv - gv; epe = sqrtf(du*du + dv*dv); mag = sqrtf(gu*gu + gv*gv); n = epe / abs_thresh;
 *      if (mag > 0) n = fminf(n, (epe / mag) / rel_thresh).
 *   4. the colour of the bin with lo <= n < hi:
 *        [0, 0.0625)     49  54 149      [0.0625, 0.125)  69 117 180      [0.125, 0.25)  116 173 209      [0.25, 0.5)  171 217 233
 *        [0.5, 1)       224 243 248      [1, 2)          254 224 144      [2, 4)         253 174  97      [4, 8)       244 109  67
 *        [8, 16)        215  48  39      [16, inf]       165   0  38
 *      This table is the definition, whatever a given devkit version holds.
 *   5. occ present and non-zero there: each byte becomes (unsigned char)(int)(0.5f * byte)  (every pixel, those of 1 and 2 included).
 *   The published thresholds are abs_thresh = 3, rel_thresh = 0.05.  n >= 1 is the Fl outlier test of fn2_flow_metrics (epe > outlier_abs
 *   && epe > outlier_rel * mag) rearranged; the two can differ by rounding: at epe == outlier_abs or epe == outlier_rel * mag exactly
 *   (strict there, n == 1 here counts as beyond), and where a quotient epe / abs_thresh or (epe / mag) / rel_thresh rounds across 1
 *   while the product comparison does not (two more roundings here, and outlier_rel * mag is itself rounded there); with mag == 0 the
 *   relative test there is epe > 0 and is left out here, which agrees wherever epe > abs_thresh.
 *   The devkit's dilation of sparse error pixels is not part of this call.
 *
 * Launch shape, both calls: workgroups of 256 threads, a sample cut into B = min(ceil(H W / 1024), 128) workgroups.  Where W is a multiple
 * of 4 a thread owns four neighbouring pixels of a row per step: 16-byte loads where every float pointer given is 16-byte aligned (4-byte
 * ones otherwise), and its 12 output bytes as three 4-byte stores where rgb is 4-byte aligned (twelve byte stores otherwise).  Otherwise
 * a thread owns one pixel per step and stores byte by byte.  The forms compute the same values and give the same bytes.  No byte outside
 * [N,H,W,3] is written.
 *   The maximum (NORM_SAMPLE, NORM_BATCH): a first launch writes one maximum per workgroup to the workspace (float [N][B]); the colouring
 *   launch reduces its sample's B partial maxima (all N B under NORM_BATCH) itself.  No host readback, no floating-point atomics; a
 *   maximum does not depend on order, so a sample's bytes under NORM_SAMPLE and NORM_FIXED are the same alone and in any batch.
 *   NORM_FIXED is a single launch and needs no workspace (workspace may be NULL); fn2_flow_error_map is a single launch.
 *
 * fn2_flow_visualize_sizes is host-only: the workspace bytes of fn2_flow_color for (N, H, W).  The calls return FN2_OK or refuse on the
 * host before any launch, writing nothing: FN2_ERR_INVALID_ARG a NULL flow / pred / gt / rgb, a non-positive extent, a blob of 2^31
 * elements or more (N 2 H W), an unknown norm, a max_flow that is NaN or <= 0 under NORM_FIXED, an abs_thresh or rel_thresh that is NaN
 * or <= 0; FN2_ERR_WORKSPACE a workspace that is NULL or too small under NORM_SAMPLE and NORM_BATCH.  _sizes refuses the same extents and
 * then writes nothing. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
enum {
  FN2_FLOW_COLOR_NORM_SAMPLE = 0,
  FN2_FLOW_COLOR_NORM_BATCH,
  FN2_FLOW_COLOR_NORM_FIXED
};
/* the out-pointer may be NULL */
int fn2_flow_visualize_sizes(int N, int H, int W, size_t* workspace_bytes);
/* max_flow is read under NORM_FIXED only; maxrad_out: DEVICE float [N] or NULL; workspace: needed under NORM_SAMPLE and NORM_BATCH */
int fn2_flow_color(const float* flow, int N, int H, int W, int norm, float max_flow, unsigned char* rgb, float* maxrad_out, void* workspace,
                   size_t workspace_bytes, void* stream);
/* valid, occ: NULL = absent */
int fn2_flow_error_map(const float* pred, const float* gt, const float* valid, const float* occ, int N, int H, int W, float abs_thresh,
                       float rel_thresh, unsigned char* rgb, void* stream);
#ifdef __cplusplus
}
#endif
