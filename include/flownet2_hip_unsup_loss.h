/* Unsupervised training loss (csrc/unsup_loss.hip): brightness constancy over the pixels that are not occluded plus an edge-aware
 * smoothness prior on the flow, one fused pass per direction of differentiation.  A header of its own, includable on its own.  A library
 * call with a gradient, not a Caffe layer: the reference tree has no counterpart.  The penalty is the generalised Charbonnier function
 * psi(t) = (t^2 + eps^2)^gamma of Sun, Roth and Black, "Secrets of optical flow estimation and their principles" (CVPR 2010); masking by
 * forward-backward occlusion, the first- and second-order smoothness and the image-edge weight follow Meister, Hur and Roth, "UnFlow"
 * (AAAI 2018), and Jason, Harley and Derpanis, "Back to basics" (ECCV 2016 workshops).
 *
 * Inputs: img0, img1 contiguous float [N,C,H,W], C in 1 .. 4; fw contiguous float [N,2,H,W] (u plane, then v plane), frame 0 to frame 1;
 * bw likewise, frame 1 to frame 0, or NULL (one direction only); occ_fw, occ_bw float [N,1,H,W] or NULL (nothing occluded): the occ planes
 * of fn2_flow_consistency go in as they are.  Float pointers need 4-byte alignment only; results and the workspace hold doubles.
 * Direction 0 uses a = fw, Ia = img0, Io = img1, occ = occ_fw; direction 1 uses a = bw, Ia = img1, Io = img0, occ = occ_bw.
 *
 * Arithmetic, fp32, every operation rounded on its own (no contraction); sums over channels run in ascending c from 0.0f.  ok(t) means
 * |t| <= 1e9 (false for NaN and +-Inf, as in flownet2_hip_flow_consistency.h); "not finite" means !ok.
 *   flow(p) = (au, av) = (flow_mult * a_u[p], flow_mult * a_v[p]), one rounding each: a prediction at a coarse scale in FlowNet's 1/20
 *   units becomes pixels of that scale.  ok is tested on the scaled values.
 *   psi(t; eps, gamma):  r = t*t + eps*eps;  psi = sqrtf(r) when gamma == 0.5f, powf(r, gamma) otherwise
 *   psi'(t; eps, gamma): t / sqrtf(r) when gamma == 0.5f, ((2.0f*gamma) * t) * powf(r, gamma - 1.0f) otherwise
 *
 * Data term of pixel p = (x, y); the first test that holds decides, the pixel is counted in that column and has no data term:
 *   1. !ok(au) || !ok(av): NONFINITE.
 *   2. occ given and !(occ[p] == 0.0f) (so a NaN too): OCCLUDED.
 *   3. x2 = float(x) + au, y2 = float(y) + av; !(x2 >= 0 && y2 >= 0 && x2 < W && y2 < H) (FlowWarp's rule): OUTSIDE.
 *   4. ixL = (int)x2, ixR = min(ixL + 1, W - 1), iyT = (int)y2, iyB = min(iyT + 1, H - 1), al = x2 - ixL, be = y2 - iyT;
 *      cTL = (1-al)*(1-be), cTR = al*(1-be), cBL = (1-al)*be, cBR = al*be  (FlowWarp's taps and weights).  No index is formed before 1-3
 *      have passed, and every one is clamped: nothing outside [0,W) x [0,H) of the pixel's own sample is read.
 *   5. per channel c: TL = Io[c,iyT,ixL], TR = Io[c,iyT,ixR], BL = Io[c,iyB,ixL], BR = Io[c,iyB,ixR], I = Ia[c,y,x]; one of the five not
 *      finite, in any channel: NONFINITE.  warped = ((cTL*TL + cTR*TR) + cBL*BL) + cBR*BR;  d_c = I - warped.
 *   6. COUNTED; e = sum_c psi(d_c; eps_d, gamma_d); DATA_SUM += double(e).
 *
 * Smoothness terms, on flow(.), not masked by occ.  Pixel p owns one term per axis (x: step (1,0); y: step (0,1)):
 *   order 1: exists where p+ = p + step is inside;  s = flow(p+) - flow(p);  q = p
 *   order 2: exists where p- = p - step and p+ are inside;  s = (flow(p-) - 2.0f*flow(p)) + flow(p+);  q = p-
 *   (per component, s_u and s_v).  An axis of extent 1 (or 2 at order 2) has no terms.
 *   edge_weight == 0: wgt = 1.0f, no image value is read and no expf is executed.  Otherwise g = sum_c |Ia[c,p+] - Ia[c,q]|,
 *   wgt = expf((-edge_weight) * (g / float(C))).
 *   term = wgt * (psi(s_u; eps_s, gamma_s) + psi(s_v; eps_s, gamma_s));  SMOOTH_TERMS += 1;  SMOOTH_SUM += double(term), the x term of a
 *   pixel before its y term.
 *   A term is dropped -- not counted, zero gradient -- where one of the flow values it reads is not finite or, with edge_weight != 0, one
 *   of the image values it reads is not finite.
 *
 * results: DEVICE double [2][(N + 1) * FN2_UNSUP_LOSS_K]: per direction one row per sample, then a totals row (the fp64 sum of the sample
 * rows in sample order, from 0); columns as the enum below; counts are exact integers held in doubles; PIXELS = H W = COUNTED + OCCLUDED +
 * OUTSIDE + NONFINITE.  Without bw the rows of direction 1 are written as zeros.
 * loss: DEVICE float[1] or NULL; asking for it changes no other bit.  In fp64, from the totals rows, over the directions given in order,
 * from 0:  L += (double(data_weight) * DATA_SUM) / max(COUNTED, 1) + (double(smooth_weight) * SMOOTH_SUM) / max(SMOOTH_TERMS, 1);
 * loss = float(L), rounded once.
 *
 * Order of the sums: fixed by (H, W) alone, the cut of flownet2_hip_flow_consistency.h.  A (direction, sample) is cut into
 * B = min(ceil(H W / 1024), 128) workgroups of 256 threads; where W is a multiple of 4 a thread owns four neighbouring pixels of a row per
 * step (16-byte loads and stores where every pointer given is 16-byte aligned, 4-byte ones otherwise: same values, same order, same bits),
 * one pixel per step otherwise; unit u = chunk * 256 + thread, then every B * 256 further on; a thread adds its pixels in ascending order,
 * a wave64 shuffle tree (offsets 32, 16, .. 1) and the four waves in order give the workgroup's partial row in the workspace; one finalise
 * workgroup adds a sample's B partial rows in index order.  A sample's row has the same bits alone or in any batch, from run to run and for
 * any allocation.  Two launches, no floating-point atomics, no host synchronisation.
 *
 * Backward: one launch, a pure gather; writes every element of fw_diff (and of bw_diff where given) = d loss / d fw (bw), times
 * total_diff[0] (a DEVICE scalar; NULL means 1).  It reads the normalisers from the totals rows of the forward's `results` on the device:
 *   kd = gdiff * float(double(data_weight) / max(COUNTED, 1)),  ks = gdiff * float(double(smooth_weight) / max(SMOOTH_TERMS, 1))
 * Data part of a COUNTED pixel (steps 1-5 are taken again): gy = float(iyB) - y2, gx = float(ixR) - x2 and per channel
 *   tu = gy*(TR - TL) + (1 - gy)*(BR - BL),  tv = gx*(BL - TL) + (1 - gx)*(BR - TR)    (the reference's flow gradient,
 *   flow_warp_layer.cu:203-227, whose `0 +` start can only change the sign of a zero),
 *   Su = sum_c psi'(d_c; eps_d, gamma_d) * tu,  Sv likewise with tv;  Du = (-kd) * Su,  Dv = (-kd) * Sv.  Any other pixel: Du = Dv = 0.0f.
 * Smoothness part, per component (u shown) and axis, with h(t) = wgt * psi'(s_u; eps_s, gamma_s) for the term t owned by a pixel and
 * h = 0.0f where that pixel is outside the plane or the term does not exist or was dropped:
 *   order 1: G_axis = h(p - step) - h(p);   order 2: G_axis = (h(p - step) - 2.0f*h(p)) + h(p + step);   G = G_x + G_y
 * fw_diff[p] = flow_mult * (Du + ks * G_u), and likewise v.  The images get no gradient.  bw given without bw_diff: direction 1 is left out.
 *
 * fn2_unsup_loss_sizes is host-only: the workspace bytes of the forward for (N, H, W) and K.  The other functions return FN2_OK or refuse
 * on the host before any launch, writing nothing: FN2_ERR_INVALID_ARG a NULL img0, img1, fw or results (backward: or fw_diff), a
 * non-positive extent, C outside 1 .. 4, a blob of 2^31 elements or more (N max(C, 2) H W; H W alone below 2^30), a NaN or negative
 * data_weight, smooth_weight, eps_d, eps_s or edge_weight, a NaN or non-positive gamma_d or gamma_s, a smooth_order other than 1 or 2, a
 * NaN flow_mult, a bw_diff without a bw; FN2_ERR_WORKSPACE a workspace that is NULL or too small.  _sizes refuses the same extents and then
 * writes nothing.  The header declares no structure. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
enum {
  FN2_UNSUP_LOSS_PIXELS = 0,
  FN2_UNSUP_LOSS_COUNTED,
  FN2_UNSUP_LOSS_OCCLUDED,
  FN2_UNSUP_LOSS_OUTSIDE,
  FN2_UNSUP_LOSS_NONFINITE,
  FN2_UNSUP_LOSS_DATA_SUM,
  FN2_UNSUP_LOSS_SMOOTH_TERMS,
  FN2_UNSUP_LOSS_SMOOTH_SUM,
  FN2_UNSUP_LOSS_K
};
/* either out-pointer may be NULL */
int fn2_unsup_loss_sizes(int N, int H, int W, size_t* workspace_bytes, int* K);
/* bw, occ_fw, occ_bw, loss: NULL = absent; results: DEVICE double [2][(N + 1) * FN2_UNSUP_LOSS_K] */
int fn2_unsup_loss_forward(const float* img0, const float* img1, const float* fw, const float* bw, const float* occ_fw, const float* occ_bw,
                           int N, int C, int H, int W, float data_weight, float smooth_weight, float eps_d, float gamma_d, float eps_s,
                           float gamma_s, float edge_weight, int smooth_order, float flow_mult, double* results, float* loss,
                           void* workspace, size_t workspace_bytes, void* stream);
/* results: what the forward wrote for the same inputs; total_diff: DEVICE float[1] or NULL (= 1); bw_diff: NULL = absent */
int fn2_unsup_loss_backward(const float* img0, const float* img1, const float* fw, const float* bw, const float* occ_fw, const float* occ_bw,
                            int N, int C, int H, int W, float data_weight, float smooth_weight, float eps_d, float gamma_d, float eps_s,
                            float gamma_s, float edge_weight, int smooth_order, float flow_mult, const double* results,
                            const float* total_diff, float* fw_diff, float* bw_diff, void* stream);
#ifdef __cplusplus
}
#endif
