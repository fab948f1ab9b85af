/* Census data term of the unsupervised loss (csrc/census_loss.hip): the soft Hamming distance between the ternary census signatures of
 * an image and of the other image warped by the flow, over a (2 radius + 1)^2 patch, under the generalised Charbonnier penalty.  It
 * compares the ORDER of the grey values inside a patch, not the values: an additive change of brightness (exposure, shadow, gain offset)
 * leaves it unchanged, where the brightness-constancy term of flownet2_hip_unsup_loss.h pays for it.  A header of its own, includable on
 * its own.  A library call with a gradient, not a Caffe layer: the reference tree has no counterpart.  The signature, the soft distance and
 * the constants follow Meister, Hur and Roth, "UnFlow" (AAAI 2018), after Zabih and Woodfill (ECCV 1994) and Stein (DAGM 2004).
 *
 * Inputs: img0, img1 contiguous float [N,C,H,W], C in 1 .. 4; fw contiguous float [N,2,H,W] (u plane, then v plane), frame 0 to frame 1;
 * bw likewise, frame 1 to frame 0, or NULL (one direction only); occ_fw, occ_bw float [N,1,H,W] or NULL (nothing occluded): the occ planes
 * of fn2_flow_consistency go in as they are.  Float pointers need 4-byte alignment only; results and the workspace hold doubles.
 * Direction 0 uses a = fw, Ia = img0, Io = img1, occ = occ_fw; direction 1 uses a = bw, Ia = img1, Io = img0, occ = occ_bw.
 *
 * Arithmetic, fp32, every operation rounded on its own (no contraction), division and sqrtf correctly rounded; sums over channels run in
 * ascending c from 0.0f.  ok(t) means |t| <= 1e9 (false for NaN and +-Inf, as in flownet2_hip_flow_consistency.h); "not finite" means !ok.
 *   flow(p) = (au, av) = (flow_mult * a_u[p], flow_mult * a_v[p]), one rounding each: a prediction at a coarse scale in FlowNet's 1/20
 *   units becomes pixels of that scale.  ok is tested on the scaled values.
 *   psi(t; eps, gamma):  r = t*t + eps*eps;  psi = sqrtf(r) when gamma == 0.5f, powf(r, gamma) otherwise
 *   psi'(t; eps, gamma): t / sqrtf(r) when gamma == 0.5f, ((2.0f*gamma) * t) * powf(r, gamma - 1.0f) otherwise
 *   gsc = intensity_scale / float(C)
 *
 * Two grey values per pixel p = (x, y) and direction:
 *   G(p), the own image: DEFINED where every Ia[c,p] is ok;  G = (sum_c Ia[c,p]) * gsc.
 *   Wg(p), the other image warped by the flow: DEFINED where
 *     1. ok(au) && ok(av);
 *     2. x2 = float(x) + au, y2 = float(y) + av;  x2 >= 0 && y2 >= 0 && x2 < W && y2 < H (FlowWarp's rule);
 *     3. ixL = (int)x2, ixR = min(ixL + 1, W - 1), iyT = (int)y2, iyB = min(iyT + 1, H - 1), al = x2 - ixL, be = y2 - iyT;
 *        cTL = (1-al)*(1-be), cTR = al*(1-be), cBL = (1-al)*be, cBR = al*be  (FlowWarp's taps and weights); per channel c
 *        TL = Io[c,iyT,ixL], TR = Io[c,iyT,ixR], BL = Io[c,iyB,ixL], BR = Io[c,iyB,ixR]: all four ok, in every channel.
 *     warped_c = ((cTL*TL + cTR*TR) + cBL*BL) + cBR*BR;  Wg = (sum_c warped_c) * gsc.
 *   occ plays no part in whether Wg is defined: an occluded pixel still has a warped value and still serves its neighbours' patches, as in
 *   UnFlow.  No index is formed before 1 and 2 have passed, and every one is clamped: nothing outside [0,W) x [0,H) of the pixel's own
 *   sample is read.
 *
 * Status of p, the first rule that holds: !ok(au) || !ok(av): NONFINITE;  occ given and !(occ[p] == 0.0f) (so a NaN too): OCCLUDED;  the
 * target outside (2): OUTSIDE;  G(p) or Wg(p) not defined: NONFINITE;  otherwise COUNTED.  PIXELS = H W is the sum of the four.
 *
 * Pairs.  q = (dx, dy) runs over [-radius, radius]^2 without (0, 0).  The pair (p, q) EXISTS where p + q lies inside the plane and G and Wg
 * are both defined at p + q and at p: one rule for the image border and for undefined neighbours (UnFlow masks a border of `radius`
 * pixels instead; here every pixel keeps a term and maps smaller than the patch work).  For an existing pair
 *   a  = G(p+q) - G(p);    ra = a*a + c_t;   ta = a / sqrtf(ra)
 *   b  = Wg(p+q) - Wg(p);  rb = b*b + c_t;   tb = b / sqrtf(rb)
 *   e  = ta - tb;   s = e*e;   den = s + c_h;   h = s / den
 * A COUNTED pixel: dist(p) = sum_q h over its existing pairs in row-major order (dy ascending, then dx ascending) from 0.0f;  PAIRS +=
 * their number;  DIST_SUM += double(dist);  DATA_SUM += double(psi(dist; eps_d, gamma_d));  pd(p) = psi'(dist; eps_d, gamma_d).  Any other
 * pixel: pd(p) = 0.0f.  (Exchanging the two pixels of a pair negates a, b, ta, tb and e exactly, so h(p, q) and h(p+q, -q) have the same
 * bits.)
 *
 * results: DEVICE double [2][(N + 1) * FN2_CENSUS_LOSS_K]: per direction one row per sample, then a totals row (the fp64 sum of the sample
 * rows in sample order, from 0); columns as the enum below; counts are exact integers held in doubles.  Without bw the rows of direction 1
 * are written as zeros.
 * loss: DEVICE float[1] or NULL; asking for it changes no other bit.  In fp64, from the totals rows, over the directions given in order,
 * from 0:  L += (double(data_weight) * DATA_SUM) / max(COUNTED, 1);  loss = float(L), rounded once.
 * saved: DEVICE float [2][N][3][H][W] or NULL (no backward will follow): per direction and sample the planes G, Wg and pd; an undefined G
 * or Wg is stored as a quiet NaN, which is how "defined" is read back.  A direction that is not run is not written.
 *
 * Order of the sums: fixed by (H, W) alone.  A plane is cut into tiles of 32 x 8 pixels, T = ceil(W / 32) ceil(H / 8) of them in row-major
 * order; a (direction, sample) is cut into B = min(T, 128) workgroups of 256 threads, one pixel of a tile per thread; workgroup k takes the
 * tiles k, k + B, ...; a thread adds its pixels in that order, a wave64 shuffle tree (offsets 32, 16, .. 1) and the four waves in order
 * give the workgroup's partial row in the workspace; one finalise workgroup adds a sample's B partial rows in index order.  A sample's row
 * has the same bits alone or in any batch, from run to run, for any radius' tile and for any allocation.  Three launches (warp, stencil,
 * finalise), no floating-point atomics, no host synchronisation.
 *
 * Backward: one launch, a pure gather; writes every element of fw_diff (and of bw_diff where given) = d loss / d fw (bw), times
 * total_diff[0] (a DEVICE scalar; NULL means 1).  It reads G, Wg and pd from `saved` and the normaliser from the totals rows of `results`:
 *   kd = gdiff * float(double(data_weight) / max(COUNTED, 1))
 * A pixel r where G(r) or Wg(r) is not defined (no pair holds it) gets 0.0f.  Otherwise, over the existing pairs (r, q), row-major from 0.0f:
 *   F    = -(((2.0f*c_h) * e) / (den*den)) * (c_t / (rb * sqrtf(rb)))            (dh/db)
 *   acc += (pd(r) + pd(r+q)) * F
 * DW = (-kd) * acc.  (F is odd in (a, b), and Wg(r) enters b with coefficient -1 as a centre and +1 as a neighbour: the gather over the
 * patches that contain r collapses into this one sum over r's own patch.)  The taps of r are taken again (1-3 above; a flow that fails 1
 * or 2 here gives 0.0f), gy = float(iyB) - y2, gx = float(ixR) - x2 and per channel
 *   tu = gy*(TR - TL) + (1 - gy)*(BR - BL),  tv = gx*(BL - TL) + (1 - gx)*(BR - TR)    (as in flownet2_hip_unsup_loss.h)
 *   Su = sum_c tu,  Sv = sum_c tv;   fw_diff_u[r] = flow_mult * ((DW * gsc) * Su),  fw_diff_v[r] = flow_mult * ((DW * gsc) * Sv).
 * An occluded pixel therefore does get a gradient, through its neighbours' patches.  The images get none.  bw given without bw_diff:
 * direction 1 is left out.
 *
 * fn2_census_loss_sizes is host-only: the workspace bytes of the forward for (N, H, W) (the partial rows, and room for the three planes
 * of a forward without `saved`), the floats of `saved`, and K.  The other functions return FN2_OK or refuse on the host before any
 * launch, writing nothing: FN2_ERR_INVALID_ARG a NULL img0, img1, fw or results (backward: or fw_diff or saved), a non-positive extent, C
 * outside 1 .. 4, a blob of 2^31 elements or more (N max(C, 3) H W; H W alone below 2^30), a NaN or negative data_weight or eps_d, a NaN or
 * non-positive gamma_d, c_t, c_h or intensity_scale, a radius outside 1 .. 3, a NaN flow_mult, a bw_diff without a bw; FN2_ERR_WORKSPACE a
 * workspace that is NULL or too small.  _sizes refuses the same extents and radius and then writes nothing.  The header declares no
 * structure. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
enum {
  FN2_CENSUS_LOSS_PIXELS = 0,
  FN2_CENSUS_LOSS_COUNTED,
  FN2_CENSUS_LOSS_OCCLUDED,
  FN2_CENSUS_LOSS_OUTSIDE,
  FN2_CENSUS_LOSS_NONFINITE,
  FN2_CENSUS_LOSS_DATA_SUM,
  FN2_CENSUS_LOSS_PAIRS,
  FN2_CENSUS_LOSS_DIST_SUM,
  FN2_CENSUS_LOSS_K
};
/* any out-pointer may be NULL */
int fn2_census_loss_sizes(int N, int H, int W, int radius, size_t* workspace_bytes, size_t* saved_floats, int* K);
/* bw, occ_fw, occ_bw, loss, saved: NULL = absent; results: DEVICE double [2][(N + 1) * FN2_CENSUS_LOSS_K] */
int fn2_census_loss_forward(const float* img0, const float* img1, const float* fw, const float* bw, const float* occ_fw, const float* occ_bw,
                            int N, int C, int H, int W, float data_weight, float eps_d, float gamma_d, int radius, float c_t, float c_h,
                            float intensity_scale, float flow_mult, double* results, float* loss, float* saved, void* workspace,
                            size_t workspace_bytes, void* stream);
/* results, saved: what the forward wrote for the same inputs; total_diff: DEVICE float[1] or NULL (= 1); bw_diff: NULL = absent */
int fn2_census_loss_backward(const float* img0, const float* img1, const float* fw, const float* bw, int N, int C, int H, int W,
                             float data_weight, float eps_d, float gamma_d, int radius, float c_t, float c_h, float intensity_scale,
                             float flow_mult, const double* results, const float* saved, const float* total_diff, float* fw_diff,
                             float* bw_diff, void* stream);
#ifdef __cplusplus
}
#endif
