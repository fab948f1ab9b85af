/* Dense point trajectories (csrc/flow_track.hip): points carried through a sequence of forward and backward flows, each stopped where it
 * is occluded, leaves the image or is marked (a motion boundary), and new points seeded where coverage is lost.  A header of its own,
 * includable on its own.  A library call, not a Caffe layer, and not differentiable: the reference tree has no counterpart.  The method is
 * that of Sundaram, Brox and Keutzer, "Dense point trajectories by GPU-accelerated large displacement optical flow" (ECCV 2010), on the
 * sampling and the consistency test of flownet2_hip_flow_consistency.h; their structure-tensor test for where to seed is not built.
 *
 * Layouts, all contiguous and planar.  Float pointers need 4-byte alignment only; results and the workspace hold doubles (8 bytes).
 *   fw, bw      float [N,T,2,H,W]          fw[n,t] maps frame t to frame t+1, bw[n,t] frame t+1 to frame t (u plane, then v plane)
 *   stop        unsigned char [N,T,1,H,W]  or NULL; for instance the flags_fw plane of fn2_flow_consistency for every frame
 *   stop_mask   unsigned                   a point stops where stop & stop_mask != 0
 *   points      float [N,2,P]              x plane, then y plane: the positions in frame 0
 *   state_in    unsigned char [N,P]        or NULL = every point alive.  A point with a non-zero entry passes through: state_out = state_in,
 *                                          points_out = points, steps = 0, tracks[:,0] = points and NaN afterwards; it is in no count but POINTS
 *   tracks      float [N,T+1,2,P]          or NULL.  tracks[:,0] = points; the position in every frame up to the last one reached, NaN after
 *   points_out  float [N,2,P]              or NULL.  The last position reached (= points for a point that did not move); may be `points` itself
 *   state_out   unsigned char [N,P]        0 = alive, else one FN2_FLOW_TRACK_STOP_* value; may be `state_in` itself
 *   steps       int [N,P]                  or NULL.  Frames advanced in this call, 0 .. T
 * For a dense grid P = H W and a points plane is itself a [N,2,H,W] blob.  Asking for an optional output changes no bit of another.
 *
 * Arithmetic per point, fp32, every operation rounded on its own (no contraction).  ok(t) means |t| <= 1e9, false for NaN and +-Inf.
 *   0. (x, y) = points.  !ok(x) || !ok(y): NONFINITE, 0 steps.  Not (x >= 0 && y >= 0 && x < W && y < H): OUTSIDE, 0 steps.  No index is
 *      formed for such a point.
 *   then for t = 0 .. T-1 while the point is alive:
 *   1. ixL = (int)x, ixR = min(ixL + 1, W - 1), iyT = (int)y, iyB = min(iyT + 1, H - 1), al = x - ixL, be = y - iyT; per channel of fw[n,t],
 *      with TL = f[iyT, ixL], TR = f[iyT, ixR], BL = f[iyB, ixL], BR = f[iyB, ixR]:
 *      a = ((((1-al)*(1-be))*TL + (al*(1-be))*TR) + ((1-al)*be)*BL) + (al*be)*BR   (step 5 of the consistency header).
 *      !ok(au) || !ok(av): NONFINITE.
 *   2. with stop: jx = min((int)(x + 0.5f), W - 1), jy = min((int)(y + 0.5f), H - 1); stop[n,t,0,jy,jx] & stop_mask != 0: MARKED.
 *   3. x2 = x + au, y2 = y + av.  Not (x2 >= 0 && y2 >= 0 && x2 < W && y2 < H) (FlowWarp's rule): OUTSIDE.
 *   4. (bu, bv): bw[n,t] sampled at (x2, y2) as in 1.  !ok(bu) || !ok(bv): NONFINITE.
 *   5. su = au + bu, sv = av + bv, s = su*su + sv*sv, m = (au*au + av*av) + (bu*bu + bv*bv); s > alpha1 * m + alpha2: INCONSISTENT
 *      (step 6 of the consistency header).
 *   6. otherwise (x, y) = (x2, y2) and steps grows by one.
 * A point that stops keeps the position it had.  The published constants are alpha = (0.01, 0.5).
 * No index is formed before the finite test and the inside test of the position it is formed from have passed, and every one is clamped as
 * in 1 and 2: nothing outside [0,W) x [0,H) of the point's own sample is ever read, whatever the inputs hold.
 *
 * results: DEVICE double [(N + 1) * FN2_FLOW_TRACK_K]: one row per sample, then a totals row; columns as the first enum below.  Counts are
 * exact integers held in doubles.
 *   POINTS                                      P
 *   ALIVE                                       points with state_out == 0
 *   NONFINITE, OUTSIDE, INCONSISTENT, MARKED    points that were alive on entry and stopped in this call, by reason
 *   STEPS_SUM, STEPS_MAX                        sum and maximum of steps
 *   DISP_SUM, DISP_MAX                          over the points alive at the end, with dx = x - x0, dy = y - y0 between `points` and the last
 *                                               position: the fp64 sum and the maximum of the fp32 sqrtf(dx*dx + dy*dy) (0 if none)
 * The totals row is the fp64 sum of the sample rows in sample order (starting from 0), the max for STEPS_MAX and DISP_MAX.
 *
 * Order of the sums: fixed by P alone.  A sample is cut into B = min(ceil(P / 1024), 128) workgroups of 256 threads; one point per thread
 * and step, the T frames in a loop inside the thread; workgroup c takes the points c * 256 + thread, then every B * 256 further on; a thread
 * adds its points in ascending order, a wave64 shuffle tree and the four waves in order give the workgroup's partial row in the
 * workspace; one finalise workgroup adds a sample's B partial rows in index order.  Every access is a 4-byte (or 1-byte) one, so a sample's
 * row and maps have the same bits alone or in any batch, from run to run and at any alignment.  Two launches, no floating-point atomics,
 * no host synchronisation.
 *
 * fn2_flow_track_reseed fills gaps in coverage, in place.  The plane is cut into cells of cell x cell pixels, P = ceil(H / cell) *
 * ceil(W / cell) slots, slot c = cy * ceil(W / cell) + cx has the home cell (cy, cx).  points float [N,2,P], state unsigned char [N,P],
 * born unsigned char [N,P] or NULL.  A coverage map of N P bytes in the workspace is cleared; every alive point with ok coordinates inside
 * [0,W) x [0,H) stores 1 into the byte of its cell ((int)y / cell, (int)x / cell) (the same byte value from every writer, so the map does
 * not depend on their order); then every slot that is NOT alive and whose home cell is uncovered becomes alive (state 0) at the cell's
 * centre, x = min(float(cx * cell) + 0.5f * float(cell - 1), float(W - 1)), y likewise, with born = 1; born is 0 for every other slot.
 * With every slot stopped the call produces the initial grid (cell = 1: the pixel grid); there is no separate grid entry point.  An alive
 * point that has wandered off its home cell keeps its slot, so an uncovered cell whose slot is busy stays uncovered.  Three launches.
 *
 * fn2_flow_track_sizes is host-only: K, and the workspace bytes that serve both calls for (N, P): max(8 K N B, N P).  Every entry point
 * returns FN2_OK or refuses on the host before any launch, writing nothing: FN2_ERR_INVALID_ARG a NULL fw, bw, points, state_out or
 * results (reseed: points or state), a non-positive extent (N, T, H, W, P, cell), a blob of 2^31 elements or more (N T 2 H W,
 * N (T+1) 2 P), a NaN or negative alpha1 or alpha2; FN2_ERR_WORKSPACE a workspace that is NULL or too small (8 K N B bytes for
 * fn2_flow_track, N P for the reseed).  _sizes refuses the same extents and then writes nothing. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
enum {
  FN2_FLOW_TRACK_POINTS = 0,
  FN2_FLOW_TRACK_ALIVE,
  FN2_FLOW_TRACK_NONFINITE,
  FN2_FLOW_TRACK_OUTSIDE,
  FN2_FLOW_TRACK_INCONSISTENT,
  FN2_FLOW_TRACK_MARKED,
  FN2_FLOW_TRACK_STEPS_SUM,
  FN2_FLOW_TRACK_STEPS_MAX,
  FN2_FLOW_TRACK_DISP_SUM,
  FN2_FLOW_TRACK_DISP_MAX,
  FN2_FLOW_TRACK_K
};
enum {
  FN2_FLOW_TRACK_STOP_NONFINITE = 1,
  FN2_FLOW_TRACK_STOP_OUTSIDE = 2,
  FN2_FLOW_TRACK_STOP_INCONSISTENT = 4,
  FN2_FLOW_TRACK_STOP_MARKED = 8
};
/* either out-pointer may be NULL */
int fn2_flow_track_sizes(int N, int T, int H, int W, int P, size_t* workspace_bytes, int* K);
/* stop, state_in, tracks, points_out, steps: NULL = absent; results: DEVICE double [(N + 1) * FN2_FLOW_TRACK_K] */
int fn2_flow_track(const float* fw, const float* bw, const unsigned char* stop, unsigned stop_mask, const float* points,
                   const unsigned char* state_in, int N, int T, int H, int W, int P, float alpha1, float alpha2, double* results, float* tracks,
                   float* points_out, unsigned char* state_out, int* steps, void* workspace, size_t workspace_bytes, void* stream);
/* born: NULL = absent */
int fn2_flow_track_reseed(float* points, unsigned char* state, unsigned char* born, int N, int H, int W, int cell, void* workspace,
                          size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
