/* LpqLoss (csrc/lpq_loss.hip): loss = sum over (n, y, x) of ( sum_c w (|d_c| + p_eps)^p + q_eps )^q / normalize_coeff, d = bottom0 - bottom1.
 * A header of its own, includable on its own; it adds no structure, enumerator or constant.
 *
 *   replaces  LpqLossLayer::Forward_gpu    lpq_loss_layer.cu:97-198   (Eltwise, FindNotNaNs, blocking dot, KillMasked, ComputeSign,
 *                                                                      EltwiseMult, Power p, 1x1 Convolution, Power q, blocking dot, host loss)
 *             LpqLossLayer::Backward_gpu   lpq_loss_layer.cu:205-245  (Power q, Convolution, Power p backward, EltwiseMult, KillMasked,
 *                                                                      Eltwise backward)
 *             the five element-wise kernels lpq_loss_layer.cu:21-88
 *             the composition               lpq_loss_layer.cpp:84-143 (Eltwise coeff +1 / -1, Power{p, shift p_eps}, Convolution{1x1, constant
 *                                                                      1 or 1 / C, zero bias}, Power{q, shift q_eps}), Reshape :146-173
 *             PowerLayer::Forward_gpu / Backward_gpu  power_layer.cu:9-30, :33-80 (scale = 1)
 *             LpqLossParameter              caffe.proto:563-602
 *   The schedule (lpq_loss_layer.cpp:19-82, lpq_loss_layer.cu:100-135) is the caller's: p and q are arguments of every call;
 *   fn2_lpq_loss_schedule_step picks the episode.
 *
 * Arithmetic, fp32, every operation rounded on its own (no contraction):
 *   d = b0 - b1 (b0 alone with one bottom); ok = (d == d); d = ok ? d : 0; a = |d|; t = a + p_eps
 *   u = t (p == 1), 1 (p == 0), powf(t, p) otherwise          a masked element still contributes (0 + p_eps)^p, as in the reference
 *   s = sum_c w u_c in ascending c, w = 1 / C with l2_prescale_by_channels, else 1;   v = (s + q_eps)^q by the same three cases
 *   loss = float(sum of v in fp64 / normalize_coeff), normalize_coeff = float(valid entries) / float(C) with normalize_by_num_entries, else N
 * The fp64 sum runs in an order fixed by [N, C, H, W] alone (a plane size that is a multiple of 4 gives every thread four neighbouring
 * pixels, read as one 16-byte load where every pointer is 16-byte aligned and as four 4-byte loads otherwise: same order, same bits); no
 * floating-point atomics; bits are the same from run to run and for any allocation.  Pointers need 4-byte alignment only.
 * Backward recomputes the element-wise terms from the bottoms (no sign or mask blob), alpha = top_diff / normalize_coeff:
 *   dq = 1 (q == 1), 0 (q == 0), 2 (s + q_eps) (q == 2), q * (v / (s + q_eps)) otherwise (with q_eps == 0 that is the reference's q * (v / s));
 *   du likewise from p, t, u;   g = (((alpha dq) w) du) sign, sign = d > 0 ? 1 : -1, g = 0 where !ok;   bottom0_diff = g, bottom1_diff = -g,
 *   each written only where its pointer is given.
 * NaN by 0 / 0, as in the reference (power_layer.cu:55-62): with p_eps == 0 and p none of 0, 1, 2 an element with d == 0 (not a masked
 * one) gets g = NaN -- that element only.  Likewise q_eps == 0 with q none of 0, 1, 2 at a pixel whose s is 0: every channel of that pixel.
 *
 * workspace: float[0] = loss, float[1] = normalize_coeff (kept on the device for the backward), then the per-workgroup partial sums.
 * The _multi forms run every LpqLoss layer of a net (1 .. 8) in one launch per direction, the weighted sum total = sum_k loss_weight[k]
 * loss[k] (float, list order) included; shapes = {N, C, H, W} per scale; per scale the bits of the single calls with top_diff =
 * loss_weight[k] * total_diff[0] (total_diff: a DEVICE scalar, NULL = 1).  bottoms1 / bottom1_diffs / bottom0_diffs may be NULL or hold NULL
 * entries.  sync: device memory, zero before the first call, left zero by every call, one per stream.  p, q, the epsilons and the flags
 * are per call.
 *
 * fn2_lpq_loss_sizes and fn2_lpq_loss_schedule_step are host-only.  _schedule_step: the index of the last of the n ascending `starts` that
 * is <= iter (a pure function of iter; the reference pops a queue and never steps back), -1 when there is none.
 * The other functions return FN2_OK or refuse on the host before any launch, writing nothing: FN2_ERR_INVALID_ARG a NULL blob, a
 * non-positive extent, a blob of 2^31 elements or more, a NaN p or q, a NaN or negative p_epsilon or q_epsilon, a scale count outside
 * 1 .. 8, a NULL sync; FN2_ERR_WORKSPACE a workspace that is NULL or too small. */
#pragma once
#include "flownet2_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* any out-pointer may be NULL; multi_workspace_bytes is for nscales scales (0 when nscales is outside 1 .. 8) */
int fn2_lpq_loss_sizes(int nscales, size_t* workspace_bytes, size_t* multi_workspace_bytes, size_t* sync_bytes);
int fn2_lpq_loss_schedule_step(int n, const int* starts, int iter);
/* loss_out: DEVICE float[1] or NULL */
int fn2_lpq_loss_forward(const float* bottom0, const float* bottom1, float* loss_out, int N, int C, int H, int W, float p, float q,
                         float p_epsilon, float q_epsilon, int l2_prescale_by_channels, int normalize_by_num_entries, void* workspace,
                         size_t workspace_bytes, void* stream);
int fn2_lpq_loss_backward(const float* bottom0, const float* bottom1, float top_diff, float* bottom0_diff, float* bottom1_diff, int N, int C,
                          int H, int W, float p, float q, float p_epsilon, float q_epsilon, int l2_prescale_by_channels,
                          int normalize_by_num_entries, void* workspace, size_t workspace_bytes, void* stream);
/* losses: DEVICE float[nscales] or NULL; total: DEVICE float[1] or NULL */
int fn2_lpq_loss_forward_multi(int nscales, const void* const* bottoms0, const void* const* bottoms1, const int* shapes,
                               const float* loss_weights, float p, float q, float p_epsilon, float q_epsilon, int l2_prescale_by_channels,
                               int normalize_by_num_entries, float* losses, float* total, void* workspace, size_t workspace_bytes, void* sync,
                               void* stream);
int fn2_lpq_loss_backward_multi(int nscales, const void* const* bottoms0, const void* const* bottoms1, void* const* bottom0_diffs,
                                void* const* bottom1_diffs, const int* shapes, const float* loss_weights, float p, float q, float p_epsilon,
                                float q_epsilon, int l2_prescale_by_channels, int normalize_by_num_entries, const float* total_diff,
                                void* workspace, size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
