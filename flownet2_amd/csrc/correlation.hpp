// Shared between correlation.hip (generic kernels, C ABI) and correlation_mfma.hip (fast path).
#pragma once
#include "fn2_common.hpp"

namespace fn2 {

struct CorrGeom {
  int N, C, H, W;
  int pad, K, md, s1, s2, kr;
  int topC, topH, topW, ngr, ngw;
  int type;
  // fused epilogue (fn2_correlation_forward_fused): the top blob may be a channel slice [top_c0, top_c0 + topC) of a blob with
  // top_ctot channels, and the in-place ReLU that follows the layer in the FlowNetC graph can be applied on the way out
  int top_ctot, top_c0, relu;
  float slope;
};

bool corr_fwd_mfma_supported(const CorrGeom& g);
int corr_fwd_mfma_launch(const CorrGeom& g, const float* b0, const float* b1, float* top, hipStream_t st);
// third-generation forward of the FlowNetC instance (correlation_units.hip): unit lists, loader wave; corr_fwd_pair serves what it does not take
bool corr_fwd_units_supported(const CorrGeom& g, const float* b0, const float* b1, const float* top);
int corr_fwd_units_launch(const CorrGeom& g, const float* b0, const float* b1, float* top, hipStream_t st);
int corr_fwd_units_plan_words(int N, int H, int W, int policy, unsigned* out, int max_words);
// the FlowNetC instance in split-bf16 arithmetic (correlation_bf16x3.hip; FN2_CONV_ARITH_BF16X3 beside FN2_CORR_ROUTE_OWN)
bool corr_bf16x3_geometry_ok(const fn2_corr_params* p, int N, int C, int H, int W);
int corr_bf16x3_launch(const CorrGeom& g, const float* b0, const float* b1, float* top, hipStream_t st);
bool corr_bwd_mfma_supported(const CorrGeom& g);
int corr_bwd_mfma_launch(const CorrGeom& g, int which, const float* other, const float* top_diff, float* out, hipStream_t st);
// both bottom diffs in ONE launch; FN2_ERR_UNSUPPORTED (no error text) where it does not apply
int corr_bwd_mfma_launch_both(const CorrGeom& g, const float* b0, const float* b1, const float* top_diff, float* d0, float* d1, hipStream_t st);


// Test / profiling hooks, set together by fn2_debug_set_correlation_impl (correlation.hip); each is defined beside the launch code that reads it.
extern int g_corr_force_dword;         // correlation_mfma.hip: corr_fwd_glds even where corr_fwd_pair applies
extern int g_corr_simd_plan;           // correlation_mfma.hip: 0 = corr_fwd_pair without the SIMD plan
extern int g_corr_ablation;            // correlation_mfma.hip: ablation bits of corr_fwd_glds (FN2_ABLATION builds)
extern unsigned long long* g_corr_dbg; // correlation_mfma.hip: per-workgroup trace buffer (FN2_ABLATION builds; fn2_debug_set_correlation_trace)
extern int g_corr_units;               // correlation_units.hip: 0 = corr_fwd_pair where both apply, 1 + policy = the unit kernel
extern int g_corr_units_lds;           // correlation_units.hip: extra dynamic LDS per workgroup, bytes
extern int g_corr_units_abl;           // correlation_units.hip: ablation bits of corr_fwd_units (FN2_ABLATION builds)
extern int g_corr1d_force_generic;     // correlation1d.hip: generic 1-D kernels
extern int g_corr1d_no_mfma;           // correlation1d.hip: the LDS-tiled VALU forward instead of the MFMA one
namespace bwd {
extern int g_corr_bwd_first_gen;       // correlation_bwd_mfma.hip: corr_bwd_mfma where the G-ring kernel applies
extern int g_corr_bwd_separate;        // correlation_bwd_mfma.hip: one launch per bottom where the merged launch applies
}  // namespace bwd

}  // namespace fn2
