// LpqLoss, the scheduled Lp/q loss, for gfx950:  loss = sum_(n,y,x) ( sum_c w (|d_c| + p_eps)^p + q_eps )^q / normalize_coeff.
//
// Replaces LpqLossLayer::Forward_gpu / Backward_gpu (reference: src/caffe/layers/lpq_loss_layer.cu:97-245, composition in
// lpq_loss_layer.cpp:84-143): an Eltwise, two Power layers, a 1x1 convolution, five element-wise kernels, two blocking cublasSdot and a
// host read of the loss per forward.  Here, as in l1loss.hip, the forward is ONE fused streaming pass (difference, NaN mask, |.|, p-power,
// channel sum, q-power, wave64 reduction -> LDS -> one fp64 partial per workgroup) plus a one-workgroup finalise; the loss and the
// normalisation coefficient stay on the device; the backward is one pass that recomputes the element-wise terms from the bottoms (no
// sign_ / mask_ blob).  The reduction order is fixed by the blob shape alone (no atomics on floats), so the bits repeat from run to run.
// All LpqLoss layers of a net run in one launch per direction (lpq_fwd_multi / lpq_bwd_multi), bit-identical per scale to the single calls.
//
// A thread owns one pixel, or four neighbouring pixels of a plane where H * W is a multiple of 4; those are read as one 16-byte load per
// channel where every blob pointer is 16-byte aligned and as four 4-byte loads otherwise -- the same values in the same order.
// Every operation is rounded on its own (fp contract off), so a float32 restatement op by op gives the bits where no powf runs.
//
// -Rpass-analysis=kernel-resource-usage (gfx950, -O3; each kernel holds the three load forms and both powf sites):
//   lpq_fwd_partial  VGPRs 44   SGPRs 73  LDS 64 B   occupancy 8     lpq_fwd_final  VGPRs 19  SGPRs 23  LDS 64 B  occupancy 8
//   lpq_bwd          VGPRs 46   SGPRs 79  LDS 0 B    occupancy 8
//   lpq_fwd_multi    VGPRs 44   SGPRs 71  LDS 72 B   occupancy 8     lpq_bwd_multi  VGPRs 47  SGPRs 75  LDS 0 B   occupancy 8
// no scratch in any of them.
#include "stream_reduce.hpp"
#include "../../include/flownet2_hip_lpq_loss.h"

#pragma clang fp contract(off)

namespace fn2 {

using namespace stream;

constexpr int kLpqMaxBlocks = 1024;
constexpr int kLpqMaxScales = 8;

// how a power is taken (PowerLayer::Forward_gpu, power_layer.cu:9-30) and differentiated (Backward_gpu :33-80), scale = 1
enum : int { kPowOne = 0 /* power 0 */, kPowIdentity = 1 /* power 1 */, kPowSquare = 2 /* power 2: powf forward, 2 x backward */, kPowGeneral = 3 };

struct LpqArgs {
  float p, q, p_eps, q_eps;
  int pmode, qmode;
  int prescale, normalize;
};

struct LpqBlob {
  const float* b0; const float* b1; float* d0; float* d1;
  float* ws; double* partial;
  int N, C, H, W;
  int quad;        // H * W % 4 == 0: four pixels per thread
  int vec;         // and every pointer 16-byte aligned: 16-byte loads / stores
  int blk0, nb;
  float loss_weight;
};

struct LpqMulti {
  int n;
  LpqBlob s[kLpqMaxScales];
  LpqArgs a;
  unsigned* sync;           // [kLpqMaxScales] arrival counters + [1] finished scales; zero between calls
  float* losses;            // [n] or null
  float* total;             // [1] or null
  const float* total_diff;  // backward: d(objective) / d(total), a device scalar (null: 1)
};

__device__ __forceinline__ float lpq_pow(float t, float power, int mode) {
  if (mode == kPowIdentity) return t;
  if (mode == kPowOne) return 1.f;
  return powf(t, power);                                       // caffe_gpu_powx, power_layer.cu:27-29 (power 2 included)
}

// d (t^power) / dt, t = x + shift
__device__ __forceinline__ float lpq_dpow(float t, float power, int mode) {
  if (mode == kPowIdentity) return 1.f;                        // power_layer.cu:40-41
  if (mode == kPowOne) return 0.f;                             // diff_scale == 0
  if (mode == kPowSquare) return 2.f * t;                      // :46-54 (2 x + 2 shift: the same bits)
  return power * (powf(t, power) / t);                         // :55-76 (shift == 0: t is x itself)
}

// d = b0 - b1 of V neighbouring pixels of one channel (Eltwise coeff +1, -1: lpq_loss_layer.cpp:87-97)
template <int V, bool VEC>
__device__ __forceinline__ void lpq_diff(const LpqBlob& s, size_t i, float (&d)[V]) {
  load<V, VEC>(s.b0 + i, d);
  if (s.b1) {
    float e[V];
    load<V, VEC>(s.b1 + i, e);
#pragma unroll
    for (int k = 0; k < V; ++k) d[k] = d[k] - e[k];
  }
}

// s = sum_c w (|d_c| + p_eps)^p of V pixels; cnt += their non-NaN entries
template <int V, bool VEC>
__device__ __forceinline__ void lpq_channel_sum(const LpqBlob& s, const LpqArgs& a, float wgt, size_t i0, size_t hw, float (&acc)[V], int& cnt) {
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
  for (int c = 0; c < s.C; ++c) {
    float d[V];
    lpq_diff<V, VEC>(s, i0 + c * hw, d);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const bool ok = (d[k] == d[k]);                          // FindNotNaNs cu:33-40
      cnt += ok;
      const float dd = ok ? d[k] : 0.f;                        // KillMasked cu:53-60, :165-169
      const float t = fabsf(dd) + a.p_eps;                     // d * sign cu:173-186; Power shift power_layer.cu:24-26
      acc[k] = acc[k] + wgt * lpq_pow(t, a.p, a.pmode);        // 1x1 convolution, constant filler, zero bias: cpp:112-129
    }
  }
}

// partial[2*b] = sum of the per-pixel terms, partial[2*b+1] = number of non-NaN entries.  (bid, nblk): this workgroup's index and the
// number of workgroups of ITS blob pair, so that the summation order is a function of the blob shape only (as l1_partial_body).
template <int V, bool VEC>
__device__ __forceinline__ void lpq_partial_body(const LpqBlob& s, const LpqArgs& a, unsigned bid, unsigned nblk, double* lds) {
  const size_t hw = (size_t)s.H * s.W;
  const long long per_sample = (long long)(hw / V);
  const long long total = (long long)s.N * per_sample;
  const float wgt = a.prescale ? 1.f / (float)s.C : 1.f;      // cpp:120-127
  double dot = 0.0, nvalid = 0.0;
  for (long long u = bid * (long long)blockDim.x + threadIdx.x; u < total; u += (long long)nblk * blockDim.x) {
    const size_t n = u / per_sample, r = (size_t)(u % per_sample) * V;
    float acc[V];
    int cnt = 0;
    lpq_channel_sum<V, VEC>(s, a, wgt, n * s.C * hw + r, hw, acc, cnt);
#pragma unroll
    for (int k = 0; k < V; ++k) dot += (double)lpq_pow(acc[k] + a.q_eps, a.q, a.qmode);     // Power q cu:191, dot with ones cu:194
    nvalid += (double)cnt;
  }
  block_sum2(dot, nvalid, lds);
  if (threadIdx.x == 0) {
    s.partial[2 * bid] = dot;
    s.partial[2 * bid + 1] = nvalid;
  }
}

__device__ __forceinline__ void lpq_partial(const LpqBlob& s, const LpqArgs& a, unsigned bid, unsigned nblk, double* lds) {
  if (!s.quad) lpq_partial_body<1, false>(s, a, bid, nblk, lds);
  else if (s.vec) lpq_partial_body<4, true>(s, a, bid, nblk, lds);
  else lpq_partial_body<4, false>(s, a, bid, nblk, lds);
}

// ws[0] = loss, ws[1] = normalize_coeff; loss_out[0] = loss.
__device__ __forceinline__ void lpq_final_body(const LpqBlob& s, const LpqArgs& a, float* __restrict__ loss_out, double* lds) {
  double dot = 0.0, nvalid = 0.0;
  for (int b = threadIdx.x; b < s.nb; b += blockDim.x) {
    dot += s.partial[2 * b];
    nvalid += s.partial[2 * b + 1];
  }
  block_sum2(dot, nvalid, lds);
  if (threadIdx.x == 0) {
    const float norm = a.normalize ? (float)nvalid / (float)s.C : (float)s.N;      // cu:157-162
    const float loss = (float)(dot / (double)norm);                                // cu:196
    s.ws[0] = loss;
    s.ws[1] = norm;
    if (loss_out) loss_out[0] = loss;
  }
}

template <int V, bool VEC>
__device__ __forceinline__ void lpq_bwd_body(const LpqBlob& s, const LpqArgs& a, float top_diff, unsigned bid, unsigned nblk) {
  const size_t hw = (size_t)s.H * s.W;
  const long long per_sample = (long long)(hw / V);
  const long long total = (long long)s.N * per_sample;
  const float wgt = a.prescale ? 1.f / (float)s.C : 1.f;
  const float alpha = top_diff / s.ws[1];                      // cu:215
  for (long long u = bid * (long long)blockDim.x + threadIdx.x; u < total; u += (long long)nblk * blockDim.x) {
    const size_t n = u / per_sample, r = (size_t)(u % per_sample) * V;
    const size_t i0 = n * s.C * hw + r;
    float acc[V], coef[V];
    int cnt = 0;
    lpq_channel_sum<V, VEC>(s, a, wgt, i0, hw, acc, cnt);
#pragma unroll
    for (int k = 0; k < V; ++k)                                // q_output diff = alpha cu:218; Power q backward; convolution backward
      coef[k] = (alpha * lpq_dpow(acc[k] + a.q_eps, a.q, a.qmode)) * wgt;
    for (int c = 0; c < s.C; ++c) {
      const size_t i = i0 + c * hw;
      float d[V], g[V];
      lpq_diff<V, VEC>(s, i, d);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const bool ok = (d[k] == d[k]);
        const float dd = ok ? d[k] : 0.f;
        const float sign = dd > 0.f ? 1.f : -1.f;              // ComputeSign cu:21-28
        const float t = fabsf(dd) + a.p_eps;
        const float gk = (coef[k] * lpq_dpow(t, a.p, a.pmode)) * sign;     // Power p backward; EltwiseMult cu:225-231
        g[k] = ok ? gk : 0.f;                                  // KillMasked cu:233-237
      }
      if (s.d0) store<V, VEC>(s.d0 + i, g);                // Eltwise backward, coeff +1
      if (s.d1) {
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = -g[k];              // coeff -1
        store<V, VEC>(s.d1 + i, g);
      }
    }
  }
}

__device__ __forceinline__ void lpq_bwd_dispatch(const LpqBlob& s, const LpqArgs& a, float top_diff, unsigned bid, unsigned nblk) {
  if (!s.quad) lpq_bwd_body<1, false>(s, a, top_diff, bid, nblk);
  else if (s.vec) lpq_bwd_body<4, true>(s, a, top_diff, bid, nblk);
  else lpq_bwd_body<4, false>(s, a, top_diff, bid, nblk);
}

__global__ void __launch_bounds__(kThreads) lpq_fwd_partial(LpqBlob s, LpqArgs a) {
  __shared__ double lds[8];
  lpq_partial(s, a, blockIdx.x, gridDim.x, lds);
}

__global__ void __launch_bounds__(kThreads) lpq_fwd_final(LpqBlob s, LpqArgs a, float* __restrict__ loss_out) {
  __shared__ double lds[8];
  lpq_final_body(s, a, loss_out, lds);
}

__global__ void __launch_bounds__(kThreads) lpq_bwd(LpqBlob s, LpqArgs a, float top_diff) {
  lpq_bwd_dispatch(s, a, top_diff, blockIdx.x, gridDim.x);
}

__device__ __forceinline__ int lpq_scale_of(const LpqMulti& m) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < kLpqMaxScales; ++i) s += (i < m.n && (int)blockIdx.x >= m.s[i].blk0) ? 1 : 0;
  return s;
}

// The protocol of l1loss_fwd_multi: a workgroup belongs to one scale and runs that scale's body with the (bid, nblk) of its own launch;
// the workgroup that arrives LAST at its scale's counter (release / acquire around an integer atomic) runs the finalise body; the scale
// that finishes last adds up total = sum_s loss_weight[s] * loss[s] in scale order, each product and sum rounded to float.  The
// counters are left at zero for the next call.
__global__ void __launch_bounds__(kThreads) lpq_fwd_multi(LpqMulti m) {
  __shared__ double lds[8];
  __shared__ int s_last;
  const int si = lpq_scale_of(m);
  const LpqBlob& sc = m.s[si];
  lpq_partial(sc, m.a, blockIdx.x - sc.blk0, sc.nb, lds);
  if (threadIdx.x == 0) {
    __threadfence();                                                  // release: this workgroup's partial before its arrival
    s_last = atomicAdd(&m.sync[si], 1u) == (unsigned)(sc.nb - 1);
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();                                                    // acquire: the other workgroups' partials
  lpq_final_body(sc, m.a, m.losses ? m.losses + si : nullptr, lds);
  if (threadIdx.x == 0) {
    m.sync[si] = 0u;
    __threadfence();
    if (atomicAdd(&m.sync[kLpqMaxScales], 1u) == (unsigned)(m.n - 1)) {
      __threadfence();
      float total = 0.f;
      for (int i = 0; i < m.n; ++i) {
        const float l = *reinterpret_cast<volatile float*>(m.s[i].ws);
        total = total + m.s[i].loss_weight * l;
      }
      if (m.total) m.total[0] = total;
      m.sync[kLpqMaxScales] = 0u;
    }
  }
}

__global__ void __launch_bounds__(kThreads) lpq_bwd_multi(LpqMulti m) {
  const int si = lpq_scale_of(m);
  const LpqBlob& sc = m.s[si];
  const float g = m.total_diff ? m.total_diff[0] : 1.f;
  lpq_bwd_dispatch(sc, m.a, sc.loss_weight * g, blockIdx.x - sc.blk0, sc.nb);      // top_diff of the layer = loss_weight x d(total)
}

static int lpq_pow_mode(float power) { return power == 0.f ? kPowOne : power == 1.f ? kPowIdentity : power == 2.f ? kPowSquare : kPowGeneral; }

static int lpq_args(const char* what, float p, float q, float p_eps, float q_eps, int prescale, int normalize, LpqArgs* a) {
  if (p != p || q != q) return fail(FN2_ERR_INVALID_ARG, "%s: p or q is NaN", what);
  if (!(p_eps >= 0.f) || !(q_eps >= 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: p_epsilon = %g, q_epsilon = %g (need >= 0)", what, p_eps, q_eps);
  a->p = p; a->q = q; a->p_eps = p_eps; a->q_eps = q_eps;
  a->pmode = lpq_pow_mode(p); a->qmode = lpq_pow_mode(q);
  a->prescale = prescale != 0; a->normalize = normalize != 0;
  return FN2_OK;
}

static size_t lpq_ws_bytes() { return 64 + sizeof(double) * 2 * kLpqMaxBlocks; }   // float[0] = loss, float[1] = normalize_coeff, pad to 64 B, partial[2 * kLpqMaxBlocks]

// One blob pair: shape and pointer checks, the launch geometry (by the shape alone) and the load form.
static int lpq_blob(const char* what, int scale, const float* b0, const float* b1, float* d0, float* d1, bool backward, int N, int C, int H,
                    int W, void* ws, LpqBlob* s) {
  if (N < 1 || C < 1 || H < 1 || W < 1) return fail(FN2_ERR_INVALID_ARG, "%s: bad shape [%d,%d,%d,%d] (scale %d)", what, N, C, H, W, scale);
  const long long count = (long long)N * C * H * W;
  if (count >= (1LL << 31)) return fail(FN2_ERR_INVALID_ARG, "%s: blob of %lld elements (2^31 or more) (scale %d)", what, count, scale);
  if (!b0) return fail(FN2_ERR_INVALID_ARG, "%s: bottom[0] == NULL (scale %d)", what, scale);
  if (!b1) d1 = nullptr;
  if (backward && !d0 && !d1) return fail(FN2_ERR_INVALID_ARG, "%s: no bottom diff to write (scale %d)", what, scale);
  s->b0 = b0; s->b1 = b1; s->d0 = d0; s->d1 = d1;
  s->ws = reinterpret_cast<float*>(ws);
  s->partial = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + 64);
  s->N = N; s->C = C; s->H = H; s->W = W;
  const long long hw = (long long)H * W;
  s->quad = (hw % 4) == 0;
  s->vec = s->quad && aligned16(b0) && aligned16(b1) && aligned16(d0) && aligned16(d1);
  s->nb = (int)blocks_for((long long)N * (hw / (s->quad ? 4 : 1)), kThreads, kLpqMaxBlocks);
  s->blk0 = 0;
  s->loss_weight = 1.f;
  return FN2_OK;
}

static int lpq_multi_fill(const char* what, int nscales, const void* const* bottoms0, const void* const* bottoms1, void* const* diffs0,
                          void* const* diffs1, const int* shapes, const float* loss_weights, bool backward, void* workspace,
                          size_t workspace_bytes, LpqMulti* m, unsigned* total_blocks) {
  if (nscales < 1 || nscales > kLpqMaxScales) return fail(FN2_ERR_INVALID_ARG, "%s: 1 .. %d scales (got %d)", what, kLpqMaxScales, nscales);
  if (!bottoms0 || !shapes || !loss_weights) return fail(FN2_ERR_INVALID_ARG, "%s: bottoms0, shapes or loss_weights == NULL", what);
  if (!workspace || workspace_bytes < (size_t)nscales * lpq_ws_bytes())
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, (size_t)nscales * lpq_ws_bytes());
  m->n = nscales;
  int blk = 0;
  for (int i = 0; i < nscales; ++i) {
    LpqBlob& sc = m->s[i];
    int rc = lpq_blob(what, i, reinterpret_cast<const float*>(bottoms0[i]), bottoms1 ? reinterpret_cast<const float*>(bottoms1[i]) : nullptr,
                      diffs0 ? reinterpret_cast<float*>(diffs0[i]) : nullptr, diffs1 ? reinterpret_cast<float*>(diffs1[i]) : nullptr, backward,
                      shapes[4 * i], shapes[4 * i + 1], shapes[4 * i + 2], shapes[4 * i + 3],
                      reinterpret_cast<char*>(workspace) + (size_t)i * lpq_ws_bytes(), &sc);
    if (rc) return rc;
    sc.blk0 = blk;
    sc.loss_weight = loss_weights[i];
    blk += sc.nb;
  }
  *total_blocks = (unsigned)blk;
  return FN2_OK;
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_lpq_loss_sizes(int nscales, size_t* workspace_bytes, size_t* multi_workspace_bytes, size_t* sync_bytes) {
  if (workspace_bytes) *workspace_bytes = lpq_ws_bytes();
  if (multi_workspace_bytes) *multi_workspace_bytes = (nscales >= 1 && nscales <= kLpqMaxScales) ? (size_t)nscales * lpq_ws_bytes() : 0;
  if (sync_bytes) *sync_bytes = sizeof(unsigned) * (kLpqMaxScales + 1 + 7);
  return FN2_OK;
}

FN2_API int fn2_lpq_loss_schedule_step(int n, const int* starts, int iter) {
  int step = -1;
  for (int i = 0; starts && i < n; ++i)
    if (starts[i] <= iter) step = i;
  return step;
}

FN2_API int fn2_lpq_loss_forward(const float* bottom0, const float* bottom1, float* loss_out, int N, int C, int H, int W, float p, float q,
                                 float p_epsilon, float q_epsilon, int l2_prescale_by_channels, int normalize_by_num_entries,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  LpqArgs a;
  LpqBlob s;
  int rc = lpq_args("lpq_loss_forward", p, q, p_epsilon, q_epsilon, l2_prescale_by_channels, normalize_by_num_entries, &a);
  if (rc) return rc;
  rc = lpq_blob("lpq_loss_forward", 0, bottom0, bottom1, nullptr, nullptr, false, N, C, H, W, workspace, &s);
  if (rc) return rc;
  if (!workspace || workspace_bytes < lpq_ws_bytes())
    return fail(FN2_ERR_WORKSPACE, "lpq_loss_forward: workspace too small (%zu < %zu)", workspace ? workspace_bytes : (size_t)0, lpq_ws_bytes());
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(lpq_fwd_partial, dim3(s.nb), dim3(kThreads), 0, st, s, a);
  hipLaunchKernelGGL(lpq_fwd_final, dim3(1), dim3(kThreads), 0, st, s, a, loss_out);
  return check_launch("lpq_loss_forward");
}

FN2_API int fn2_lpq_loss_backward(const float* bottom0, const float* bottom1, float top_diff, float* bottom0_diff, float* bottom1_diff, int N,
                                  int C, int H, int W, float p, float q, float p_epsilon, float q_epsilon, int l2_prescale_by_channels,
                                  int normalize_by_num_entries, void* workspace, size_t workspace_bytes, void* stream) {
  LpqArgs a;
  LpqBlob s;
  int rc = lpq_args("lpq_loss_backward", p, q, p_epsilon, q_epsilon, l2_prescale_by_channels, normalize_by_num_entries, &a);
  if (rc) return rc;
  rc = lpq_blob("lpq_loss_backward", 0, bottom0, bottom1, bottom0_diff, bottom1_diff, true, N, C, H, W, workspace, &s);
  if (rc) return rc;
  if (!workspace || workspace_bytes < lpq_ws_bytes())
    return fail(FN2_ERR_WORKSPACE, "lpq_loss_backward: workspace too small (%zu < %zu)", workspace ? workspace_bytes : (size_t)0, lpq_ws_bytes());
  hipLaunchKernelGGL(lpq_bwd, dim3(s.nb), dim3(kThreads), 0, as_stream(stream), s, a, top_diff);
  return check_launch("lpq_loss_backward");
}

FN2_API int fn2_lpq_loss_forward_multi(int nscales, const void* const* bottoms0, const void* const* bottoms1, const int* shapes,
                                       const float* loss_weights, float p, float q, float p_epsilon, float q_epsilon,
                                       int l2_prescale_by_channels, int normalize_by_num_entries, float* losses, float* total, void* workspace,
                                       size_t workspace_bytes, void* sync, void* stream) {
  LpqMulti m{};
  unsigned blocks = 0;
  int rc = lpq_args("lpq_loss_forward_multi", p, q, p_epsilon, q_epsilon, l2_prescale_by_channels, normalize_by_num_entries, &m.a);
  if (rc) return rc;
  rc = lpq_multi_fill("lpq_loss_forward_multi", nscales, bottoms0, bottoms1, nullptr, nullptr, shapes, loss_weights, false, workspace,
                      workspace_bytes, &m, &blocks);
  if (rc) return rc;
  if (!sync) return fail(FN2_ERR_INVALID_ARG, "lpq_loss_forward_multi: sync == NULL (fn2_lpq_loss_sizes' sync bytes, zero, left zero by every call)");
  m.sync = reinterpret_cast<unsigned*>(sync);
  m.losses = losses; m.total = total; m.total_diff = nullptr;
  hipLaunchKernelGGL(lpq_fwd_multi, dim3(blocks), dim3(kThreads), 0, as_stream(stream), m);
  return check_launch("lpq_loss_forward_multi");
}

FN2_API int fn2_lpq_loss_backward_multi(int nscales, const void* const* bottoms0, const void* const* bottoms1, void* const* bottom0_diffs,
                                        void* const* bottom1_diffs, const int* shapes, const float* loss_weights, float p, float q,
                                        float p_epsilon, float q_epsilon, int l2_prescale_by_channels, int normalize_by_num_entries,
                                        const float* total_diff, void* workspace, size_t workspace_bytes, void* stream) {
  LpqMulti m{};
  unsigned blocks = 0;
  int rc = lpq_args("lpq_loss_backward_multi", p, q, p_epsilon, q_epsilon, l2_prescale_by_channels, normalize_by_num_entries, &m.a);
  if (rc) return rc;
  rc = lpq_multi_fill("lpq_loss_backward_multi", nscales, bottoms0, bottoms1, bottom0_diffs, bottom1_diffs, shapes, loss_weights, true,
                      workspace, workspace_bytes, &m, &blocks);
  if (rc) return rc;
  m.sync = nullptr; m.losses = nullptr; m.total = nullptr; m.total_diff = total_diff;
  hipLaunchKernelGGL(lpq_bwd_multi, dim3(blocks), dim3(kThreads), 0, as_stream(stream), m);
  return check_launch("lpq_loss_backward_multi");
}
