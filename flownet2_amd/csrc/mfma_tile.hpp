// Building blocks shared by the MFMA tile kernels (conv_mfma, tconv_mfma, conv_plane, conv_wino, conv_wgrad; the correlation and
// stem kernels take the primitives only): vector types, the LDS-DMA window of a workgroup tile, the packed-weight stream, the XCD
// task remap, the row epilogue, and on the host the dynamic-LDS attribute, the launch tail, the argument checks and the variant picker.
// Everything on the device side is a __device__ __forceinline__ FUNCTION, never a lambda: the host pass of a __global__ template
// cannot see amdgcn builtins inside a lambda body.
#pragma once

#include "autotune.hpp"
#include "fn2_common.hpp"

namespace fn2 {
namespace mfma {

// ------------------------------------------------------------------------------------------------ primitives
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using lds_ptr_t = __attribute__((address_space(3))) void*;

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
constexpr int up_mod(int v, int r, int m) { return v + ((r - v % m) + m) % m; }   // smallest >= v with == r (mod m)

constexpr unsigned kOOB = 0x7ffffff0u;        // a byte offset beyond any supported blob: the lane's load comes back 0.0f = the zero padding
constexpr int kRsrcWord3 = 0x00020000;        // last word of a raw buffer resource (gfx9: 32-bit elements, range-checked)

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// raw buffer resource over channels [c0, c0 + C) of sample n of an NCHW blob with ctot channels and planes of `plane` floats
__device__ __forceinline__ __amdgpu_buffer_rsrc_t nchw_rsrc(const float* blob, int n, int ctot, int c0, int C, size_t plane) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(blob + ((size_t)n * ctot + c0) * plane), 0, (unsigned)(4u * C * plane), kRsrcWord3);
}

// the weight operand of a wave for one k-step: MW 16-channel groups -> one global_load_dwordx{MW} per lane
template <int MW> struct WVec;
template <> struct WVec<1> { using T = float; };
template <> struct WVec<2> { using T = f32x2; };
template <> struct WVec<4> { using T = f32x4; };

template <int MW>
__device__ __forceinline__ float wget(const typename WVec<MW>::T& v, int j) {
  if constexpr (MW == 1) return v; else return v[j];
}

// ------------------------------------------------------------------------------------------------ window geometry
// LDS geometry of the input window of a workgroup tile: WR rows x WC columns per channel, CQ channel quads per chunk, staged by
// NW waves in natural [channel][row][column] order.  RS == 4 (mod 16) and CS == 16 (mod 32) make the stride-1 operand reads
// conflict-free (stride 2: 2-way, the odd banks idle).
template <int WR_, int WC_, int CQ_, int NW_>
struct Window {
  static constexpr int WR = WR_, WC = WC_;
  static constexpr int RS = up_mod(cdiv(WC, 4) * 4, 4, 16);          // row stride (dwords)
  static constexpr int CS = up_mod(WR * RS, 16, 32);                 // channel stride
  static constexpr int SLOTS_C = CS / 4;                             // 16-byte slots per channel
  static constexpr int SLOTS = 4 * CQ_ * SLOTS_C;                    // per chunk
  static constexpr int NRUN = cdiv(SLOTS, 64);                       // 1 KiB LDS-DMA runs per chunk
  static constexpr int RPW = cdiv(NRUN, NW_);                        // runs per wave
  static constexpr int BUF = NRUN * 256;                             // dwords per window buffer (whole runs)
};

// depth of the weight-operand ring for chunks of KSC k-steps (the ring phase must repeat per chunk)
constexpr int ring_depth(int KSC) { return (KSC % 6 == 0) ? 6 : (KSC % 5 == 0) ? 5 : (KSC % 7 == 0) ? 7 : (KSC % 4 == 0) ? 4 : 3; }

// LDS-DMA plan of a window whose first row / column is input row y_first / column x_first: run r = i * NW + wave, slot
// s = 64 r + lane -> (channel, window row, group of 4 columns) -> the lane's byte offset in the sample, kOOB outside the image
template <class K>
__device__ __forceinline__ void window_plan(unsigned (&voff)[K::RPW], int wave, int lane, int y_first, int x_first, int Hin, int Win, size_t plane) {
#pragma unroll
  for (int i = 0; i < K::RPW; ++i) {
    const int s = (i * K::NW + wave) * 64 + lane;
    voff[i] = kOOB;
    if (s < K::SLOTS) {
      const int c = s / K::SLOTS_C, rem = s % K::SLOTS_C;
      const int row = rem / (K::RS / 4), gq = rem % (K::RS / 4);
      const int yi = y_first + row, xi = x_first + 4 * gq;
      if (row < K::WR && 4 * gq < K::WC && yi >= 0 && yi < Hin && xi >= 0 && xi < Win)
        voff[i] = 4u * (unsigned)(c * plane + (size_t)yi * Win + xi);
    }
  }
}

// LDS-DMA of one chunk's window: run r = i * NW + wave -> 1 KiB at dst + 1024 r
template <class K>
__device__ __forceinline__ void stage_chunk(__amdgpu_buffer_rsrc_t rs, const unsigned (&voff)[K::RPW], unsigned dst, int wave, unsigned soff) {
#pragma unroll
  for (int i = 0; i < K::RPW; ++i) {
    const int r = i * K::NW + wave;
    if (r < K::NRUN)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(uintptr_t)(dst + 1024u * (unsigned)r), 16, voff[i], soff, 0, 0);
  }
}

// stage_chunk of the window `chunk` chunks further on (chunk_bytes: the planes of one chunk): the in-image lanes of the plan advance, the
// kOOB lanes stay out of range (as do channels >= Cin: out of range = 0).  A function object over the kernel's own values with a plain
// operator(), the one exception to the rule above: as a __forceinline__ function, expanded ahead of the optimiser, it changes the scalar
// register allocation of the kernels that use it (profiles/bf16x3_toolkit.md).  It calls no amdgcn builtin itself.
template <class K>
struct ChunkStage {
  const __amdgpu_buffer_rsrc_t& rs; const unsigned (&voff)[K::RPW]; const unsigned& chunk_bytes; const unsigned& dst; const int& wave;
  __device__ void operator()(int chunk) const {
    unsigned vc[K::RPW];
#pragma unroll
    for (int i = 0; i < K::RPW; ++i) vc[i] = voff[i] == kOOB ? kOOB : voff[i] + (unsigned)chunk * chunk_bytes;
    stage_chunk<K>(rs, vc, dst, wave, 0u);
  }
};

// ------------------------------------------------------------------------------------------------ weight stream
// packed weights [Cout/64][ksteps][64 lanes][4] (fn2_conv_mfma_pack_weights): this lane's element of k-step 0 for the wave whose
// first 16-channel group is cg0; k-step ks is 256 floats further on
__device__ __forceinline__ const float* weight_lane(const float* wp, int cg0, int ksteps, int lane) {
  return wp + ((size_t)(cg0 / 4) * ksteps * 64 + lane) * 4 + (cg0 % 4);
}

template <int MW>
__device__ __forceinline__ typename WVec<MW>::T weight_load(const float* wl, int ks) {
  return *reinterpret_cast<const typename WVec<MW>::T*>(wl + (size_t)ks * 256);
}

// The weight ring with the kernel's OWN waits (conv_mfma.hip).  LDS-DMA window loads and the weight loads share the one vmcnt counter and
// loads retire in order.  Left to the compiler, the ring's plain loads get re-clustered or waited for with vmcnt(0 .. 1) right behind the
// window DMA of the next chunk, which drains that DMA a k-step after its issue instead of leaving it the ring's depth in k-steps to arrive
// (profiles/NOTES_window_lead.md).  So the ring's loads are asm volatile (the compiler neither counts nor moves them) and every use waits by hand:
//   weight_fetch       a k-step's operand of the wave: uniform `base` (SGPR pair) + the lane's byte offset
//   ring_wait          s_waitcnt vmcnt(n), n = the loads YOUNGER than the operand that may stay in flight (a smaller n is always
//                      correct, only slower).  n must fold to a constant (an unrolled loop's counter does; it does not compile otherwise)
//   ring_wait_either   one of two such waits, chosen at run time (the last chunk has fewer loads behind the operand)
//   ring_wait_if_le    a further, tighter wait, taken or not at run time
//   weight_landed      ties the operand to the waits in front of it: the MFMAs that read it stay behind them.  The waits themselves name
//                      no register and branch inside one asm block: the k loop stays one basic block for the compiler, which therefore
//                      never copies an operand that is still in flight on the way into a branch.
// A kernel that uses these leaves no ring load in flight when it reaches code whose registers the compiler allocates on its own.
template <int MW>
__device__ __forceinline__ typename WVec<MW>::T weight_fetch(const float* base, unsigned lane_bytes) {
  typename WVec<MW>::T w;
  if constexpr (MW == 1) asm volatile("global_load_dword %0, %1, %2" : "=v"(w) : "v"(lane_bytes), "s"(base));
  else if constexpr (MW == 2) asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(w) : "v"(lane_bytes), "s"(base));
  else asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(w) : "v"(lane_bytes), "s"(base));
  return w;
}

template <class T>
__device__ __forceinline__ void weight_landed(T& w) { asm volatile("" : "+v"(w)); }

constexpr int vmcnt_clamp(int n) { return n < 63 ? n : 63; }      // the counter has 6 bits

__device__ __forceinline__ void ring_wait(int n) { asm volatile("s_waitcnt vmcnt(%0)" ::"i"(vmcnt_clamp(n))); }

// vmcnt(n_short) when s < below, else vmcnt(n_full).  With s = the chunks still to come and below = 1: the last chunk, which has fewer
// loads behind the operand.  below must fold to a constant.
__device__ __forceinline__ void ring_wait_either(int s, int below, int n_short, int n_full) {
  asm volatile(
      "s_cmp_lt_u32 %0, %1\n\t"
      "s_cbranch_scc1 .Lrwt_%=\n\t"
      "s_waitcnt vmcnt(%3)\n\t"
      "s_branch .Lrwe_%=\n"
      ".Lrwt_%=:\n\t"
      "s_waitcnt vmcnt(%2)\n"
      ".Lrwe_%=:"
      :
      : "s"(s), "i"(below), "i"(vmcnt_clamp(n_short)), "i"(vmcnt_clamp(n_full))
      : "scc");
}

// vmcnt(n) when s <= most, else nothing: behind a ring_wait, the tighter wait of a chunk that stops at a run-time k-step (conv_mfma.hip)
__device__ __forceinline__ void ring_wait_if_le(int s, int most, int n) {
  asm volatile(
      "s_cmp_gt_u32 %0, %1\n\t"
      "s_cbranch_scc1 .Lrwl_%=\n\t"
      "s_waitcnt vmcnt(%2)\n"
      ".Lrwl_%=:"
      :
      : "s"(s), "i"(most), "i"(vmcnt_clamp(n))
      : "scc");
}

// weight_fetch of k-step i of the NEXT chunk unless that chunk has no such k-step: `ahead` = the k-steps it executes, 0 behind the last
// chunk, which fetches nothing beyond its own k-steps.  (i = 0 with ahead = the chunks still to come: "unless this is the last chunk".)
// i must fold to a constant, as ring_wait's n.
template <int MW>
__device__ __forceinline__ typename WVec<MW>::T weight_fetch_unless_last(int ahead, int i, const float* base, unsigned lane_bytes) {
  typename WVec<MW>::T w;
#define FN2_FETCH_UNLESS(INSN) \
  asm volatile("s_cmp_le_u32 %3, %4\n\ts_cbranch_scc1 .Lwfs_%=\n\t" INSN " %0, %1, %2\n.Lwfs_%=:" \
               : "=v"(w) : "v"(lane_bytes), "s"(base), "s"(ahead), "i"(i) : "scc")
  if constexpr (MW == 1) FN2_FETCH_UNLESS("global_load_dword");
  else if constexpr (MW == 2) FN2_FETCH_UNLESS("global_load_dwordx2");
  else FN2_FETCH_UNLESS("global_load_dwordx4");
#undef FN2_FETCH_UNLESS
  return w;
}

// ------------------------------------------------------------------------------------------------ XCD task remap
// Block b runs on XCD b % 8.  The task list is cut into 8 contiguous ranges, one per XCD, so that neighbouring tasks (which share
// an input window) run on one XCD, whose L2 serves the re-reads.  false: this block has no task.
__device__ __forceinline__ bool xcd_task(unsigned block, unsigned total, unsigned& task) {
  const unsigned per_xcd = (total + 7) / 8;
  task = (block % 8) * per_xcd + block / 8;
  return !(block / 8 >= per_xcd || task >= total);
}

// ------------------------------------------------------------------------------------------------ row epilogue
__device__ __forceinline__ f32x4 bias_relu4(f32x4 v, float bias, int relu, float slope) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float s = v[r] + bias;
    if (relu) s = s > 0.f ? s : s * slope;
    v[r] = s;
  }
  return v;
}

// v -> orow[x .. x + 3]: one 16-byte store, scalar stores where the row ends inside the four
__device__ __forceinline__ void store4(float* orow, int x, int Wout, f32x4 v) {
  if (x + 3 < Wout) *reinterpret_cast<f32x4*>(orow + x) = v;
  else {
#pragma unroll
    for (int r = 0; r < 4; ++r) if (x + r < Wout) orow[x + r] = v[r];
  }
}

__device__ __forceinline__ void store_row4(float* orow, int x, int Wout, f32x4 v, float bias, int relu, float slope) {
  store4(orow, x, Wout, bias_relu4(v, bias, relu, slope));
}

// ------------------------------------------------------------------------------------------------ host side
// raises the kernel's dynamic LDS limit on its first launch (per kernel instantiation)
template <auto Kernel>
inline void set_dynamic_lds_once(int bytes) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    attr_set = true;
  }
}

// The launch tail of a tile kernel whose blocks find their task with xcd_task: `tiles` workgroups -> a.total, the dynamic-LDS
// attribute, a grid of whole groups of 8 blocks (one per XCD), the launch check.  what: the family's name in the refusal; checked: the
// name check_launch reports.
template <auto Kernel, class Args>
int launch_tiles(Args& a, long long tiles, int threads, int lds_bytes, const char* what, const char* checked, hipStream_t st) {
  if (tiles > 0x3fffff00ll) return fail(FN2_ERR_UNSUPPORTED, "%s: grid too large", what);
  a.total = (unsigned)tiles;
  set_dynamic_lds_once<Kernel>(lds_bytes);
  hipLaunchKernelGGL(Kernel, dim3(8 * ((a.total + 7) / 8)), dim3(threads), lds_bytes, st, a);
  return check_launch(checked);
}

// The argument checks every forward entry point makes after its batch check: blobs present, the family's own geometry check
// (geometry() returns FN2_OK or its fail(...)), channel slices inside their blobs, 16-byte alignment.
template <class Geometry>
int check_conv_args(const char* what, const float* bottom, const float* packed, const float* top, int Cin, int bottom_channels, int bottom_c0,
                    int Cout, int top_channels, int top_c0, Geometry geometry) {
  if (!bottom || !packed || !top) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (const int rc = geometry()) return rc;
  if (bottom_c0 < 0 || bottom_c0 + Cin > bottom_channels || top_c0 < 0 || top_c0 + Cout > top_channels)
    return fail(FN2_ERR_INVALID_ARG, "%s: channel slice outside the blob", what);
  if (((reinterpret_cast<uintptr_t>(bottom) | reinterpret_cast<uintptr_t>(top) | reinterpret_cast<uintptr_t>(packed)) & 15) != 0)
    return fail(FN2_ERR_UNSUPPORTED, "%s: blobs must be 16-byte aligned", what);
  return FN2_OK;
}

// Picks the tile variant of one call: the forced one (a debug knob), else the autotuned one, else the cheapest by the family's
// cost model.  All candidates of a family write the same bits.
//   applies(i)      variant i takes this problem
//   cost(i, tail)   the family's cost model (measurements: they stay with the family)
//   run(i, tail)    launches variant i
//   has_tail(i)     split_tail only: variant i has a split-tail launch.  The autotune candidates are then 2 i / 2 i + 1 = plain /
//                   split-tail launch of variant i (the latter only where the cost model sees a gain: cost < 1e29), and a forced
//                   value >= 1000 asks for the split-tail launch of variant forced % 1000.
struct Pick { int variant = -1; bool tail = false; };

template <class Applies, class Cost, class Run, class HasTail>
int pick_variant(Pick& p, const char* what, int forced, int nvariants, bool split_tail, TuneCache& cache, const TuneKey& key, hipStream_t st,
                 Applies applies, Cost cost, Run run, HasTail has_tail) {
  p = Pick{};
  if (forced >= 0) {
    p.tail = split_tail && forced >= 1000;
    p.variant = split_tail ? forced % 1000 : forced;
    if (p.variant >= nvariants || !applies(p.variant) || (p.tail && !has_tail(p.variant)))
      return fail(FN2_ERR_UNSUPPORTED, "%s: forced variant %d does not apply", what, forced);
    return FN2_OK;
  }
  int picked = -1;
  if (autotune_enabled(st)) {
    auto usable = [&](int c) -> bool {
      const int i = split_tail ? c / 2 : c;
      return applies(i) && (!(split_tail && (c & 1)) || (has_tail(i) && cost(i, true) < 1e29));
    };
    picked = autotune_pick(cache, key, split_tail ? 2 * nvariants : nvariants, st, [&](int c) -> int {
      return usable(c) ? run(split_tail ? c / 2 : c, split_tail && (c & 1)) : FN2_ERR_UNSUPPORTED;
    }, usable);
  }
  if (picked >= 0) {
    p.variant = split_tail ? picked / 2 : picked;
    p.tail = split_tail && (picked & 1);
  } else {
    double bc = 0;
    for (int i = 0; i < nvariants; ++i) {
      if (!applies(i)) continue;
      for (int t = 0; t < (split_tail && has_tail(i) ? 2 : 1); ++t) {
        const double c = cost(i, t == 1);
        if (p.variant < 0 || c < bc) { p.variant = i; bc = c; p.tail = t == 1; }
      }
    }
  }
  if (p.variant < 0) return fail(FN2_ERR_UNSUPPORTED, "%s: no kernel variant for this geometry", what);
  return FN2_OK;
}

}  // namespace mfma
}  // namespace fn2
