// Solver update: clip, normalize, regularize, SGD / Adam history update and Net::Update of EVERY learnable blob of a net in one launch
// (HBM-bound: Adam moves 7 arrays of 4 bytes per element -- w, g, m, v read, w, m, v written; 8 with write_update).
//
// Reference: SGDSolver::ApplyUpdate (src/caffe/solvers/sgd_solver.cpp:101-116) = ClipGradients (:80-99) and then, PER BLOB, Normalize
// (:118-142, a scal), Regularize (:144-204, an axpy, plus a sign pass for L1), ComputeUpdateValue (sgd_solver.cu / adam_solver.cu:7-15) and
// Blob::Update (blob.cpp:166-188, an axpy): four to six launches and as many passes per blob, 200+ blobs per FlowNet2 net, plus the
// update_ / temp_ scratch blobs.  Here: a device-resident table {data, diff, hist0, hist1, count, lr_mult, decay_mult} per blob and a chunk
// list (blob, element offset) of kChunk elements per entry; workgroup c of the grid takes chunk c, so 200 blobs of very different sizes
// balance and the launch count does not depend on the number of blobs.  The table is copied to the device once per set of blobs; the
// per-step scalars are kernel arguments.  The arithmetic (include/flownet2_hip_solver.h) is fp32 with every operation rounded on its own
// (fp contraction is off in update_one: the vector and the scalar path, and a NumPy float32 restatement, give the same bits).
//
// Access: 16 bytes per lane where data / diff / hist0 / hist1 of a blob share their address modulo 16 (a scalar head of up to three
// elements brings a chunk to the boundary, a scalar tail finishes it; chunk offsets are multiples of 4 elements); blobs whose pointers are
// misaligned DIFFERENTLY (views at odd element offsets into flat buffers) take the scalar path throughout.
//
// ClipGradients: solver_sumsq writes one double per chunk (squares in fp32, sums in fp64; element -> thread and the reduction tree do not
// depend on alignment or addresses), solver_clip_finalize (one workgroup) adds them in chunk order (thread t a contiguous run, then the
// tree) and writes clip_scale = l2 > clip ? float(clip / l2) : 1 into the table header, which solver_update reads: no host readback, no
// atomics, bit-reproducible for given blob sizes -- and more accurate than the reference's per-blob fp32 dot (cublasSdot) summed in fp32.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), no scratch, no spills:
//   solver_update<SGD>   VGPR 36  SGPR 41  LDS 0      solver_update<ADAM>  VGPR 51  SGPR 54  LDS 0        8 waves / SIMD each
//   solver_sumsq         VGPR 15  SGPR 25  LDS 2048   solver_clip_finalize VGPR 14  SGPR 16  LDS 2048
#include "fn2_common.hpp"

#include <cstdint>
#include <vector>

namespace fn2 {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kChunk = FN2_SOLVER_CHUNK;
constexpr int kThreads = 256;
constexpr unsigned kMagic = 0x534f4c56u;      // "SOLV"

struct TableHeader {                // 64 bytes at the start of the table
  unsigned magic;
  int nblobs;
  long long nchunks;
  long long off_blobs, off_chunks, off_partials;      // byte offsets from the start of the table
  float clip_scale;                 // written by solver_clip_finalize
  int has_hist1;
  long long reserved[2];
};
static_assert(sizeof(TableHeader) == 64, "table header layout");
static_assert(sizeof(fn2_solver_blob) == 48, "blob descriptor layout");

struct ChunkEntry { long long offset; int blob; int pad; };
static_assert(sizeof(ChunkEntry) == 16, "chunk entry layout");

struct StepScalars {                // per launch, uniform
  float clip_on;                    // != 0: multiply by the table's clip_scale
  float accum_normalization;
  float weight_decay;
  int l1;
  float rate, correction;
  float momentum, momentum2;        // SGD: momentum; Adam: beta1, beta2
  float one_minus_b1, one_minus_b2; // formed in fp32 on the host, as adam_solver.cu forms them from its fp32 arguments
  float delta;
  int write_update;
};

struct BlobScalars {                // per chunk, uniform
  float clip_scale, accum_normalization, local_decay, local_rate;
  int clip_on, l1;
};

template <int TYPE>
__device__ __forceinline__ float update_one(float& w, float g, float& h0, float& h1, const BlobScalars& b, const StepScalars& s) {
#pragma clang fp contract(off)
  if (b.clip_on) g = g * b.clip_scale;
  g = g * b.accum_normalization;
  if (b.local_decay != 0.f) {
    const float r = b.l1 ? (float)((w > 0.f) - (w < 0.f)) : w;
    const float t = b.local_decay * r;
    g = g + t;
  }
  float upd;
  if constexpr (TYPE == FN2_SOLVER_SGD) {
    const float a = s.momentum * h0;
    const float c = b.local_rate * g;
    h0 = a + c;
    upd = h0;
  } else {
    const float a = h0 * s.momentum;
    const float c = g * s.one_minus_b1;
    h0 = a + c;
    const float d = h1 * s.momentum2;
    const float gg = g * g;
    const float e = gg * s.one_minus_b2;
    h1 = d + e;
    const float num = b.local_rate * h0;           // local_rate = rate * lr_mult * correction here
    const float den = sqrtf(h1) + s.delta;
    upd = num / den;
  }
  w = w - upd;
  return upd;
}

// grid: one workgroup per chunk
template <int TYPE>
__global__ void __launch_bounds__(kThreads) solver_update(unsigned char* __restrict__ table, StepScalars s) {
  const TableHeader* hdr = reinterpret_cast<const TableHeader*>(table);
  const long long c = blockIdx.x;
  if (hdr->magic != kMagic || c >= hdr->nchunks) return;
  const ChunkEntry ce = reinterpret_cast<const ChunkEntry*>(table + hdr->off_chunks)[c];
  const fn2_solver_blob bl = reinterpret_cast<const fn2_solver_blob*>(table + hdr->off_blobs)[ce.blob];
  const long long left = bl.count - ce.offset;
  const int n = left < (long long)kChunk ? (int)left : kChunk;
  float* __restrict__ w = bl.data + ce.offset;
  float* __restrict__ g = bl.diff + ce.offset;
  float* __restrict__ h0 = bl.hist0 + ce.offset;
  float* __restrict__ h1 = TYPE == FN2_SOLVER_ADAM ? bl.hist1 + ce.offset : nullptr;

  BlobScalars b;
  b.clip_on = s.clip_on != 0.f;
  b.clip_scale = b.clip_on ? hdr->clip_scale : 1.f;
  b.accum_normalization = s.accum_normalization;
  b.l1 = s.l1;
  {
#pragma clang fp contract(off)
    b.local_decay = s.weight_decay * bl.decay_mult;
    const float local_rate = s.rate * bl.lr_mult;
    b.local_rate = TYPE == FN2_SOLVER_ADAM ? local_rate * s.correction : local_rate;
  }

  // the four arrays share their address modulo 16 -> a scalar head of `head` elements puts all of them on a 16-byte boundary
  const unsigned mw = (unsigned)(reinterpret_cast<uintptr_t>(w) & 15), mg = (unsigned)(reinterpret_cast<uintptr_t>(g) & 15);
  const unsigned m0 = (unsigned)(reinterpret_cast<uintptr_t>(h0) & 15);
  const unsigned m1 = TYPE == FN2_SOLVER_ADAM ? (unsigned)(reinterpret_cast<uintptr_t>(h1) & 15) : mw;
  const bool vec = mw == mg && mw == m0 && mw == m1;
  int head = vec ? (int)(((16u - mw) & 15u) >> 2) : n;
  if (head > n) head = n;
  const int nvec = (n - head) >> 2;
  const int tail0 = head + 4 * nvec;
  const int tid = threadIdx.x;

  for (int i = tid; i < head + (n - tail0); i += kThreads) {            // scalar head and tail (everything, for a misaligned blob)
    const int e = i < head ? i : tail0 + (i - head);
    float wv = w[e], h0v = h0[e], h1v = 0.f;
    if constexpr (TYPE == FN2_SOLVER_ADAM) h1v = h1[e];
    const float upd = update_one<TYPE>(wv, g[e], h0v, h1v, b, s);
    w[e] = wv;
    h0[e] = h0v;
    if constexpr (TYPE == FN2_SOLVER_ADAM) h1[e] = h1v;
    if (s.write_update) g[e] = upd;
  }
  f32x4* __restrict__ w4 = reinterpret_cast<f32x4*>(w + head);
  f32x4* __restrict__ g4 = reinterpret_cast<f32x4*>(g + head);
  f32x4* __restrict__ h04 = reinterpret_cast<f32x4*>(h0 + head);
  f32x4* __restrict__ h14 = TYPE == FN2_SOLVER_ADAM ? reinterpret_cast<f32x4*>(h1 + head) : nullptr;
#pragma unroll 2
  for (int i = tid; i < nvec; i += kThreads) {
    f32x4 wv = w4[i], gv = g4[i], h0v = h04[i], h1v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (TYPE == FN2_SOLVER_ADAM) h1v = h14[i];
    f32x4 uv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = wv[j], m = h0v[j], v = h1v[j];
      uv[j] = update_one<TYPE>(a, gv[j], m, v, b, s);
      wv[j] = a; h0v[j] = m; h1v[j] = v;
    }
    w4[i] = wv;
    h04[i] = h0v;
    if constexpr (TYPE == FN2_SOLVER_ADAM) h14[i] = h1v;
    if (s.write_update) g4[i] = uv;
  }
}

// fixed-order sum of kThreads doubles (the tree does not depend on the data)
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// grid: one workgroup per chunk.  Thread t owns elements 4 (t + 256 k) .. + 3 of the chunk whatever the alignment of the diff.
__global__ void __launch_bounds__(kThreads) solver_sumsq(unsigned char* __restrict__ table) {
  __shared__ double red[kThreads];
  const TableHeader* hdr = reinterpret_cast<const TableHeader*>(table);
  const long long c = blockIdx.x;
  if (hdr->magic != kMagic || c >= hdr->nchunks) return;
  const ChunkEntry ce = reinterpret_cast<const ChunkEntry*>(table + hdr->off_chunks)[c];
  const fn2_solver_blob bl = reinterpret_cast<const fn2_solver_blob*>(table + hdr->off_blobs)[ce.blob];
  const long long left = bl.count - ce.offset;
  const int n = left < (long long)kChunk ? (int)left : kChunk;
  const float* __restrict__ g = bl.diff + ce.offset;
  const bool aligned = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
  double acc = 0.0;
  for (int e = 4 * (int)threadIdx.x; e < n; e += 4 * kThreads) {
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (aligned && e + 3 < n) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (e + j < n) x[j] = g[e + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
      const float sq = x[j] * x[j];
      acc = acc + (double)sq;
    }
  }
  const double total = block_sum(acc, red);
  if (threadIdx.x == 0) reinterpret_cast<double*>(table + hdr->off_partials)[c] = total;
}

// grid: ONE workgroup.  Thread t adds the contiguous run [t * run, (t + 1) * run) of the partials in order, then the fixed tree.
__global__ void __launch_bounds__(kThreads) solver_clip_finalize(unsigned char* __restrict__ table, float clip) {
  __shared__ double red[kThreads];
  TableHeader* hdr = reinterpret_cast<TableHeader*>(table);
  if (hdr->magic != kMagic) return;
  const long long nchunks = hdr->nchunks;
  const double* __restrict__ partial = reinterpret_cast<const double*>(table + hdr->off_partials);
  const long long run = (nchunks + kThreads - 1) / kThreads;
  const long long lo = run * threadIdx.x;
  const long long hi = lo + run < nchunks ? lo + run : nchunks;
  double acc = 0.0;
  for (long long i = lo; i < hi; ++i) acc = acc + partial[i];
  const double total = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const double l2 = sqrt(total);
    hdr->clip_scale = l2 > (double)clip ? (float)((double)clip / l2) : 1.f;
  }
}

struct Layout { long long nchunks; size_t off_blobs, off_chunks, off_partials, bytes; };

// 0: fine; otherwise the error has been recorded
int validate_blobs(int nblobs, const fn2_solver_blob* blobs, const char* who) {
  if (!blobs) return fail(FN2_ERR_INVALID_ARG, "%s: blobs is NULL", who);
  if (nblobs <= 0) return fail(FN2_ERR_INVALID_ARG, "%s: nblobs = %d", who, nblobs);
  for (int i = 0; i < nblobs; ++i) {
    const fn2_solver_blob& b = blobs[i];
    if (!b.data || !b.diff || !b.hist0) return fail(FN2_ERR_INVALID_ARG, "%s: blob %d has a NULL data / diff / hist0 pointer", who, i);
    if (b.count <= 0) return fail(FN2_ERR_INVALID_ARG, "%s: blob %d has count %lld", who, i, b.count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(b.data) | reinterpret_cast<uintptr_t>(b.diff) | reinterpret_cast<uintptr_t>(b.hist0) |
                           reinterpret_cast<uintptr_t>(b.hist1);
    if (bits & 3) return fail(FN2_ERR_INVALID_ARG, "%s: blob %d has a pointer that is not 4-byte aligned", who, i);
    if ((b.hist1 != nullptr) != (blobs[0].hist1 != nullptr))
      return fail(FN2_ERR_INVALID_ARG, "%s: blob %d: hist1 must be given for every blob (Adam) or for none (SGD)", who, i);
  }
  return FN2_OK;
}

Layout layout_of(int nblobs, const fn2_solver_blob* blobs) {
  Layout L{};
  for (int i = 0; i < nblobs; ++i) L.nchunks += (blobs[i].count + kChunk - 1) / kChunk;
  L.off_blobs = sizeof(TableHeader);
  L.off_chunks = L.off_blobs + sizeof(fn2_solver_blob) * (size_t)nblobs;            // 64 + 48 n: a multiple of 16
  L.off_partials = L.off_chunks + sizeof(ChunkEntry) * (size_t)L.nchunks;
  L.bytes = L.off_partials + sizeof(double) * (size_t)L.nchunks;
  return L;
}

}  // namespace
}  // namespace fn2

using namespace fn2;

FN2_API size_t fn2_solver_table_bytes(int nblobs, const fn2_solver_blob* blobs) {
  if (validate_blobs(nblobs, blobs, "solver_table_bytes") != FN2_OK) return 0;
  return layout_of(nblobs, blobs).bytes;
}

FN2_API int fn2_solver_table_build(int nblobs, const fn2_solver_blob* blobs, void* table, size_t bytes, fn2_solver_table_info* info, void* stream) {
  if (!table || !info) return fail(FN2_ERR_INVALID_ARG, "solver_table_build: table / info is NULL");
  if (reinterpret_cast<uintptr_t>(table) & 15) return fail(FN2_ERR_INVALID_ARG, "solver_table_build: table is not 16-byte aligned");
  if (int rc = validate_blobs(nblobs, blobs, "solver_table_build")) return rc;
  const Layout L = layout_of(nblobs, blobs);
  if (L.nchunks > 0x7fffffffLL) return fail(FN2_ERR_UNSUPPORTED, "solver_table_build: %lld chunks exceed one grid", L.nchunks);
  if (bytes < L.bytes) return fail(FN2_ERR_WORKSPACE, "solver_table_build: table holds %zu bytes, %zu needed", bytes, L.bytes);
  std::vector<unsigned char> host(L.off_partials, 0);            // the partials are written before they are read: not copied
  TableHeader* hdr = reinterpret_cast<TableHeader*>(host.data());
  hdr->magic = kMagic;
  hdr->nblobs = nblobs;
  hdr->nchunks = L.nchunks;
  hdr->off_blobs = (long long)L.off_blobs;
  hdr->off_chunks = (long long)L.off_chunks;
  hdr->off_partials = (long long)L.off_partials;
  hdr->clip_scale = 1.f;
  hdr->has_hist1 = blobs[0].hist1 != nullptr;
  fn2_solver_blob* db = reinterpret_cast<fn2_solver_blob*>(host.data() + L.off_blobs);
  ChunkEntry* dc = reinterpret_cast<ChunkEntry*>(host.data() + L.off_chunks);
  long long c = 0;
  for (int i = 0; i < nblobs; ++i) {
    db[i] = blobs[i];
    for (long long off = 0; off < blobs[i].count; off += kChunk) dc[c++] = ChunkEntry{off, i, 0};
  }
  hipStream_t st = as_stream(stream);
  hipError_t e = hipMemcpyAsync(table, host.data(), host.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);            // `host` is a temporary: the one synchronisation of this file
  if (e != hipSuccess) return fail(FN2_ERR_LAUNCH, "solver_table_build: %s", hipGetErrorString(e));
  info->nblobs = nblobs;
  info->has_hist1 = hdr->has_hist1;
  info->nchunks = L.nchunks;
  info->bytes = L.bytes;
  return FN2_OK;
}

FN2_API int fn2_solver_apply_update(const fn2_solver_params* p, void* table, const fn2_solver_table_info* info, float rate, float correction,
                                    int write_update, void* stream) {
  if (!p || !table || !info) return fail(FN2_ERR_INVALID_ARG, "solver_apply_update: params / table / info is NULL");
  if (p->type != FN2_SOLVER_SGD && p->type != FN2_SOLVER_ADAM) return fail(FN2_ERR_INVALID_ARG, "solver_apply_update: unknown solver type %d", p->type);
  if (p->regularization != FN2_SOLVER_REG_L2 && p->regularization != FN2_SOLVER_REG_L1)
    return fail(FN2_ERR_INVALID_ARG, "solver_apply_update: unknown regularization type %d", p->regularization);
  if (info->nblobs <= 0 || info->nchunks <= 0 || info->nchunks > 0x7fffffffLL) return fail(FN2_ERR_INVALID_ARG, "solver_apply_update: info describes no built table");
  if (p->type == FN2_SOLVER_ADAM && !info->has_hist1) return fail(FN2_ERR_INVALID_ARG, "solver_apply_update: Adam needs hist1, the table was built without");
  StepScalars s;
  s.clip_on = p->clip_gradients >= 0.f ? 1.f : 0.f;
  s.accum_normalization = p->accum_normalization;
  s.weight_decay = p->weight_decay;
  s.l1 = p->regularization == FN2_SOLVER_REG_L1;
  s.rate = rate;
  s.correction = correction;
  s.momentum = p->momentum;
  s.momentum2 = p->momentum2;
  s.one_minus_b1 = 1.f - p->momentum;
  s.one_minus_b2 = 1.f - p->momentum2;
  s.delta = p->delta;
  s.write_update = write_update != 0;
  hipStream_t st = as_stream(stream);
  unsigned char* t = reinterpret_cast<unsigned char*>(table);
  const dim3 grid((unsigned)info->nchunks), block(kThreads);
  if (p->clip_gradients >= 0.f) {
    hipLaunchKernelGGL(solver_sumsq, grid, block, 0, st, t);
    hipLaunchKernelGGL(solver_clip_finalize, dim3(1), block, 0, st, t, p->clip_gradients);
  }
  if (p->type == FN2_SOLVER_SGD) hipLaunchKernelGGL(solver_update<FN2_SOLVER_SGD>, grid, block, 0, st, t, s);
  else hipLaunchKernelGGL(solver_update<FN2_SOLVER_ADAM>, grid, block, 0, st, t, s);
  return check_launch("solver_apply_update");
}
