/* Solver update: SGD / Adam over every learnable blob of a net in one launch (csrc/solver_update.hip).  Part of include/flownet2_hip.h,
 * which includes this file; do not include it on its own.  There is no CPU twin in the oracle: the yardstick of tests/test_solver_update.py
 * is a NumPy float64 evaluation of the formulas below.
 *
 *   replaces  SGDSolver::ApplyUpdate            src/caffe/solvers/sgd_solver.cpp:101-116   ClipGradients, then per blob Normalize, Regularize,
 *                                                                                          ComputeUpdateValue, then Net::Update
 *             SGDSolver::ClipGradients          sgd_solver.cpp:80-99     scale = clip / ||g||_2 over ALL blobs, when the norm exceeds clip
 *             SGDSolver::Normalize              sgd_solver.cpp:118-142   g *= 1 / iter_size (skipped for iter_size == 1)
 *             SGDSolver::Regularize             sgd_solver.cpp:144-204   g += local_decay * w (L2) | local_decay * sign(w) (L1); skipped for 0
 *             SGDUpdate / sgd_update_gpu        solvers/sgd_solver.cu    h = momentum * h + local_rate * g;  g = h
 *             AdamUpdate / adam_update_gpu      solvers/adam_solver.cu:7-15   m = m*b1 + g*(1-b1); v = v*b2 + g*g*(1-b2);
 *                                                                             g = clr * m / (sqrt(v) + delta)
 *             Net::Update -> Blob::Update       net.cpp:929-934, blob.cpp:166-188   w -= g
 *
 * Per element, all in fp32, each operation rounded on its own (no fused multiply-add), with g the diff, w the data:
 *     g = g * clip_scale                     only with clip_gradients >= 0; clip_scale = 1 unless the norm of the diffs exceeds clip_gradients
 *     g = g * accum_normalization
 *     g = g + local_decay * w  |  g + local_decay * sign(w)          local_decay = weight_decay * decay_mult; skipped when it is 0
 *     SGD : hist0 = momentum * hist0 + (rate * lr_mult) * g                                     upd = hist0
 *     Adam: hist0 = hist0 * momentum + g * (1 - momentum);  hist1 = hist1 * momentum2 + (g * g) * (1 - momentum2)
 *           upd = ((rate * lr_mult * correction) * hist0) / (sqrt(hist1) + delta)
 *     w = w - upd;   diff = upd when write_update != 0, otherwise the diff is not written
 * A blob with lr_mult == 0 still updates its history, as in the reference.  The reference's update_ / temp_ blobs do not exist.
 *
 * The table (device memory, built once per set of blobs by ONE host-to-device copy): a header, the blob descriptors, a chunk list
 * {blob, element offset} of FN2_SOLVER_CHUNK elements per entry (one workgroup per chunk, so blobs of very different sizes balance), and
 * one double per chunk for the clip reduction.  fn2_solver_table_build is the only function here that synchronises (the stream, after its
 * copy: the staging buffer is a host temporary); fn2_solver_apply_update launches only: one kernel, or three with clipping
 * (per-chunk sums of squares: squared in fp32, accumulated in fp64, in an order fixed by the blob sizes alone; a one-workgroup finalize
 * that adds them in chunk order and writes clip_scale = l2 > clip ? float(clip / l2) : 1 into the table; the update reads it).  No
 * host readback, no atomics: the result is bit-reproducible, and the norm is more accurate than the reference's per-blob fp32 dot.
 * The "Gradient clipping" log line of the reference is not reproduced. */
#ifndef FLOWNET2_HIP_SOLVER_H_
#define FLOWNET2_HIP_SOLVER_H_
enum { FN2_SOLVER_SGD = 0, FN2_SOLVER_ADAM = 1 };
enum { FN2_SOLVER_REG_L2 = 0, FN2_SOLVER_REG_L1 = 1 };
#define FN2_SOLVER_CHUNK 4096      /* elements per chunk-list entry */

typedef struct fn2_solver_blob {
  float* data;            /* Blob::mutable_gpu_data of a learnable parameter; device pointers, 4-byte aligned at least */
  float* diff;            /* Blob::mutable_gpu_diff */
  float* hist0;           /* history_[i]: momentum (SGD) / first moment (Adam) */
  float* hist1;           /* history_[i + n]: second moment (Adam); may be NULL for SGD */
  long long count;        /* > 0 */
  float lr_mult;          /* Net::params_lr()[i] */
  float decay_mult;       /* Net::params_weight_decay()[i] */
} fn2_solver_blob;

typedef struct fn2_solver_params {
  int type;                   /* FN2_SOLVER_SGD, FN2_SOLVER_ADAM */
  int regularization;         /* FN2_SOLVER_REG_L2, FN2_SOLVER_REG_L1 */
  float momentum;             /* SolverParameter.momentum (Adam: beta1) */
  float momentum2;            /* SolverParameter.momentum2 (Adam: beta2) */
  float delta;                /* SolverParameter.delta */
  float weight_decay;         /* SolverParameter.weight_decay */
  float clip_gradients;       /* SolverParameter.clip_gradients; < 0: off, neither clip kernel is launched */
  float accum_normalization;  /* 1 / iter_size */
} fn2_solver_params;

/* What the HOST keeps about a built table (the library is stateless and never reads device memory back). */
typedef struct fn2_solver_table_info {
  int nblobs;
  int has_hist1;              /* every blob came with a hist1 pointer */
  long long nchunks;
  size_t bytes;               /* what fn2_solver_table_bytes returned */
} fn2_solver_table_info;

/* Bytes of table + chunk list + clip partials; 0 (and the error string) for what fn2_solver_table_build refuses in the blobs. */
size_t fn2_solver_table_bytes(int nblobs, const fn2_solver_blob* blobs);
/* HOST array of blobs -> device table.  Refused before anything is copied: NULL blobs / table / info, nblobs <= 0, a NULL data / diff /
 * hist0 pointer, count <= 0, a pointer that is not 4-byte aligned, hist1 set for some blobs and NULL for others, bytes too small. */
int fn2_solver_table_build(int nblobs, const fn2_solver_blob* blobs, void* table, size_t bytes, fn2_solver_table_info* info, void* stream);
/* One update of every blob in the table.  rate = GetLearningRate(), correction = sqrt(1 - b2^t) / (1 - b1^t) with t = iter + 1 (Adam;
 * ignored by SGD).  Refused on the host before any launch: NULL p / table / info, an unknown type or regularization, Adam on a table
 * without hist1. */
int fn2_solver_apply_update(const fn2_solver_params* p, void* table, const fn2_solver_table_info* info, float rate, float correction,
                            int write_update, void* stream);
#endif
