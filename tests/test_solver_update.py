"""The solver update kernel (csrc/solver_update.hip) through flownet2_amd.ops and the C ABI, against a NumPy float64 evaluation of the
formulas in include/flownet2_hip_solver.h on the same float32 inputs and constants (tests/solver_ref.py holds the yardsticks and the
derivation of the one-step bound).

One blob set exercises every path of the kernel: counts around the vector width, the wave and the chunk; 300 blobs of 2 elements (more
than any by-value table would hold); views at element offsets 1, 2, 3 into flat buffers, whose data / diff / history are misaligned
DIFFERENTLY (the scalar path), and one view whose four arrays share their misalignment (scalar head, vector body, scalar tail).
No element is excluded from any comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

import solver_ref as R
from flownet2_amd import Fn2Error, _lib, ops

CHUNK = ops.SOLVER_CHUNK
COUNTS = [1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 7, 2 * CHUNK + 1] + [2] * 300
# (count, element offsets of data / diff / hist0 / hist1 inside their flat buffers)
VIEWS = [(37, (1, 2, 3, 1)), (130, (2, 3, 1, 2)), (CHUNK + 5, (3, 1, 2, 3)), (CHUNK + 77, (1, 1, 1, 1))]
SPECS = [(n, (0, 0, 0, 0)) for n in COUNTS] + VIEWS
NB = len(SPECS)
LR_MULT = np.array([(1.0, 2.0, 0.0)[i % 3] for i in range(NB)], np.float32)
DECAY_MULT = np.array([(1.0, 0.0)[i % 2] for i in range(NB)], np.float32)
SIZES = np.array([n for n, _ in SPECS])
STARTS = np.concatenate([[0], np.cumsum(SIZES)])
TOTAL = int(STARTS[-1])
BLOB_OF = np.repeat(np.arange(NB), SIZES)            # element -> blob
TWO_ELEMENT = np.isin(BLOB_OF, [i for i, (n, _) in enumerate(SPECS) if n == 2])


def _inputs(seed=0):
    """w ~ N(0,1), g, m ~ 1e-3 N(0,1), v ~ 1e-6 |N(0,1)|; planted: g = m = v = 0 (every 97th element), and w = 0 as well (every 389th)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(TOTAL).astype(np.float32)
    g = (1e-3 * rng.standard_normal(TOTAL)).astype(np.float32)
    m = (1e-3 * rng.standard_normal(TOTAL)).astype(np.float32)
    v = (1e-6 * np.abs(rng.standard_normal(TOTAL))).astype(np.float32)
    zero = np.zeros(TOTAL, bool)
    zero[::97] = True
    zero[STARTS[:-1][SIZES == CHUNK + 7] + 3] = True
    g[zero] = 0
    m[zero] = 0
    v[zero] = 0
    w[::389] = 0
    return w, g, m, v, zero


class BlobSet:
    """Device tensors for SPECS (separate allocations, or views into flat buffers) and their table."""

    def __init__(self, lr_mult=LR_MULT, decay_mult=DECAY_MULT, with_hist1=True, pad=0):
        def alloc(n, off):
            return torch.zeros(n + 4 + pad, device="cuda")[off:off + n]
        self.t = [[alloc(n, offs[k]) for n, offs in SPECS] for k in range(4)]
        for k in range(4):
            for t, (n, offs) in zip(self.t[k], SPECS):
                assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offs[k]
        self.table = ops.SolverTable(self.t[0], self.t[1], self.t[2], self.t[3] if with_hist1 else None, lr_mult, decay_mult)

    def load(self, w, g, m, v):
        for k, a in enumerate((w, g, m, v)):
            for i, t in enumerate(self.t[k]):
                t.copy_(torch.from_numpy(a[STARTS[i]:STARTS[i + 1]]))

    def read(self):
        torch.cuda.synchronize()
        return [np.concatenate([t.cpu().numpy() for t in self.t[k]]) for k in range(4)]

    def run(self, inputs, params, rate, correction=1.0, write_update=False):
        self.load(*inputs)
        ops.solver_apply_update(self.table, params, rate, correction, write_update)
        return self.read()


@pytest.fixture(scope="module")
def blobs():
    return BlobSet()


RATE = {"SGD": 0.01, "Adam": 0.001}
MOMENTUM, MOMENTUM2, DELTA, WEIGHT_DECAY = 0.9, 0.999, 1e-8, 0.0004
CORRECTION = float(np.float32(np.sqrt(1 - float(np.float32(MOMENTUM2)) ** 3) / (1 - float(np.float32(MOMENTUM)) ** 3)))      # t = 3


def _params(type_, reg="none", accum=1.0, clip=-1.0, momentum=MOMENTUM):
    return ops.solver_params(type=ops.SOLVER_ADAM if type_ == "Adam" else ops.SOLVER_SGD,
                             regularization=ops.SOLVER_REG_L1 if reg == "L1" else ops.SOLVER_REG_L2, momentum=momentum, momentum2=MOMENTUM2,
                             delta=DELTA, weight_decay=0.0 if reg == "none" else WEIGHT_DECAY, clip_gradients=clip, accum_normalization=accum)


def _consts(type_, reg, accum, clip_scale=1.0, lr_mult=LR_MULT, decay_mult=DECAY_MULT, rate=None, momentum=MOMENTUM):
    return R.constants(type_, RATE[type_] if rate is None else rate, CORRECTION, momentum, MOMENTUM2, DELTA, 0.0 if reg == "none" else WEIGHT_DECAY,
                       lr_mult[BLOB_OF], decay_mult[BLOB_OF], accum, clip_scale)


CASES = [(t, r, a) for t in ("SGD", "Adam") for r in ("none", "L2", "L1") for a in (1.0, 0.5)]


@pytest.mark.parametrize("type_,reg,accum", CASES)
def test_numpy_float32_restatement_stays_within_the_bound(type_, reg, accum):
    """The bound is checked on the CPU first: an op-by-op float32 restatement of the kernel must itself meet it."""
    w, g, m, v, zero = _inputs()
    c = _consts(type_, reg, accum)
    bnd, ref = R.bound(w, g, m, v, c, reg == "L1")
    got = R.ref32(w, g, m, v, c, reg == "L1")
    ratios = {k: R.worst_ratio(got[k], ref[k], bnd[k]) for k in ("h0", "h1", "upd", "w") if ref[k] is not None}
    print("float32 restatement %s %s accum %g: worst error / bound %s" % (type_, reg, accum, {k: round(x, 3) for k, x in ratios.items()}))
    assert max(ratios.values()) <= 1.0, ratios
    assert 0.01 < max(ratios.values()), "a bound a hundred times the error pins nothing"
    no_reg = zero & ((c["ld"] == 0) | (w == 0))
    assert no_reg.sum() > 20 and np.all(got["upd"][no_reg] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("type_,reg,accum", CASES)
def test_one_step_meets_the_bound_against_fp64(blobs, type_, reg, accum):
    w, g, m, v, zero = _inputs()
    c = _consts(type_, reg, accum)
    bnd, ref = R.bound(w, g, m, v, c, reg == "L1")
    wn, gn, mn, vn = blobs.run((w, g, m, v), _params(type_, reg, accum), RATE[type_], CORRECTION, write_update=True)
    got = {"h0": mn, "h1": vn if type_ == "Adam" else None, "upd": gn, "w": wn}
    ratios = {k: R.worst_ratio(got[k], ref[k], bnd[k]) for k in ("h0", "h1", "upd", "w") if ref[k] is not None}
    same = all(np.array_equal(got[k], x) for k, x in R.ref32(w, g, m, v, c, reg == "L1").items() if x is not None)
    print("GPU %s %s accum %g: worst error / bound %s; bits of the float32 restatement: %s" % (type_, reg, accum, {k: round(x, 3) for k, x in ratios.items()}, same))
    for k in ratios:
        err = np.abs(got[k].astype(np.float64) - ref[k])
        assert np.all(err <= bnd[k]), (k, ratios[k], int(np.argmax(err - bnd[k])))
    if type_ == "SGD":
        assert np.array_equal(vn, v)                          # hist1 is not touched by SGD
    no_reg = zero & ((c["ld"] == 0) | (w == 0))
    assert np.all(gn[no_reg] == 0) and np.array_equal(wn[no_reg], w[no_reg])          # g = m = v = 0: the update is exactly 0


@pytest.mark.gpu
@pytest.mark.parametrize("type_", ["SGD", "Adam"])
def test_frozen_blobs_no_regularization_bits_and_the_diff_flag(blobs, type_):
    w, g, m, v = inputs = _inputs()[:4]
    frozen = LR_MULT[BLOB_OF] == 0
    if type_ == "SGD":
        # SGD's update IS the history (upd = momentum * h + 0 * g for lr_mult == 0, as in the reference): a frozen blob stands still
        # where its history is zero, and that history stays zero
        m[frozen] = 0
    wn, gn, mn, vn = blobs.run(inputs, _params(type_, "L2"), RATE[type_], CORRECTION)
    assert np.array_equal(gn.view(np.uint32), g.view(np.uint32))                      # write_update off: the diff is not written
    assert frozen.sum() > 1000 and np.array_equal(wn[frozen].view(np.uint32), w[frozen].view(np.uint32))          # lr_mult == 0: w keeps its bits ...
    moved = frozen & (g != 0)
    if type_ == "Adam":                                                                # ... while Adam's moments move
        assert np.mean(mn[moved] != m[moved]) > 0.99 and np.mean(vn[moved] != v[moved]) > 0.99
    else:
        assert not np.any(mn[frozen]) and np.array_equal(vn, v)
    assert np.mean(wn[~frozen & (g != 0)] != w[~frozen & (g != 0)]) > 0.99
    # decay_mult == 0 gives the bits of the run without regularization; so does weight_decay == 0 with any regularization type
    plain = blobs.run(inputs, _params(type_, "none"), RATE[type_], CORRECTION)
    nodecay = DECAY_MULT[BLOB_OF] == 0
    for a, b in zip((wn, mn, vn), (plain[0], plain[2], plain[3])):
        assert np.array_equal(a[nodecay].view(np.uint32), b[nodecay].view(np.uint32))
        assert not np.array_equal(a[~nodecay], b[~nodecay]) or a is vn and type_ == "SGD"
    p = _params(type_, "L1")
    p.weight_decay = 0.0
    for a, b in zip(blobs.run(inputs, p, RATE[type_], CORRECTION), plain):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_clip_scale(blobs):
    """SGD with momentum 0, rate 1, w = 0, no decay: w_new = -clip_scale * g.  Most of the norm sits in the 2-element blobs: the norm spans
    ALL blobs of the table."""
    w, g, m, v, _ = _inputs(seed=1)
    w[:] = 0
    g[TWO_ELEMENT] *= 100
    ones = BlobSet(lr_mult=np.ones(NB, np.float32))
    norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    assert np.sum(g[TWO_ELEMENT].astype(np.float64) ** 2) > 0.9 * norm ** 2
    clip = float(np.float32(norm / 2))
    wn = ones.run((w, g, m, v), _params("SGD", clip=clip, momentum=0.0), 1.0)[0]
    want = -g.astype(np.float64) * (clip / norm)
    err = np.abs(wn - want)
    print("clip: worst error / (4 u |g scale|) = %.3f" % float(np.max(np.where(err == 0, 0, err / np.maximum(4 * R.U * np.abs(want), 1e-300)))))
    assert np.all(err <= 4 * R.U * np.abs(want))
    above = ones.run((w, g, m, v), _params("SGD", clip=float(np.float32(norm * 1.01)), momentum=0.0), 1.0)[0]
    assert np.array_equal(above, -g) and np.array_equal(above[g != 0].view(np.uint32), (-g)[g != 0].view(np.uint32))      # the scale is exactly 1
    off = ones.run((w, g, m, v), _params("SGD", clip=-1.0, momentum=0.0), 1.0)[0]
    assert np.array_equal(off.view(np.uint32), above.view(np.uint32))


@pytest.mark.gpu
def test_bit_reproducible_across_runs_and_allocations(blobs):
    inputs = _inputs(seed=2)[:4]
    norm = float(np.sqrt(np.sum(inputs[1].astype(np.float64) ** 2)))
    p = _params("Adam", "L2", 0.5, clip=norm / 3)
    first = blobs.run(inputs, p, RATE["Adam"], CORRECTION, write_update=True)
    again = blobs.run(inputs, p, RATE["Adam"], CORRECTION, write_update=True)
    elsewhere = BlobSet(pad=64).run(inputs, p, RATE["Adam"], CORRECTION, write_update=True)          # the same blobs in the same order, other addresses
    for a, b, c in zip(first, again, elsewhere):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))
    assert not np.array_equal(first[0], blobs.run(inputs, _params("Adam", "L2", 0.5), RATE["Adam"], CORRECTION, write_update=True)[0])      # the clip did scale


@pytest.mark.gpu
def test_a_nan_gradient_reaches_only_its_own_element(blobs):
    w, g, m, v = _inputs(seed=3)[:4]
    clean = blobs.run((w, g, m, v), _params("Adam", "L2"), RATE["Adam"], CORRECTION)
    at = int(STARTS[:-1][SIZES == 2 * CHUNK + 1][0]) + CHUNK + 9
    assert LR_MULT[BLOB_OF[at]] != 0
    g2 = g.copy()
    g2[at] = np.nan
    dirty = blobs.run((w, g2, m, v), _params("Adam", "L2"), RATE["Adam"], CORRECTION)
    others = np.arange(TOTAL) != at
    for k in (0, 2, 3):
        assert np.isnan(dirty[k][at]) and np.array_equal(dirty[k][others].view(np.uint32), clean[k][others].view(np.uint32))


@pytest.mark.gpu
def test_refusals_are_decided_on_the_host_and_touch_nothing():
    L = _lib.lib()
    INVALID, WORKSPACE = -1, -3
    n = 3
    t = [[torch.full((8,), float(10 * k + i), device="cuda") for i in range(n)] for k in range(4)]
    before = [[x.clone() for x in row] for row in t]

    def descr(**change):
        arr = (_lib.SolverBlob * n)()
        for i in range(n):
            arr[i] = _lib.SolverBlob(t[0][i].data_ptr(), t[1][i].data_ptr(), t[2][i].data_ptr(), t[3][i].data_ptr(), 8, 1.0, 1.0)
        for field, value in change.items():
            setattr(arr[1], field, value)
        return arr

    good = descr()
    nbytes = L.fn2_solver_table_bytes(n, good)
    assert nbytes > 0
    table = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    info = _lib.SolverTableInfo()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tp = C.c_void_p(table.data_ptr())

    def refused(rc, code, pattern):
        assert rc == code, (rc, L.fn2_last_error_string())
        assert pattern in L.fn2_last_error_string().decode(), L.fn2_last_error_string()

    for change, pattern in (({"data": None}, "NULL"), ({"diff": None}, "NULL"), ({"hist0": None}, "NULL"), ({"count": 0}, "count 0"),
                            ({"count": -5}, "count -5"), ({"diff": t[1][1].data_ptr() + 2}, "not 4-byte aligned"),
                            ({"hist1": None}, "hist1 must be given for every blob")):
        bad = descr(**change)
        assert L.fn2_solver_table_bytes(n, bad) == 0 and pattern in L.fn2_last_error_string().decode()
        refused(L.fn2_solver_table_build(n, bad, tp, nbytes, C.byref(info), stream), INVALID, pattern)
    refused(L.fn2_solver_table_build(n, None, tp, nbytes, C.byref(info), stream), INVALID, "blobs is NULL")
    refused(L.fn2_solver_table_build(0, good, tp, nbytes, C.byref(info), stream), INVALID, "nblobs = 0")
    refused(L.fn2_solver_table_build(n, good, None, nbytes, C.byref(info), stream), INVALID, "NULL")
    refused(L.fn2_solver_table_build(n, good, tp, nbytes, None, stream), INVALID, "NULL")
    refused(L.fn2_solver_table_build(n, good, tp, nbytes - 1, C.byref(info), stream), WORKSPACE, "needed")
    assert not table.any()                                                              # nothing was copied
    # a table without hist1 (SGD) refuses Adam; unknown type / regularization; NULL arguments
    sgd_blobs = (_lib.SolverBlob * n)()
    for i in range(n):
        sgd_blobs[i] = _lib.SolverBlob(t[0][i].data_ptr(), t[1][i].data_ptr(), t[2][i].data_ptr(), None, 8, 1.0, 1.0)
    assert L.fn2_solver_table_build(n, sgd_blobs, tp, nbytes, C.byref(info), stream) == 0 and info.has_hist1 == 0 and info.nchunks == 3 and info.nblobs == 3
    built = table.clone()
    p = ops.solver_params(type=ops.SOLVER_ADAM)
    refused(L.fn2_solver_apply_update(C.byref(p), tp, C.byref(info), 0.1, 1.0, 0, stream), INVALID, "Adam needs hist1")
    for field, value, pattern in (("type", 2, "unknown solver type 2"), ("type", -1, "unknown solver type -1"), ("regularization", 7, "unknown regularization type 7")):
        p = ops.solver_params()
        setattr(p, field, value)
        refused(L.fn2_solver_apply_update(C.byref(p), tp, C.byref(info), 0.1, 1.0, 0, stream), INVALID, pattern)
    p = ops.solver_params()
    refused(L.fn2_solver_apply_update(None, tp, C.byref(info), 0.1, 1.0, 0, stream), INVALID, "NULL")
    refused(L.fn2_solver_apply_update(C.byref(p), None, C.byref(info), 0.1, 1.0, 0, stream), INVALID, "NULL")
    refused(L.fn2_solver_apply_update(C.byref(p), tp, None, 0.1, 1.0, 0, stream), INVALID, "NULL")
    refused(L.fn2_solver_apply_update(C.byref(p), tp, C.byref(_lib.SolverTableInfo()), 0.1, 1.0, 0, stream), INVALID, "no built table")
    torch.cuda.synchronize()
    assert torch.equal(table, built)
    for row, brow in zip(t, before):
        for x, b in zip(row, brow):
            assert torch.equal(x, b)
    # the Python layer: CPU tensors and mismatched lists are refused before the library is asked
    with pytest.raises(ValueError, match="no CPU path"):
        ops.SolverTable([torch.zeros(4)], [torch.zeros(4)], [torch.zeros(4)])
    with pytest.raises(ValueError, match="data\\[0\\] has 8"):
        ops.SolverTable([t[0][0]], [t[1][0][:4]], [t[2][0]])
    with pytest.raises(Fn2Error, match="Adam needs hist1"):
        ops.solver_apply_update(ops.SolverTable(t[0], t[1], t[2]), ops.solver_params(type=ops.SOLVER_ADAM), 0.1)
    # and the accepted call does update: SGD, momentum 0, rate 1 -> w = w - g
    ops.solver_apply_update(ops.SolverTable(t[0], t[1], t[2]), ops.solver_params(), 1.0)
    assert torch.equal(t[0][0], before[0][0] - before[1][0])
