"""Host side of the Solver (flownet2_amd/solver.py): SolverParameter parsing, the seven learning-rate policies, Adam's correction, the
solver-state HDF5 file, the refusal of a CPU net.  No GPU."""
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import flownet2_amd
from flownet2_amd import _h5write, _lib, net as fnet, solver as fsolver
from flownet2_amd.layers import CheckError
from flownet2_amd.solver import SolverParameter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 4 * 2.0 ** -23        # one float32 rounding of the result plus the float32 roundings of the stored parameters

FULL = """
# every field the solver reads
train_net: "train.prototxt"
test_net: "a.prototxt" test_net: "b.prototxt"
test_iter: 10 test_iter: 20
test_interval: 500
test_state { stage: "x" } test_state { stage: "y" }
base_lr: 0.0001
display: 20
average_loss: 3
max_iter: 1200000
iter_size: 2
lr_policy: "multistep"
gamma: 0.5
power: 0.75
momentum: 0.9
momentum2: 0.999
delta: 1e-4
weight_decay: 0.0004
regularization_type: "L1"
stepsize: 100
stepvalue: 300000 stepvalue: 400000 stepvalue: 500000
clip_gradients: 10
snapshot: 20000
snapshot_prefix: "flow"
snapshot_format: HDF5
solver_mode: GPU
random_seed: 1
type: "Adam"
train_state { level: 1 stage: "s" }
"""


def test_parse_round_trip_defaults_and_refusals():
    p = SolverParameter(FULL)
    assert p.stepvalue == [300000, 400000, 500000] and p.test_net == ["a.prototxt", "b.prototxt"] and p.test_iter == [10, 20]
    assert [d["stage"] for d in p.to_dict()["test_state"]] == [["x"], ["y"]] and p.to_dict()["train_state"] == {"level": 1, "stage": ["s"]}
    assert p.type == "Adam" and p.lr_policy == "multistep" and p.regularization_type == "L1" and p.snapshot_format == "HDF5"
    assert p.base_lr == float(np.float32(0.0001)) and p.weight_decay == float(np.float32(0.0004)) and p.clip_gradients == 10.0
    assert p.iter_size == 2 and p.average_loss == 3 and p.max_iter == 1200000 and p.snapshot_prefix == "flow" and p.random_seed == 1
    again = SolverParameter(p.to_prototxt())
    assert again == p and again.to_prototxt() == p.to_prototxt()
    assert SolverParameter(p.to_dict()) == p and SolverParameter(p) == p
    # one repeated value without brackets, several in brackets
    assert SolverParameter("stepvalue: 7").stepvalue == [7] and SolverParameter("stepvalue: [1, 2]").stepvalue == [1, 2]
    # defaults of caffe.proto:104-244
    d = SolverParameter("")
    assert d.type == "SGD" and d.delta == float(np.float32(1e-8)) and d.momentum2 == float(np.float32(0.999)) and d.clip_gradients == -1.0
    assert d.iter_size == 1 and d.regularization_type == "L2" and d.average_loss == 1 and d.snapshot == 0 and d.snapshot_format == "BINARYPROTO"
    assert d.stepvalue == [] and d.base_lr is None and not d.has("type") and d.test_initialization is True and d.random_seed == -1
    # from a dict and from keywords
    assert SolverParameter({"base_lr": 0.1, "stepvalue": [3, 4], "type": "Adam"}) == SolverParameter('base_lr: 0.1 stepvalue: 3 stepvalue: 4 type: "Adam"')
    assert SolverParameter(base_lr=0.5, lr_policy="fixed").base_lr == 0.5
    # the deprecated enum maps to the string (upgrade_proto.cpp: UpgradeSolverType)
    for enum, name in (("SGD", "SGD"), ("NESTEROV", "Nesterov"), ("ADAGRAD", "AdaGrad"), ("RMSPROP", "RMSProp"), ("ADADELTA", "AdaDelta"), ("ADAM", "Adam")):
        assert SolverParameter("solver_type: %s" % enum).type == name
    with pytest.raises(CheckError, match="cannot be both"):
        SolverParameter('solver_type: ADAM type: "Adam"')
    with pytest.raises(CheckError, match='no field named "learning_rate"'):
        SolverParameter("learning_rate: 0.1")
    with pytest.raises(CheckError, match="Unknown solver type: Lion"):
        SolverParameter('type: "Lion"')
    with pytest.raises(CheckError, match="unknown enumeration value"):
        SolverParameter("snapshot_format: JSON")
    for name in ("Nesterov", "AdaGrad", "RMSProp", "AdaDelta"):
        with pytest.raises(CheckError, match="Solver type %s is not implemented" % name):
            fsolver.get_solver(SolverParameter('type: "%s" base_lr: 0.1 lr_policy: "fixed"' % name))
    assert flownet2_amd.SolverParameter is SolverParameter and flownet2_amd.get_solver is fsolver.get_solver
    assert flownet2_amd.CaffeOptimizer is fsolver.CaffeOptimizer and flownet2_amd.AdamSolver is fsolver.AdamSolver


def test_solver_header_declares_exactly_what_is_exported():
    hdr = open(os.path.join(ROOT, "include", "flownet2_hip_solver.h")).read()
    declared = set(re.findall(r"\b(fn2_solver_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SOLVER_EXPORTS) and len(declared) == 3
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert '#include "flownet2_hip_solver.h"' in open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()


class _Sched(fsolver._Schedule):
    def __init__(self, text):
        self._init_schedule(SolverParameter(text))


# base_lr 0.01 is inexact in float32 (one rounding); the parameters an exponent amplifies (gamma, power) are exact in float32
BASE, GAMMA, POWER, STEPSIZE, MAX_ITER, STEPVALUES = 0.01, 0.5, 0.75, 4, 24, (6, 9)
ITERS = (0, 1, STEPSIZE - 1, STEPSIZE, STEPVALUES[0], STEPVALUES[0] + 1, MAX_ITER - 1)


def _closed_form(policy, it, gamma):
    """The proto comment (caffe.proto:159-173) in fp64."""
    if policy == "fixed":
        return BASE
    if policy == "step":
        return BASE * gamma ** (it // STEPSIZE)
    if policy == "exp":
        return BASE * gamma ** it
    if policy == "inv":
        return BASE * (1 + gamma * it) ** (-POWER)
    if policy == "multistep":
        return BASE * gamma ** sum(it >= s for s in STEPVALUES)
    if policy == "poly":
        return BASE * (1 - it / MAX_ITER) ** POWER
    return BASE * (1 / (1 + math.exp(-gamma * (it - STEPSIZE))))


@pytest.mark.parametrize("policy", ["fixed", "step", "exp", "inv", "multistep", "poly", "sigmoid"])
def test_learning_rate_policies_against_fp64(policy):
    gamma = -GAMMA if policy == "sigmoid" else GAMMA         # a decaying sigmoid
    s = _Sched('base_lr: %r lr_policy: "%s" gamma: %r power: %r stepsize: %d max_iter: %d stepvalue: %d stepvalue: %d'
               % (BASE, policy, gamma, POWER, STEPSIZE, MAX_ITER, STEPVALUES[0], STEPVALUES[1]))
    for it in ITERS:
        if policy == "multistep":                            # current_step_ advances one stepvalue per call: walk there like training does
            s.iter_, s.current_step_ = 0, 0
            for k in range(it):
                s.iter_ = k
                s.GetLearningRate()
        s.iter_ = it
        got, want = s.GetLearningRate(), _closed_form(policy, it, gamma)
        assert got == float(np.float32(got))                  # a float32 value
        assert abs(got - want) <= TOL * abs(want), (policy, it, got, want)
        if policy == "step":
            assert s.current_step_ == it // STEPSIZE
    with pytest.raises(CheckError, match="Unknown learning rate policy"):
        _Sched('base_lr: 0.1 lr_policy: "cosine"').GetLearningRate()


def test_multistep_crosses_two_stepvalues_in_sequence():
    s = _Sched('base_lr: 0.01 lr_policy: "multistep" gamma: 0.5 stepvalue: 2 stepvalue: 5')
    steps, rates = [], []
    for it in range(8):
        s.iter_ = it
        rates.append(s.GetLearningRate())
        steps.append(s.current_step_)
    assert steps == [0, 0, 1, 1, 1, 2, 2, 2]
    b = float(np.float32(0.01))
    assert rates == [float(np.float32(b * 0.5 ** k)) for k in steps]


def test_adam_correction_against_fp64():
    s = _Sched('type: "Adam" momentum: 0.9 momentum2: 0.999 base_lr: 0.1 lr_policy: "fixed"')
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))            # the constants as the proto holds them
    for t in (1, 2, 1000):
        s.iter_ = t - 1
        got, want = s.AdamCorrection(), math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        assert got == float(np.float32(got)) and abs(got - want) <= TOL * want, (t, got, want)


TINY = """
name: "tiny"
input: "x" input_shape { dim: 1 dim: 2 dim: 4 dim: 4 }
layer { name: "c1" type: "Convolution" bottom: "x" top: "a" param { lr_mult: 1 decay_mult: 1 } param { lr_mult: 2 decay_mult: 0 }
        convolution_param { num_output: 3 kernel_size: 3 pad: 1 weight_filler { type: "gaussian" std: 0.1 } } }
layer { name: "c2" type: "Convolution" bottom: "a" top: "b" param { lr_mult: 0 } convolution_param { num_output: 2 kernel_size: 1 bias_term: false } }
"""
ADAM = 'type: "Adam" base_lr: 0.01 lr_policy: "multistep" gamma: 0.5 stepvalue: 2 stepvalue: 5 momentum: 0.9 snapshot_format: HDF5 snapshot_prefix: "%s"'


def _cpu_solver(prefix="s", text=ADAM):
    return fsolver.get_solver(SolverParameter(text % prefix), net=fnet.Net(TINY, phase="TRAIN", device="cpu"))


def test_snapshot_round_trip_and_history_order(tmp_path):
    s = _cpu_solver(str(tmp_path / "snap"))
    assert isinstance(s, fsolver.AdamSolver) and len(s.net.learnable_) == 3 and len(s.history_) == 6
    assert s.net.params_lr_ == [1.0, 2.0, 0.0] and s.net.params_decay_ == [1.0, 0.0, 1.0]
    g = torch.Generator().manual_seed(3)
    for k, h in enumerate(s.history_):                        # all m, then all v (AdamPreSolve appends the second set)
        h.copy_(torch.randn(h.shape, generator=g) + 10 * k)
    for it in range(4):                                      # walk the schedule to iteration 3: current_step_ = 1
        s.iter_ = it
        s.GetLearningRate()
    model, state = s.Snapshot()
    assert model == str(tmp_path / "snap_iter_3.caffemodel.h5") and state == str(tmp_path / "snap_iter_3.solverstate.h5")
    d = fsolver._read_h5_datasets(state)
    assert sorted(d) == ["/current_step", "/history/0", "/history/1", "/history/2", "/history/3", "/history/4", "/history/5", "/iter"]
    assert d["/iter"].shape == (1,) and d["/iter"][0] == 3 and d["/current_step"][0] == 1
    n = len(s.net.learnable_)
    for k in range(2 * n):
        assert d["/history/%d" % k].shape == tuple(s.net.learnable_[k % n].shape()) and np.array_equal(d["/history/%d" % k], s.history_[k].numpy())
        assert 10 * k - 6 < float(d["/history/%d" % k].mean()) < 10 * k + 6          # m of blob 0..n-1 first, then v of blob 0..n-1
    # the int32 datasets are what H5LTmake_dataset_int writes: fixed-point, 4 bytes, signed
    L = _lib.lib()
    import ctypes as C
    buf = np.frombuffer(open(state, "rb").read(), np.uint8)
    cnt = C.c_int()
    L.fn2_hdf5_index(C.c_void_p(buf.ctypes.data), buf.size, None, 0, C.byref(cnt))
    ents = (_lib.Hdf5Entry * cnt.value)()
    assert L.fn2_hdf5_index(C.c_void_p(buf.ctypes.data), buf.size, ents, cnt.value, C.byref(cnt)) == 0
    it_entry = [e for e in ents if e.path == b"/iter"][0]
    assert (it_entry.type_class, it_entry.type_size, it_entry.type_signed, it_entry.big_endian, it_entry.num_axes, it_entry.count) == (0, 4, 1, 0, 1, 1)
    # a fresh solver restores iteration, step, history and weights; current_step survives: the next rate is the restored schedule's
    fresh = _cpu_solver(str(tmp_path / "other"))
    fresh.Restore(state, model)
    assert fresh.iter_ == 3 and fresh.current_step_ == 1
    for a, b in zip(fresh.history_, s.history_):
        assert torch.equal(a, b)
    for a, b in zip(fresh.net.learnable_, s.net.learnable_):
        assert torch.equal(a.data, b.data)
    fresh.iter_ = 4
    assert fresh.GetLearningRate() == float(np.float32(float(np.float32(0.01)) * 0.5)) and fresh.current_step_ == 1
    # a wrong history length is refused (an SGD solver has 3 history blobs, the file 6)
    sgd = _cpu_solver(str(tmp_path / "sgd"), 'type: "SGD" base_lr: 0.01 lr_policy: "fixed" snapshot_format: HDF5 snapshot_prefix: "%s"')
    with pytest.raises(CheckError, match="Incorrect length of history blobs."):
        sgd.Restore(state)
    with pytest.raises(CheckError, match="only HDF5"):
        sgd.Restore(str(tmp_path / "x.solverstate"))
    with pytest.raises(CheckError, match="BINARYPROTO is not supported"):
        _cpu_solver(str(tmp_path / "b"), 'base_lr: 0.01 lr_policy: "fixed" snapshot_prefix: "%s"').Snapshot()


def test_h5write_bytes_for_weight_files_are_unchanged():
    """tests/golden/h5/tiny_h5write.caffemodel.h5 is what the writer produced for the layers of tests/golden/tiny_caffemodel.npz BEFORE it learned
    int32 scalars; the same call must give the same bytes."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "tiny_caffemodel.npz"))
    layers = [("img0s_aug", [z["img0s_aug.count"], z["img0s_aug.pixel_mean"], z["img0s_aug.mean"]]), ("conv1", [z["conv1.w"], z["conv1.b"]]),
              ("deconv5", [z["deconv5.w"], z["deconv5.b"]]), ("net2_conv6", [z["net2_conv6.w"], z["net2_conv6.b"].reshape(2)]), ("fuse_conv0", [z["fuse_conv0.w"]])]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "w.h5")
        _h5write.write(path, {"data": {n: {str(j): np.ascontiguousarray(b, np.float32) for j, b in enumerate(bl)} for n, bl in layers}})
        got = open(path, "rb").read()
    assert got == open(os.path.join(ROOT, "tests", "golden", "h5", "tiny_h5write.caffemodel.h5"), "rb").read()


def test_test_fields_are_ignored_with_one_warning_and_train_net_comes_from_the_param(tmp_path):
    (tmp_path / "train.prototxt").write_text(TINY)
    (tmp_path / "solver.prototxt").write_text('net: "train.prototxt" base_lr: 0.1 lr_policy: "fixed" test_iter: 5 test_interval: 100\n')
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        s = flownet2_amd.Solver(str(tmp_path / "solver.prototxt"), device="cpu")
    assert len([x for x in w if "test nets are not implemented" in str(x.message)]) == 1
    assert s.net.phase_ == "TRAIN" and s.net.name_ == "tiny" and isinstance(s, fsolver.Solver)
    inline = fsolver.get_solver(SolverParameter('base_lr: 0.1 lr_policy: "fixed" net_param { %s }' % TINY), device="cpu")
    assert isinstance(inline, fsolver.SGDSolver) and inline.net.layer_names == ["c1", "c2"] and len(inline.history_) == 3
    with pytest.raises(CheckError, match="must specify a train net"):
        fsolver.get_solver(SolverParameter('base_lr: 0.1 lr_policy: "fixed"'), device="cpu")
    with pytest.raises(CheckError, match="more than one"):
        fsolver.get_solver(SolverParameter('net: "a" train_net: "b"'), device="cpu")
    with pytest.raises(CheckError, match="built with a SolverParameter of type SGD"):
        fsolver.AdamSolver(SolverParameter('base_lr: 0.1'), net=s.net)


def test_apply_update_on_a_cpu_net_has_no_fallback():
    s = _cpu_solver()
    with pytest.raises(ValueError, match="no CPU path"):
        s.ApplyUpdate()
    opt = fsolver.CaffeOptimizer([torch.zeros(3, requires_grad=True)], SolverParameter('base_lr: 0.1 lr_policy: "fixed"'))
    opt._flat[0].grad = torch.ones(3)
    with pytest.raises(ValueError, match="no CPU path"):
        opt.step()


def test_table_geometry_and_refusals_are_host_logic():
    """fn2_solver_table_bytes and every refusal are decided before anything touches the device: made-up addresses are never read."""
    import ctypes as C
    L = _lib.lib()
    chunk = flownet2_amd.ops.SOLVER_CHUNK
    counts = [1, chunk, chunk + 1, 3 * chunk]
    blobs = (_lib.SolverBlob * 4)(*[_lib.SolverBlob(0x1000 * (k + 1), 0x2000 * (k + 1) + 4, 0x4000 * (k + 1) + 8, None, n, 1.0, 1.0) for k, n in enumerate(counts)])
    nchunks = 1 + 1 + 2 + 3
    assert L.fn2_solver_table_bytes(4, blobs) == 64 + 48 * 4 + 16 * nchunks + 8 * nchunks          # header, descriptors, chunk list, clip partials
    blobs[2].count = 0
    assert L.fn2_solver_table_bytes(4, blobs) == 0 and b"blob 2 has count 0" in L.fn2_last_error_string()
    blobs[2].count = counts[2]
    blobs[3].hist0 = 0x4002
    info = _lib.SolverTableInfo()
    assert L.fn2_solver_table_build(4, blobs, C.c_void_p(0x100000), 1 << 20, C.byref(info), None) == -1 and b"not 4-byte aligned" in L.fn2_last_error_string()
    blobs[3].hist0 = 0x4000
    assert L.fn2_solver_table_build(4, blobs, C.c_void_p(0x100000), 100, C.byref(info), None) == -3 and b"needed" in L.fn2_last_error_string()
    p = flownet2_amd.ops.solver_params(type=5)
    info = _lib.SolverTableInfo(4, 0, nchunks, 0)
    assert L.fn2_solver_apply_update(C.byref(p), C.c_void_p(0x100000), C.byref(info), 0.1, 1.0, 0, None) == -1 and b"unknown solver type 5" in L.fn2_last_error_string()
    p = flownet2_amd.ops.solver_params(type=flownet2_amd.ops.SOLVER_ADAM)
    assert L.fn2_solver_apply_update(C.byref(p), C.c_void_p(0x100000), C.byref(info), 0.1, 1.0, 0, None) == -1 and b"Adam needs hist1" in L.fn2_last_error_string()
