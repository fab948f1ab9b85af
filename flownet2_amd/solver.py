"""The Solver: what `caffe train --solver=...` does around the net, for SGD and Adam, on one HIP update kernel.

    SolverParameter          src/caffe/proto/caffe.proto:104-244     every field, with the proto's defaults; floats are held as float32
    Solver::Step             src/caffe/solver.cpp:193-275            ClearParamDiffs, callbacks on_start, iter_size x ForwardBackward, the
                                                                     loss / iter_size, UpdateSmoothedLoss (:483-495), callbacks
                                                                     on_gradients_ready, ApplyUpdate, ++iter, Snapshot
    SGDSolver::GetLearningRate  solvers/sgd_solver.cpp:26-63         fixed, step, exp, inv, multistep, poly, sigmoid (current_step_ kept)
    SGDSolver::ApplyUpdate   sgd_solver.cpp:101-116                  ClipGradients (:80-99), then per blob Normalize (:118-142), Regularize
                                                                     (:144-204), ComputeUpdateValue (sgd_solver.cu / adam_solver.cpp:25-89,
                                                                     adam_solver.cu:7-15), then Net::Update: ONE fn2_solver_apply_update
                                                                     (csrc/solver_update.hip) over a device-resident table of all blobs
    Snapshot / Restore       solver.cpp:395-481, sgd_solver.cpp:278-347   HDF5 only: <prefix>_iter_<N>.caffemodel.h5 (Net::ToHDF5) and
                                                                     <prefix>_iter_<N>.solverstate.h5 (iter, current_step, history/0..n-1)

What differs from the reference, all of it on purpose:
  * the learning rate and Adam's correction are evaluated in double from the float32 parameters and rounded to float32 ONCE (the reference
    evaluates them in float through powf / expf: a few units in the last place apart);
  * the clip norm is summed in fp64 in a fixed order on the device and never read back, so there is no "Gradient clipping" log line;
  * update_ / temp_ blobs do not exist; the diff holds the update value afterwards only with write_update=True (the reference always
    leaves it there; nothing reads it before the next ClearParamDiffs);
  * test nets and TestAll are out of scope: test_* fields are accepted and ignored with one warning;
  * only SGD and Adam; Nesterov, AdaGrad, RMSProp and AdaDelta raise a CheckError that says so; only snapshot_format: HDF5;
  * `learned_net` is not written into the solver state (the reference's Restore treats it as optional): pass the weights file to Restore.
There is no CPU path: ApplyUpdate on a CPU net raises the package's ValueError.
"""
from __future__ import annotations

import logging
import math
import os
import warnings
from collections import OrderedDict
from typing import Any, Callable, Dict, List, Optional

import numpy as np
import torch

from . import ops, prototxt
from .layers import CHECK, CheckError  # noqa: F401  (CheckError: what this module raises)

log = logging.getLogger("flownet2_amd.solver")

# ---- SolverParameter ---------------------------------------------------------------------------------------------------------------
# name -> (kind, default); default None = the proto declares none (has_<field>() is false until it is set)
_FIELDS: "OrderedDict[str, tuple]" = OrderedDict([
    ("net", ("string", None)), ("net_param", ("message", None)), ("train_net", ("string", None)), ("test_net", ("rstring", None)),
    ("train_net_param", ("message", None)), ("test_net_param", ("rmessage", None)), ("train_state", ("message", None)),
    ("test_state", ("rmessage", None)), ("test_iter", ("rint", None)), ("test_interval", ("int", 0)), ("test_compute_loss", ("bool", False)),
    ("test_initialization", ("bool", True)), ("base_lr", ("float", None)), ("display", ("int", None)), ("average_loss", ("int", 1)),
    ("max_iter", ("int", None)), ("iter_size", ("int", 1)), ("lr_policy", ("string", None)), ("gamma", ("float", None)),
    ("power", ("float", None)), ("momentum", ("float", None)), ("weight_decay", ("float", None)), ("regularization_type", ("string", "L2")),
    ("stepsize", ("int", None)), ("stepvalue", ("rint", None)), ("clip_gradients", ("float", -1.0)), ("snapshot", ("int", 0)),
    ("snapshot_prefix", ("string", None)), ("snapshot_diff", ("bool", False)), ("snapshot_format", ("enum", "BINARYPROTO")),
    ("solver_mode", ("enum", "GPU")), ("device_id", ("int", 0)), ("random_seed", ("int", -1)), ("type", ("string", "SGD")),
    ("delta", ("float", 1e-8)), ("momentum2", ("float", 0.999)), ("rms_decay", ("float", None)), ("debug_info", ("bool", False)),
    ("snapshot_after_train", ("bool", True)), ("solver_type", ("enum", "SGD")),
])
_ENUMS = {"snapshot_format": ("HDF5", "BINARYPROTO"), "solver_mode": ("CPU", "GPU"),
          "solver_type": ("SGD", "NESTEROV", "ADAGRAD", "RMSPROP", "ADADELTA", "ADAM")}
_SOLVER_TYPE_TO_TYPE = {"SGD": "SGD", "NESTEROV": "Nesterov", "ADAGRAD": "AdaGrad", "RMSPROP": "RMSProp", "ADADELTA": "AdaDelta", "ADAM": "Adam"}
_MESSAGE_PARENT = {"net_param": "", "train_net_param": "", "test_net_param": "", "train_state": "state", "test_state": "state"}
_TEST_FIELDS = ("test_net", "test_net_param", "test_state", "test_iter", "test_interval", "test_compute_loss", "test_initialization")
KNOWN_TYPES = ("SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta", "Adam")
IMPLEMENTED_TYPES = ("SGD", "Adam")


def _f32(x) -> float:
    """A proto `float` field: the value as float32 holds it."""
    return float(np.float32(x))


def _dict_to_message(d: Dict[str, Any]) -> prototxt.Message:
    m = prototxt.Message()
    for k, v in d.items():
        for item in (v if isinstance(v, (list, tuple)) else [v]):
            m.add(k, _dict_to_message(item) if isinstance(item, dict) else item)
    return m


def _scalar_text(v) -> str:
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, prototxt.Enum):
        return str(v)
    if isinstance(v, str):
        return '"' + v.replace("\\", "\\\\").replace('"', '\\"').replace("\n", "\\n") + '"'
    if isinstance(v, float):
        return "inf" if v == math.inf else "-inf" if v == -math.inf else "nan" if v != v else repr(v)
    return str(v)


def message_to_text(m: prototxt.Message, indent: int = 0) -> str:
    """A prototxt.Message back to text format (what prototxt.parse reads)."""
    pad, out = "  " * indent, []
    for k, v in m.fields:
        if isinstance(v, prototxt.Message):
            out.append("%s%s {\n%s%s}\n" % (pad, k, message_to_text(v, indent + 1), pad))
        else:
            out.append("%s%s: %s\n" % (pad, k, _scalar_text(v)))
    return "".join(out)


class SolverParameter:
    """`message SolverParameter` (caffe.proto:104-244).  Built from a solver prototxt (a path, or the text itself), a prototxt.Message, a
    dict {field: value} (repeated fields as lists, sub-messages as dicts or prototxt text), or another SolverParameter.  Every field is an
    attribute holding the value or the proto's default (None where the proto declares none); `has(field)` tells whether it was set.
    `float` fields hold the float32 value.  The deprecated `solver_type` enum maps to `type` (upgrade_proto.cpp:UpgradeSolverType).
    Unknown fields raise CheckError."""

    def __init__(self, source=None, **fields):
        self._set: Dict[str, Any] = OrderedDict()
        self.source_dir_: Optional[str] = None
        if isinstance(source, SolverParameter):
            self._set = OrderedDict(source._set)
            self.source_dir_ = source.source_dir_
        elif isinstance(source, prototxt.Message):
            self._from_message(source)
        elif isinstance(source, dict):
            self._from_message(_dict_to_message(source))
        elif isinstance(source, str):
            text = source
            if source.strip() and "\n" not in source and ":" not in source and "{" not in source:
                CHECK(os.path.exists(source), f"Failed to parse SolverParameter file: {source}")             # upgrade_proto.cpp:ReadSolverParamsFromTextFileOrDie
                self.source_dir_ = os.path.dirname(os.path.abspath(source))
                with open(source) as f:
                    text = f.read()
            self._from_message(prototxt.parse(text))
        else:
            CHECK(source is None, f"SolverParameter: cannot be built from {type(source).__name__}")
        if fields:
            self._from_message(_dict_to_message(fields))
        if "solver_type" in self._set:                                                                     # upgrade_proto.cpp:UpgradeSolverType
            CHECK("type" not in self._set, "Failed to upgrade solver: old solver_type field (enum) and new type field (string) cannot be both "
                                            "specified in solver proto text.")
            self._set["type"] = _SOLVER_TYPE_TO_TYPE[self._set.pop("solver_type")]
        CHECK(self.type in KNOWN_TYPES, f"Unknown solver type: {self.type} (known types: {', '.join(KNOWN_TYPES)})")     # solver_factory.hpp:75-79

    def _convert(self, name: str, kind: str, v):
        kind = kind[1:] if kind in ("rstring", "rint", "rmessage") else kind
        if kind == "message":
            if isinstance(v, str):
                v = prototxt.parse(v)
            CHECK(isinstance(v, prototxt.Message), f"SolverParameter.{name}: expected a message")
            return v
        CHECK(not isinstance(v, prototxt.Message), f"SolverParameter.{name}: expected a {kind}, got a message")
        if kind == "string":
            CHECK(isinstance(v, str) and not isinstance(v, prototxt.Enum), f"SolverParameter.{name}: expected a string, got {v!r}")
            return str(v)
        if kind == "enum":
            names = _ENUMS[name]
            if isinstance(v, int) and not isinstance(v, bool) and 0 <= v < len(names):
                v = names[v]
            CHECK(str(v) in names, f"SolverParameter.{name}: unknown enumeration value {v!r}")
            return str(v)
        if kind == "bool":
            CHECK(isinstance(v, bool) or v in (0, 1), f"SolverParameter.{name}: expected a bool, got {v!r}")
            return bool(v)
        CHECK(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool), f"SolverParameter.{name}: expected a number, got {v!r}")
        if kind == "int":
            CHECK(float(v) == int(v), f"SolverParameter.{name}: expected an integer, got {v!r}")
            return int(v)
        return _f32(v)

    def _from_message(self, m: prototxt.Message):
        for key in m.keys():
            CHECK(key in _FIELDS, f"Error parsing text-format caffe.SolverParameter: Message type \"caffe.SolverParameter\" has no field named \"{key}\".")
            kind = _FIELDS[key][0]
            vals = [self._convert(key, kind, v) for v in m.all(key)]
            if kind in ("rstring", "rint", "rmessage"):
                self._set[key] = list(self._set.get(key, [])) + vals
            else:
                self._set[key] = vals[-1]                                     # a singular field set twice: the last one wins

    def has(self, name: str) -> bool:
        return name in self._set

    def __getattr__(self, name: str):
        if name.startswith("_") or name not in _FIELDS:
            raise AttributeError(name)
        kind, default = _FIELDS[name]
        if name in self._set:
            return self._set[name]
        if kind in ("rstring", "rint", "rmessage"):
            return []
        return _f32(default) if kind == "float" and default is not None else default

    def to_dict(self) -> Dict[str, Any]:
        """The fields that were set: messages as plain dicts (prototxt.to_dict)."""
        def plain(name, v):
            return prototxt.to_dict(v, _MESSAGE_PARENT[name]) if isinstance(v, prototxt.Message) else v
        return OrderedDict((k, [plain(k, x) for x in v] if isinstance(v, list) else plain(k, v)) for k, v in self._set.items())

    def to_prototxt(self) -> str:
        m = prototxt.Message()
        for k, v in self._set.items():
            for item in (v if isinstance(v, list) else [v]):
                m.add(k, prototxt.Enum(item) if _FIELDS[k][0] == "enum" else item)
        return message_to_text(m)

    def __eq__(self, other):
        return isinstance(other, SolverParameter) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return "SolverParameter(%s)" % ", ".join("%s=%r" % kv for kv in self.to_dict().items())


# ---- rate and iteration bookkeeping (shared by Solver and CaffeOptimizer) -------------------------------------------------------
class _Schedule:
    """iter_, current_step_ and what depends on them.  Parameters are float32 (the proto's `float`); every formula is evaluated in double
    and rounded to float32 once."""

    param_: SolverParameter
    iter_: int
    current_step_: int

    def _init_schedule(self, param: SolverParameter):
        self.param_ = param
        self.iter_ = 0
        self.current_step_ = 0
        self._table = None                  # ops.SolverTable of the tensors last stepped
        self.table_builds_ = 0
        CHECK(param.type in IMPLEMENTED_TYPES, f"Solver type {param.type} is not implemented (implemented: {', '.join(IMPLEMENTED_TYPES)})")
        CHECK(param.regularization_type in ("L2", "L1"), f"Unknown regularization type: {param.regularization_type}")        # sgd_solver.cpp:170
        CHECK(param.iter_size >= 1, "iter_size must be >= 1")

    def GetLearningRate(self) -> float:
        """SGDSolver::GetLearningRate, sgd_solver.cpp:26-63.  `step` and `multistep` update current_step_ as the reference does."""
        p, it = self.param_, self.iter_
        policy = p.lr_policy
        need = {"fixed": (), "step": ("gamma", "stepsize"), "exp": ("gamma",), "inv": ("gamma", "power"), "multistep": ("gamma",),
                "poly": ("power", "max_iter"), "sigmoid": ("gamma", "stepsize")}
        CHECK(policy in need, f"Unknown learning rate policy: {policy}")
        base = float(p.base_lr if p.base_lr is not None else 0.0)
        v = {k: (getattr(p, k) if getattr(p, k) is not None else 0) for k in need[policy]}       # an unset proto field reads as 0
        if policy == "fixed":
            rate = base
        elif policy == "step":
            CHECK(v["stepsize"] > 0, "lr_policy \"step\" needs stepsize > 0")
            self.current_step_ = it // v["stepsize"]
            rate = base * math.pow(v["gamma"], self.current_step_)
        elif policy == "exp":
            rate = base * math.pow(v["gamma"], it)
        elif policy == "inv":
            rate = base * math.pow(1.0 + v["gamma"] * it, -v["power"])
        elif policy == "multistep":
            sv = p.stepvalue
            if self.current_step_ < len(sv) and it >= sv[self.current_step_]:
                self.current_step_ += 1
                log.info("MultiStep Status: Iteration %d, step = %d", it, self.current_step_)
            rate = base * math.pow(v["gamma"], self.current_step_)
        elif policy == "poly":
            CHECK(v["max_iter"] > 0, "lr_policy \"poly\" needs max_iter > 0")
            rate = base * math.pow(1.0 - it / float(v["max_iter"]), v["power"])
        else:
            rate = base * (1.0 / (1.0 + math.exp(-v["gamma"] * (it - v["stepsize"]))))
        return _f32(rate)

    def AdamCorrection(self) -> float:
        """sqrt(1 - beta2^t) / (1 - beta1^t) with t = iter + 1 (adam_solver.cpp:39-41)."""
        t = self.iter_ + 1
        b1, b2 = float(self._momentum()), float(self.param_.momentum2)
        return _f32(math.sqrt(1.0 - math.pow(b2, t)) / (1.0 - math.pow(b1, t)))

    def _momentum(self) -> float:
        return self.param_.momentum if self.param_.momentum is not None else 0.0

    def _update_params(self):
        p = self.param_
        return ops.solver_params(type=ops.SOLVER_ADAM if p.type == "Adam" else ops.SOLVER_SGD,
                                 regularization=ops.SOLVER_REG_L1 if p.regularization_type == "L1" else ops.SOLVER_REG_L2,
                                 momentum=self._momentum(), momentum2=p.momentum2, delta=p.delta,
                                 weight_decay=p.weight_decay if p.weight_decay is not None else 0.0, clip_gradients=p.clip_gradients,
                                 accum_normalization=_f32(1.0 / p.iter_size))

    def _apply(self, data, diff, hist, lr_mults, decay_mults, write_update: bool):
        """One fn2_solver_apply_update over (data, diff, hist); the table is rebuilt only when a tensor has moved."""
        for t in list(data) + list(diff):
            if not t.is_cuda:
                raise ValueError("Solver.ApplyUpdate: expected CUDA (HIP) tensors; flownet2_amd has no CPU path")
        n = len(data)
        h0, h1 = hist[:n], (hist[n:] if self.param_.type == "Adam" else None)
        table = self._table
        if table is None or not table.matches(data, diff, h0, h1):
            table = self._table = ops.SolverTable(data, diff, h0, h1, lr_mults, decay_mults)
            self.table_builds_ += 1
        rate = self.GetLearningRate()
        correction = self.AdamCorrection() if self.param_.type == "Adam" else 1.0
        ops.solver_apply_update(table, self._update_params(), rate, correction, write_update)
        return rate


def _read_h5_datasets(path: str) -> "OrderedDict[str, np.ndarray]":
    """{"/path/of/dataset": float32 array} of an HDF5 file, through the package's reader (integers come back as float32: exact below 2^24)."""
    import ctypes as C
    from . import _lib
    from .caffemodel import _check
    with open(path, "rb") as f:
        buf = np.frombuffer(f.read(), dtype=np.uint8)
    L = _lib.lib()
    ptr, n = C.c_void_p(buf.ctypes.data), C.c_int()
    _check(L.fn2_hdf5_index(ptr, buf.size, None, 0, C.byref(n)))
    entries = (_lib.Hdf5Entry * max(1, n.value))()
    _check(L.fn2_hdf5_index(ptr, buf.size, entries, n.value, C.byref(n)))
    out = OrderedDict()
    for i in range(n.value):
        e = entries[i]
        arr = np.empty(e.count, np.float32)
        _check(L.fn2_hdf5_read_float(ptr, buf.size, C.byref(e), arr.ctypes.data_as(C.c_void_p), arr.size))
        out[e.path.decode("utf-8")] = arr.reshape(tuple(int(e.dim[k]) for k in range(e.num_axes)))
    return out


def write_solverstate_h5(path: str, iter_: int, current_step: int, history: List[np.ndarray]) -> None:
    """SGDSolver::SnapshotSolverStateToHDF5 (sgd_solver.cpp:278-302) without `learned_net`: int32 datasets `iter` and `current_step`, group
    `history` with datasets "0" .. "n-1" (Adam: all first moments, then all second moments, as AdamPreSolve appends them)."""
    from . import _h5write
    _h5write.write(path, {"iter": _h5write.IntScalar(iter_), "current_step": _h5write.IntScalar(current_step),
                          "history": {str(i): np.ascontiguousarray(h, np.float32) for i, h in enumerate(history)}})


def read_solverstate_h5(path: str):
    """-> (iter, current_step, [history arrays in index order]).  `iter` and `current_step` pass through the float32 reader: exact below
    2^24 (16.7 M iterations; the authors' longest schedule is 1.2 M)."""
    d = _read_h5_datasets(path)
    CHECK("/iter" in d and "/current_step" in d, f"Failed to load int dataset with name iter / current_step from {path}")     # hdf5.cpp:150-156
    hist = {k[len("/history/"):]: v for k, v in d.items() if k.startswith("/history/")}
    CHECK(all(k.isdigit() for k in hist), f"Error reading history from {path}")
    history = []
    while str(len(history)) in hist:
        history.append(hist[str(len(history))])
    return int(d["/iter"].ravel()[0]), int(d["/current_step"].ravel()[0]), history, len(hist)


# ---- Solver --------------------------------------------------------------------------------------------------------------------------
class Solver(_Schedule):
    """Solver<float> + SGDSolver<float> for the types this package implements.  `net`: a flownet2_amd.net.Net built for TRAIN; without
    one the train net comes from net / train_net / net_param / train_net_param (solver.cpp:InitTrainNet) with phase TRAIN on `device`."""

    solver_type: Optional[str] = None

    def __init__(self, param, net=None, device=None, write_update: bool = False, extra_layers=()):
        """extra_layers: handed on to the train net this solver builds (Net(..., extra_layers=...))."""
        param = param if isinstance(param, SolverParameter) else SolverParameter(param)
        self.extra_layers_ = tuple(extra_layers)
        self._init_schedule(param)
        CHECK(self.solver_type is None or param.type == self.solver_type, f"{type(self).__name__} built with a SolverParameter of type {param.type}")
        self.write_update_ = bool(write_update)
        self.callbacks_: List[Any] = []
        self.losses_: List[np.float32] = []
        self.smoothed_loss_ = np.float32(0)
        ignored = [f for f in _TEST_FIELDS if param.has(f)]
        if ignored:
            warnings.warn("Solver: test nets are not implemented; ignoring " + ", ".join(ignored), stacklevel=2)
        self.net_ = net if net is not None else self._init_train_net(device)
        self._pre_solve()

    net = property(lambda self: self.net_)
    iter = property(lambda self: self.iter_)
    param = property(lambda self: self.param_)
    smoothed_loss = property(lambda self: float(self.smoothed_loss_))

    def _init_train_net(self, device):
        """Solver::InitTrainNet, solver.cpp:76-117: exactly one of the four fields; phase TRAIN, then train_state's level / stages."""
        from .net import Net
        p = self.param_
        given = [f for f in ("net", "net_param", "train_net", "train_net_param") if p.has(f)]
        CHECK(len(given) >= 1, "SolverParameter must specify a train net using one of these fields: net, net_param, train_net, train_net_param")
        CHECK(len(given) == 1, "SolverParameter must not contain more than one of these fields specifying a train_net: " + ", ".join(given))
        v = getattr(p, given[0])
        if isinstance(v, prototxt.Message):
            text = message_to_text(v)
        else:
            path = v if os.path.exists(v) or p.source_dir_ is None else os.path.join(p.source_dir_, v)
            CHECK(os.path.exists(path), f"Failed to parse NetParameter file: {v}")
            with open(path) as f:
                text = f.read()
        st = prototxt.to_dict(p.train_state, "state") if p.has("train_state") else {}
        return Net(text, phase="TRAIN", device=device, level=int(st.get("level", 0)), stages=tuple(st.get("stage", [])),
                   extra_layers=self.extra_layers_)

    def _pre_solve(self):
        """SGDSolver::PreSolve (sgd_solver.cpp:65-78) and AdamPreSolve (adam_solver.cpp:7-17): history_ = one zero blob per learnable blob,
        Adam appends a second set.  update_ and temp_ are not allocated."""
        copies = 2 if self.param_.type == "Adam" else 1
        self.history_: List[torch.Tensor] = [torch.zeros_like(b.data) for _ in range(copies) for b in self.net_.learnable_]

    def add_callback(self, cb):
        """Solver::add_callback (solver.hpp:82-84): an object with on_start() and on_gradients_ready()."""
        self.callbacks_.append(cb)

    def ApplyUpdate(self):
        net = self.net_
        data = [b.data for b in net.learnable_]
        diff = [b.mutable_gpu_diff() for b in net.learnable_]
        with torch.no_grad():
            rate = self._apply(data, diff, self.history_, net.params_lr_, net.params_decay_, self.write_update_)
        if self.param_.display and self.iter_ % self.param_.display == 0:
            log.info("Iteration %d, lr = %g", self.iter_, rate)
        for layer in net.layers:
            if hasattr(layer, "note_weights_changed"):
                layer.note_weights_changed()

    def _update_smoothed_loss(self, loss, start_iter: int):                                               # solver.cpp:483-495
        average_loss = self.param_.average_loss
        if len(self.losses_) < average_loss:
            self.losses_.append(loss)
            size = len(self.losses_)
            self.smoothed_loss_ = np.float32((self.smoothed_loss_ * np.float32(size - 1) + loss) / np.float32(size))
        else:
            idx = (self.iter_ - start_iter) % average_loss
            self.smoothed_loss_ = np.float32(self.smoothed_loss_ + (loss - self.losses_[idx]) / np.float32(average_loss))
            self.losses_[idx] = loss

    def Step(self, iters: int, inputs: Optional[Callable[[], Dict[str, Any]]] = None):
        """Solver::Step, solver.cpp:193-275.  `inputs`: a callable that returns the feed dict of ONE ForwardBackward pass (called iter_size
        times per iteration), or None for a net with a data layer.  The loss of every pass is read back, as the reference does."""
        start_iter, stop_iter = self.iter_, self.iter_ + int(iters)
        self.losses_ = []
        self.smoothed_loss_ = np.float32(0)
        p = self.param_
        while self.iter_ < stop_iter:
            if hasattr(self.net_, "set_iter"):
                self.net_.set_iter(self.iter_)                                                            # solver.cpp:202
            self.net_.ClearParamDiffs()
            for cb in self.callbacks_:
                cb.on_start()
            loss = np.float32(0)
            for _ in range(p.iter_size):
                l = self.net_.ForwardBackward(**(inputs() if inputs is not None else {}))
                loss = np.float32(loss + np.float32(float(l) if l is not None else 0.0))
            loss = np.float32(loss / np.float32(p.iter_size))
            self._update_smoothed_loss(loss, start_iter)
            if p.display and self.iter_ % p.display == 0:
                log.info("Iteration %d, loss = %g", self.iter_, float(self.smoothed_loss_))
            for cb in self.callbacks_:
                cb.on_gradients_ready()
            self.ApplyUpdate()
            self.iter_ += 1
            if p.snapshot and self.iter_ % p.snapshot == 0:
                self.Snapshot()

    def Solve(self, inputs=None):
        """Solver::Solve without the test passes: Step(max_iter - iter), then the final snapshot (solver.cpp:277-325)."""
        CHECK(self.param_.max_iter is not None, "Solve needs max_iter")
        self.Step(self.param_.max_iter - self.iter_, inputs)
        p = self.param_
        if p.snapshot_after_train and (not p.snapshot or self.iter_ % p.snapshot != 0):
            self.Snapshot()

    def SnapshotFilename(self, extension: str) -> str:                                                 # solver.cpp:447-451
        return "%s_iter_%d%s" % (self.param_.snapshot_prefix or "", self.iter_, extension)

    def Snapshot(self):
        """Solver::Snapshot (solver.cpp:395-420) for snapshot_format: HDF5 -> (weights path, state path).  Layers without parameter blobs
        get no group in the weights file (the reference writes an empty one); the writer holds at most 256 links per group, which
        bounds the history at 256 blobs (128 learnable blobs under Adam)."""
        CHECK(self.param_.snapshot_format == "HDF5", "snapshot_format: BINARYPROTO is not supported: set snapshot_format: HDF5")
        from .caffemodel import write_caffemodel_h5
        model = self.SnapshotFilename(".caffemodel.h5")
        write_caffemodel_h5(model, OrderedDict((name, [b.data.detach().cpu().numpy() for b in blobs]) for name, blobs in self.net_.params().items()))
        state = self.SnapshotFilename(".solverstate.h5")
        write_solverstate_h5(state, self.iter_, self.current_step_, [h.detach().cpu().numpy() for h in self.history_])
        log.info("Snapshotting to HDF5 file %s, solver state to %s", model, state)
        return model, state

    def Restore(self, state_path: str, weights_path: Optional[str] = None):
        """Solver::Restore -> RestoreSolverStateFromHDF5 (solver.cpp:471-481, sgd_solver.cpp:324-347).  The state file carries no
        `learned_net`: give the weights file here (or load it into the net yourself).  `iter` and `current_step` are read through the
        package's HDF5 reader, which returns float32: exact below 2^24 iterations."""
        CHECK(len(state_path) >= 3 and state_path.endswith(".h5"), "only HDF5 solver states (*.solverstate.h5) are supported")
        it, step, history, links = read_solverstate_h5(state_path)
        CHECK(links == len(self.history_) and len(history) == links, "Incorrect length of history blobs.")                    # sgd_solver.cpp:337-338
        if weights_path is not None:
            self.net_.CopyTrainedLayersFrom(weights_path)
        self.iter_, self.current_step_ = it, step
        with torch.no_grad():
            for dst, src in zip(self.history_, history):
                CHECK(src.size == dst.numel(), "Incorrect length of history blobs.")
                dst.copy_(torch.from_numpy(src.reshape(tuple(dst.shape))))


class SGDSolver(Solver):
    solver_type = "SGD"


class AdamSolver(Solver):
    solver_type = "Adam"


_SOLVERS = {"SGD": SGDSolver, "Adam": AdamSolver}


def get_solver(param, net=None, device=None, **kw) -> Solver:
    """SolverRegistry::CreateSolver (solver_factory.hpp:71-80) by `type`."""
    param = param if isinstance(param, SolverParameter) else SolverParameter(param)
    CHECK(param.type in _SOLVERS, f"Solver type {param.type} is not implemented (implemented: {', '.join(IMPLEMENTED_TYPES)})")
    return _SOLVERS[param.type](param, net=net, device=device, **kw)


# ---- the same update for the nets.py + autograd path -----------------------------------------------------------------------------
class CaffeOptimizer(torch.optim.Optimizer, _Schedule):
    """The solver's update as a torch.optim.Optimizer over plain tensors and their .grad: the same table and kernel, the same rate and
    iteration bookkeeping (`iter_`, `current_step_`, GetLearningRate()).  lr_mults / decay_mults: one per parameter (default 1), the
    ParamSpec multipliers of the prototxt.  The caller accumulates iter_size backward passes into .grad before step().  Being a
    torch.optim.Optimizer, its step() fires the global post-step hook of flownet2_amd.functional, so packed-operand caches follow."""

    def __init__(self, params, solver_param, lr_mults=None, decay_mults=None, write_update: bool = False):
        param = solver_param if isinstance(solver_param, SolverParameter) else SolverParameter(solver_param)
        self._init_schedule(param)
        torch.optim.Optimizer.__init__(self, params, {})
        self._flat = [p for g in self.param_groups for p in g["params"]]
        n = len(self._flat)
        self.lr_mults_ = [1.0] * n if lr_mults is None else [float(v) for v in lr_mults]
        self.decay_mults_ = [1.0] * n if decay_mults is None else [float(v) for v in decay_mults]
        CHECK(len(self.lr_mults_) == n and len(self.decay_mults_) == n, "CaffeOptimizer: one lr_mult and one decay_mult per parameter")
        self.write_update_ = bool(write_update)
        copies = 2 if param.type == "Adam" else 1
        self.history_ = [torch.zeros_like(p, memory_format=torch.contiguous_format) for _ in range(copies) for p in self._flat]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        CHECK(all(p.grad is not None for p in self._flat), "CaffeOptimizer.step: a parameter has no .grad (every blob of the table is updated)")
        self._apply([p.detach() for p in self._flat], [p.grad for p in self._flat], self.history_, self.lr_mults_, self.decay_mults_,
                    self.write_update_)
        self.iter_ += 1
        return loss
