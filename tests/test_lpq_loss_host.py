"""LpqLoss, everything that needs no GPU: the schedule, the host-only entry points and refusals of include/flownet2_hip_lpq_loss.h, the
references of lpq_ref against each other, the opt-in registration of the layer and the iteration a Solver hands its net."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lpq_cases as LC
import lpq_ref as LR
import flownet2_amd
from flownet2_amd import _lib, layers, lpq_schedule, solver as fsolver
from flownet2_amd import net as fnet
from flownet2_amd.solver import SolverParameter

TRAIN_NET = """
name: "lpq_tiny"
input: "img" input_shape { dim: 2 dim: 3 dim: 6 dim: 8 }
input: "gt" input_shape { dim: 2 dim: 2 dim: 6 dim: 8 }
layer { name: "conv" type: "Convolution" bottom: "img" top: "flow"
        convolution_param { num_output: 2 kernel_size: 3 pad: 1 weight_filler { type: "gaussian" std: 0.1 } } }
layer { name: "loss" type: "LpqLoss" bottom: "flow" bottom: "gt" top: "loss" loss_weight: 1
        lpq_loss_param { pq_episode_starts_at_iter: 0 pq_episode_starts_at_iter: 1 p: 1 p: 2 q: 1 q: 0.2 normalize_by_num_entries: true } }
"""


# ---- LpqSchedule ------------------------------------------------------------------------------------------------------------------
def test_schedule_is_exported_and_constant_without_a_start():
    assert flownet2_amd.LpqSchedule is lpq_schedule.LpqSchedule and "LpqSchedule" in flownet2_amd.__all__
    s = flownet2_amd.LpqSchedule((), [2.0], [0.2])
    assert s.starts == (0,) and [s.at(i) for i in (0, 1, 10 ** 9)] == [(2.0, 0.2)] * 3


@pytest.mark.parametrize("args, message", [
    (([0, 10], [1.0], [1.0, 2.0]), r"Incompatible sizes: \(pq_episode_starts_at_iter -> 2, p -> 1, q -> 2\)"),
    (([0], [1.0, 2.0], [1.0, 2.0]), r"Incompatible sizes: \(pq_episode_starts_at_iter -> 1, p -> 2, q -> 2\)"),
    (([], [1.0, 2.0], [1.0, 2.0]), r"Incompatible sizes: \(pq_episode_starts_at_iter -> 0, p -> 2, q -> 2\)"),
    (([], [], []), "Lpq schedule parameters must not be empty"),
    (([0, 10, 10], [1, 2, 3], [1, 2, 3]), "pq_episode_starts_at_frame is not ordered or contains duplicates: 0 10 10"),
    (([0, 20, 10], [1, 2, 3], [1, 2, 3]), "pq_episode_starts_at_frame is not ordered or contains duplicates: 0 20 10"),
    (([5, 10], [1, 2], [1, 2]), "First entry in pq_episode_starts_at_frame is not 0, this is probably a mistake."),
    (([3], [1], [1]), "First entry in pq_episode_starts_at_frame is not 0"),
])
def test_schedule_checks_and_messages(args, message):
    with pytest.raises(ValueError, match=message):
        flownet2_amd.LpqSchedule(*args)
    with pytest.raises(layers.CheckError, match=message):
        flownet2_amd.LpqSchedule(*args, error=layers.CheckError)


def test_schedule_at_every_boundary_and_the_c_entry_point():
    starts, ps, qs = [0, 1, 1000, 500000], [1.0, 2.0, 2.0, 0.8], [1.0, 1.0, 2.0, 0.6]
    s = flownet2_amd.LpqSchedule(starts, ps, qs)
    arr = (C.c_int * len(starts))(*starts)
    step = lambda it: _lib.lib().fn2_lpq_loss_schedule_step(len(starts), arr, it)
    want = {0: 0, 1: 1, 2: 1, 999: 1, 1000: 2, 1001: 2, 499999: 2, 500000: 3, 500001: 3, 2 ** 31 - 1: 3}
    for it, k in want.items():
        assert s.step(it) == k and step(it) == k and s.at(it) == (ps[k], qs[k]), it
    assert s.at(1000) == (2.0, 2.0) and s.at(999) == (2.0, 1.0)           # pure: going back gives the earlier episode again
    assert step(-1) == -1 and _lib.lib().fn2_lpq_loss_schedule_step(0, arr, 5) == -1 and _lib.lib().fn2_lpq_loss_schedule_step(3, None, 5) == -1


# ---- the header, the binding, sizes and refusals ----------------------------------------------------------------------------------
def test_header_declares_exactly_what_the_binding_has():
    with open(os.path.join(_lib.INCLUDE_DIR, "flownet2_hip_lpq_loss.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = re.findall(r"\b(fn2_\w+)\s*\(", body)
    want = ["fn2_lpq_loss_sizes", "fn2_lpq_loss_schedule_step", "fn2_lpq_loss_forward", "fn2_lpq_loss_backward", "fn2_lpq_loss_forward_multi",
            "fn2_lpq_loss_backward_multi"]
    assert declared == want and list(_lib.LPQ_LOSS_EXPORTS) == want
    assert not re.search(r"\b(struct|enum|double)\b|#\s*define", body)
    L = _lib.lib()
    for name in want:
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is C.c_int and getattr(L, name).argtypes == argtypes
    assert _lib.PROTOTYPES["fn2_lpq_loss_forward_multi"][1][:5] == [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    from flownet2_amd.graph_backend import GraphBackend
    assert "lpq_loss" in GraphBackend.FORWARDED and "lpq_loss_multi" in GraphBackend.FORWARDED


def test_sizes_geometry():
    one, multi1, sync = LC.sizes(1)
    assert one == multi1 == 64 + 2 * 8 * 1024 and one % 64 == 0            # {loss, normalize_coeff} padded to 64 B + 1024 pairs of fp64 partials
    assert sync >= 4 * (8 + 1) and sync % 16 == 0
    for n in range(1, 9):
        assert LC.sizes(n) == (one, n * one, sync)
    assert LC.sizes(0)[1] == 0 and LC.sizes(9)[1] == 0 and LC.sizes(-3)[1] == 0
    assert _lib.lib().fn2_lpq_loss_sizes(3, None, None, None) == 0        # any out-pointer may be NULL


def test_every_host_refusal():
    """Refusals are decided before any launch, so they need no device: the blob pointers are host buffers that nobody dereferences."""
    one, multi, sync_bytes = LC.sizes(2)
    buf = lambda n: (C.c_ubyte * n)(*([0x5A] * n))
    bufs = {k: buf(n) for k, n in (("b0", 560), ("b1", 560), ("loss", 4), ("d0", 560), ("d1", 560), ("ws", multi), ("sync", sync_bytes),
                                   ("losses", 8), ("total", 4))}
    cases = LC.refusals(bufs["b0"], bufs["b1"], bufs["loss"], bufs["d0"], bufs["d1"], bufs["ws"], one, bufs["sync"], bufs["losses"], bufs["total"])
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels) >= 40
    for label, want, call in cases:
        assert call() == want, label
        assert _lib.lib().fn2_last_error_string().decode().startswith("lpq_loss_"), label
    for k, b in bufs.items():
        assert bytes(b) == b"\x5a" * len(b), k


# ---- the references -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pq", LC.PQ_CASES, ids=lambda c: "p%g_q%g_pe%g" % c)
@pytest.mark.parametrize("name", ["2x2x5x7", "1x1x3x3", "2x3x9x8_prescale", "one_bottom"])
def test_ref32_within_bound_of_ref64(name, pq):
    shape, two, prescale, normalize, _ = LC.SHAPES[name]
    b0, b1 = LC.make_inputs(shape, two, seed=7)
    p, q, pe = pq
    B = LR.bound(b0, b1, p, q, pe, LC.Q_EPS, prescale, normalize, 0.75)
    r32, r64 = LR.ref32(b0, b1, p, q, pe, LC.Q_EPS, prescale, normalize, 0.75), B["ref"]
    assert abs(np.float64(r32["loss"]) - r64["loss"]) <= B["loss"]
    assert abs(np.float64(r32["norm"]) - r64["norm"]) <= B["norm"]
    for k in ("d0", "d1") if two else ("d0",):
        assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64
        assert np.array_equal(np.isnan(r32[k]), np.isnan(r64[k]))
        fin = ~np.isnan(r64[k])
        assert np.all(np.abs(r32[k].astype(np.float64) - r64[k])[fin] <= B[k][fin])
    assert np.isnan(r64["d0"]).any() == (pq == (0.8, 0.6, 0.0))
    assert (r64["d0"][~r64["ok"]] == 0).all() and (~r64["ok"]).sum() >= 2


@pytest.mark.parametrize("prescale, normalize", [(False, False), (True, True)])
def test_ref64_at_p2_q_half_is_the_l2_per_location_l1loss(prescale, normalize):
    """sum over pixels of sqrt(sum_c w d^2 + eps) / norm and its gradient alpha w d / sqrt(.), written out on their own in float64."""
    shape = (2, 3, 9, 8)
    b0, b1 = LC.make_inputs(shape, True, seed=11)
    r = LR.ref64(b0, b1, 2.0, 0.5, 0.0, 1e-2, prescale, normalize, 0.5)
    d = b0.astype(np.float64) - b1.astype(np.float64)
    ok = ~np.isnan(d)
    d = np.where(ok, d, 0.0)
    w = 1.0 / 3 if prescale else 1.0
    e = np.sqrt((w * d * d).sum(1) + np.float64(np.float32(1e-2)))
    norm = ok.sum() / 3 if normalize else 2.0
    assert r["norm"] == norm
    assert abs(r["loss"] - e.sum() / norm) <= 1e-13 * e.sum() / norm
    g = np.where(ok, (0.5 / norm) * w * d / e[:, None], 0.0)
    assert np.all(np.abs(r["d0"] - g) <= 1e-13 * np.abs(g)) and np.array_equal(r["d1"], -r["d0"])


# ---- opt-in registration, Net.iter and Solver.Step --------------------------------------------------------------------------------
def test_extra_layers_registers_for_one_construction_only():
    before = layers.LayerRegistry.LayerTypeList()
    assert "LpqLoss" not in before and layers.OPTIONAL_LAYER_CLASSES == {"LpqLoss": layers.LpqLossLayer}
    with pytest.raises(layers.CheckError, match="Unknown layer type: LpqLoss"):
        fnet.Net(TRAIN_NET, phase="TRAIN", device="cpu")
    assert layers.LayerRegistry.LayerTypeList() == before
    net = fnet.Net(TRAIN_NET, phase="TRAIN", device="cpu", extra_layers=("LpqLoss",))
    assert layers.LayerRegistry.LayerTypeList() == before
    loss = net.layer_by_name("loss")
    assert isinstance(loss, layers.LpqLossLayer) and loss.type() == "LpqLoss" and loss.AutoTopBlobs() and loss.GetNet() is net
    assert loss.schedule_.starts == (0, 1) and loss.schedule_.at(0) == (1.0, 1.0) and loss.schedule_.at(1) == (2.0, pytest.approx(0.2))
    assert all(l.GetNet() is net for l in net.layers)
    # a construction that fails (three bottoms) restores the registry too; so does an unknown optional name
    bad = TRAIN_NET.replace('bottom: "flow" bottom: "gt"', 'bottom: "flow" bottom: "gt" bottom: "img"')
    with pytest.raises(layers.CheckError, match="LpqLoss Layer takes at most 2 bottom"):
        fnet.Net(bad, phase="TRAIN", device="cpu", extra_layers=("LpqLoss",))
    assert layers.LayerRegistry.LayerTypeList() == before
    with pytest.raises(layers.CheckError, match="Unknown optional layer type: Accum"):
        fnet.Net(TRAIN_NET, phase="TRAIN", device="cpu", extra_layers=("Accum",))
    assert layers.LayerRegistry.LayerTypeList() == before
    # the layer's own schedule check, with the reference's message
    with pytest.raises(layers.CheckError, match="Incompatible sizes"):
        fnet.Net(TRAIN_NET.replace("p: 1 p: 2", "p: 1"), phase="TRAIN", device="cpu", extra_layers=("LpqLoss",))
    assert layers.LayerRegistry.LayerTypeList() == before


def test_solver_hands_extra_layers_on_and_step_sets_the_iteration():
    text = 'base_lr: 0.01 lr_policy: "fixed" max_iter: 10 type: "SGD" momentum: 0.9 net_param { %s }' % TRAIN_NET
    before = layers.LayerRegistry.LayerTypeList()
    with pytest.raises(layers.CheckError, match="Unknown layer type: LpqLoss"):
        fsolver.get_solver(SolverParameter(text), device="cpu")
    s = fsolver.get_solver(SolverParameter(text), device="cpu", extra_layers=("LpqLoss",))
    assert isinstance(s.net.layer_by_name("loss"), layers.LpqLossLayer) and layers.LayerRegistry.LayerTypeList() == before

    seen = []

    class Recorder(fsolver.SGDSolver):          # Step itself, without the GPU: record what the net is told, skip the update kernel
        def ApplyUpdate(self):
            pass

    net = s.net
    assert net.iter() == 0
    net.ForwardBackward = lambda **kw: seen.append(net.iter()) or 0.0
    r = Recorder(SolverParameter(text), net=net)
    r.iter_ = 5
    r.Step(3)
    assert seen == [5, 6, 7] and net.iter() == 7 and r.iter == 8
    net.set_iter(2)
    assert net.iter() == 2
