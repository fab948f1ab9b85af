"""Solver.Step / ApplyUpdate / Snapshot / Restore and CaffeOptimizer on a tiny TRAIN net (flownet2_amd/solver.py).  Every update is pinned
to the fp64 restatement of tests/solver_ref.py GIVEN the (w, g, h0, h1) the solver saw when the gradients were ready, so the
convolution kernels are not what is measured and nothing drifts."""
import numpy as np
import pytest
import torch

import solver_ref as R
from flownet2_amd import functional as Fn, net as fnet, solver as fsolver
from flownet2_amd.solver import SolverParameter

NET = """
name: "tiny_train"
input: "x" input_shape { dim: 2 dim: 3 dim: 8 dim: 8 }
input: "t" input_shape { dim: 2 dim: 2 dim: 8 dim: 8 }
layer { name: "c1" type: "Convolution" bottom: "x" top: "a" param { lr_mult: 1 decay_mult: 1 } param { lr_mult: 2 decay_mult: 0 }
        convolution_param { num_output: 4 kernel_size: 3 pad: 1 weight_filler { type: "gaussian" std: 0.3 } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "r1" type: "ReLU" bottom: "a" top: "a" relu_param { negative_slope: 0.1 } }
layer { name: "c2" type: "Convolution" bottom: "a" top: "b" param { lr_mult: 0 } param { lr_mult: 0 }
        convolution_param { num_output: 2 kernel_size: 1 weight_filler { type: "gaussian" std: 0.5 } } }
layer { name: "loss" type: "L1Loss" bottom: "b" bottom: "t" top: "loss" loss_weight: 1 propagate_down: true propagate_down: false
        l1_loss_param { l2_per_location: true normalize_by_num_entries: true } }
"""
CLIP = 0.01
SOLVER = ('type: "Adam" base_lr: 0.01 lr_policy: "multistep" gamma: 0.5 stepvalue: 2 momentum: 0.9 momentum2: 0.999 weight_decay: 0.0004 '
          'iter_size: 2 clip_gradients: %r snapshot_format: HDF5 ' % CLIP)
LR_MULT, DECAY_MULT = [1.0, 2.0, 0.0, 0.0], [1.0, 0.0, 1.0, 1.0]


def _feeds(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [dict(x=torch.randn((2, 3, 8, 8), generator=g).cuda(), t=torch.randn((2, 2, 8, 8), generator=g).cuda()) for _ in range(n)]


class Feeder:
    def __init__(self, feeds, start=0):
        self.feeds, self.i = feeds, start

    def __call__(self):
        self.i += 1
        return self.feeds[self.i - 1]


def _net(weights_from=None):
    n = fnet.Net(NET, phase="TRAIN", device="cuda")
    if weights_from is not None:
        for dst, src in zip(n.learnable_, weights_from.learnable_):
            dst.data.copy_(src.data)
        for layer in n.layers:
            if hasattr(layer, "note_weights_changed"):
                layer.note_weights_changed()
    return n


class Recorder:
    """on_gradients_ready: (w, g, h0, h1) of every learnable blob, the rate, the correction and the iteration, as the update will see them."""

    def __init__(self, solver, events=None):
        self.s, self.snaps, self.events = solver, [], events if events is not None else []

    def on_start(self):
        self.events.append("start")
        self.diffs_clear = all(not b.mutable_gpu_diff().any() for b in self.s.net.learnable_)

    def on_gradients_ready(self):
        self.events.append("gradients")
        s, n = self.s, len(self.s.net.learnable_)
        cpu = lambda t: t.detach().cpu().numpy().ravel().copy()
        self.snaps.append(dict(w=[cpu(b.data) for b in s.net.learnable_], g=[cpu(b.mutable_gpu_diff()) for b in s.net.learnable_],
                               h0=[cpu(h) for h in s.history_[:n]], h1=[cpu(h) for h in s.history_[n:]],
                               rate=s.GetLearningRate(), correction=s.AdamCorrection(), iter=s.iter_, step=s.current_step_))


def _state(solver):
    cpu = lambda t: t.detach().cpu().numpy().ravel().copy()
    return [cpu(b.data) for b in solver.net.learnable_], [cpu(h) for h in solver.history_]


def _check_update(snap, after_w, after_h, p, clip):
    """One update against fp64, blob by blob, with the one-step bound of solver_ref.bound.  The clip norm spans all blobs and is taken over
    the diffs as they are (ClipGradients runs before Normalize, sgd_solver.cpp:108-113).  clip / norm is evaluated in fp64: the kernel's
    float32 scale is within 2 u of it (u from its fp32 squares, u from the rounding to float32) and accum_normalization = 1/2 is exact, so
    the three roundings the bound budgets for the scaled gradient cover it."""
    n = len(snap["w"])
    scale, triggered = 1.0, False
    if clip >= 0:
        norm = float(np.sqrt(sum(np.sum(g.astype(np.float64) ** 2) for g in snap["g"])))
        triggered = norm > float(np.float32(clip))
        scale = float(np.float32(clip)) / norm if triggered else 1.0
    worst = 0.0
    for k in range(n):
        one = np.ones(snap["w"][k].size, np.float32)
        c = R.constants("Adam", snap["rate"], snap["correction"], p.momentum, p.momentum2, p.delta, p.weight_decay, LR_MULT[k] * one, DECAY_MULT[k] * one,
                        np.float32(1.0 / p.iter_size))
        c["cs"] = np.float64(scale)
        bnd, ref = R.bound(snap["w"][k], snap["g"][k], snap["h0"][k], snap["h1"][k], c)
        for name, got in (("w", after_w[k]), ("h0", after_h[k]), ("h1", after_h[n + k])):
            err = np.abs(got.astype(np.float64) - ref[name])
            assert np.all(err <= bnd[name]), (k, name, R.worst_ratio(got, ref[name], bnd[name]))
            worst = max(worst, R.worst_ratio(got, ref[name], bnd[name]))
    return triggered, worst


@pytest.fixture(scope="module")
def uninterrupted(tmp_path_factory):
    """Four iterations of Step(1) with iter_size 2, a snapshot after iteration 2; what every check below reads."""
    prefix = str(tmp_path_factory.mktemp("snap") / "tiny")
    feeds = _feeds(8)
    net = _net()
    initial = [b.data.clone() for b in net.learnable_]
    s = fsolver.get_solver(SolverParameter(SOLVER + 'snapshot: 2 snapshot_prefix: "%s"' % prefix), net=net)
    rec = Recorder(s)
    s.add_callback(rec)
    feeder, states, clear = Feeder(feeds), [], []
    for _ in range(4):
        s.Step(1, inputs=feeder)
        states.append(_state(s))
        clear.append(rec.diffs_clear)
    return dict(solver=s, rec=rec, states=states, feeds=feeds, prefix=prefix, initial=initial, clear=clear)


@pytest.mark.gpu
def test_four_iterations_meet_the_one_step_bound(uninterrupted):
    u = uninterrupted
    s, rec = u["solver"], u["rec"]
    assert isinstance(s, fsolver.AdamSolver) and s.iter_ == 4 and s.table_builds_ == 1            # the table is built once, not per step
    assert s.net.params_lr_ == LR_MULT and s.net.params_decay_ == DECAY_MULT
    assert [x["iter"] for x in rec.snaps] == [0, 1, 2, 3] and [x["step"] for x in rec.snaps] == [0, 0, 1, 1]
    b = float(np.float32(0.01))
    assert [x["rate"] for x in rec.snaps] == [b, b, float(np.float32(b * 0.5)), float(np.float32(b * 0.5))]
    for it in range(4):
        triggered, worst = _check_update(rec.snaps[it], u["states"][it][0], u["states"][it][1], s.param, CLIP)
        print("iteration %d: clip triggered %s, worst error / bound %.3f" % (it, triggered, worst))
        assert triggered
    # callbacks in the reference's order, on_start behind ClearParamDiffs
    assert rec.events == ["start", "gradients"] * 4 and all(u["clear"])
    # the lr_mult: 0 layer never moves; the others do
    for k in (2, 3):
        assert np.array_equal(u["states"][3][0][k], u["initial"][k].cpu().numpy().ravel())
    for k in (0, 1):
        assert not np.array_equal(u["states"][3][0][k], u["initial"][k].cpu().numpy().ravel())


@pytest.mark.gpu
def test_iter_size_two_sums_two_backward_passes(uninterrupted):
    u = uninterrupted
    net = _net()
    for dst, src in zip(net.learnable_, u["initial"]):
        dst.data.copy_(src)
    for layer in net.layers:
        if hasattr(layer, "note_weights_changed"):
            layer.note_weights_changed()
    passes = []
    for feed in u["feeds"][:2]:
        net.ClearParamDiffs()
        net.ForwardBackward(**feed)
        passes.append([b.mutable_gpu_diff().cpu().numpy().ravel().copy() for b in net.learnable_])
    for k, g in enumerate(u["rec"].snaps[0]["g"]):
        d1, d2 = passes[0][k].astype(np.float64), passes[1][k].astype(np.float64)
        assert np.all(np.abs(g - (d1 + d2)) <= 1e-5 * (np.abs(d1) + np.abs(d2)) + 1e-12)
    assert np.abs(u["rec"].snaps[0]["g"][0]).max() > 0 and not np.any(u["rec"].snaps[0]["g"][2])          # lr_mult 0: no parameter gradient


@pytest.mark.gpu
def test_snapshot_and_restore_continue_bit_for_bit(uninterrupted):
    u = uninterrupted
    fresh = fsolver.get_solver(SolverParameter(SOLVER + 'snapshot_prefix: "%s_other"' % u["prefix"]), net=_net())
    fresh.Restore(u["prefix"] + "_iter_2.solverstate.h5", u["prefix"] + "_iter_2.caffemodel.h5")
    assert fresh.iter_ == 2 and fresh.current_step_ == 0          # the step to stepvalue 2 is taken by the NEXT GetLearningRate, as in the reference
    w2, h2 = _state(fresh)
    for a, b in zip(w2 + h2, u["states"][1][0] + u["states"][1][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    feeder = Feeder(u["feeds"], start=4)
    for it in (2, 3):
        fresh.Step(1, inputs=feeder)
        w, h = _state(fresh)
        for a, b in zip(w + h, u["states"][it][0] + u["states"][it][1]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert fresh.iter_ == 4 and fresh.current_step_ == 1


@pytest.mark.gpu
def test_a_callback_that_halves_the_diffs_changes_the_update(uninterrupted):
    u = uninterrupted

    class Halver:                                   # what the gradient exchange does with 1 / solver_count
        def __init__(self, s):
            self.s = s

        def on_start(self):
            pass

        def on_gradients_ready(self):
            for b in self.s.net.learnable_:
                b.mutable_gpu_diff().mul_(0.5)

    text = SOLVER.replace("clip_gradients: %r" % CLIP, "clip_gradients: -1")        # a triggered clip would undo the halving
    results = []
    for halve in (False, True):
        net = _net()
        for dst, src in zip(net.learnable_, u["initial"]):
            dst.data.copy_(src)
        s = fsolver.get_solver(SolverParameter(text), net=net)
        events = []
        if halve:
            s.add_callback(Halver(s))
        rec = Recorder(s, events)
        s.add_callback(rec)                          # behind the halver: it sees what the update sees
        s.Step(1, inputs=Feeder(u["feeds"]))
        w, h = _state(s)
        triggered, _ = _check_update(rec.snaps[0], w, h, s.param, -1.0)
        assert not triggered
        results.append((rec.snaps[0]["g"], w))
    for plain, halved in zip(results[0][0], results[1][0]):
        assert np.allclose(halved, plain * np.float32(0.5), rtol=1e-4, atol=1e-9)
    assert not np.array_equal(results[0][1][0], results[1][1][0])


@pytest.mark.gpu
def test_smoothed_loss_is_the_mean_of_the_last_three(uninterrupted):
    net = _net()
    s = fsolver.get_solver(SolverParameter(SOLVER.replace("iter_size: 2", "iter_size: 1") + "average_loss: 3"), net=net)
    losses = []

    class Losses:
        def on_start(self):
            pass

        def on_gradients_ready(self):
            losses.append(float(net.loss_))

    s.add_callback(Losses())
    s.Step(5, inputs=Feeder(uninterrupted["feeds"]))
    assert len(losses) == 5 and len(set(losses)) == 5
    assert abs(s.smoothed_loss - np.mean(losses[-3:])) <= 1e-6 * np.mean(losses[-3:])


@pytest.mark.gpu
def test_caffe_optimizer_gives_the_bits_of_the_solver_and_repacks_weights(uninterrupted):
    u = uninterrupted
    net = _net()
    for dst, src in zip(net.learnable_, u["initial"]):
        dst.data.copy_(src)
    s = fsolver.get_solver(SolverParameter(SOLVER), net=net)
    net.ClearParamDiffs()
    for feed in u["feeds"][:2]:
        net.ForwardBackward(**feed)
    params = [b.data.clone().requires_grad_(True) for b in net.learnable_]
    for p, b in zip(params, net.learnable_):
        p.grad = b.mutable_gpu_diff().clone()
    opt = fsolver.CaffeOptimizer(params, SolverParameter(SOLVER), lr_mults=net.params_lr_, decay_mults=net.params_decay_)
    assert isinstance(opt, torch.optim.Optimizer)
    opt.step()
    s.ApplyUpdate()
    assert opt.iter_ == 1 and opt.table_builds_ == 1
    torch.cuda.synchronize()
    for p, b in zip(params, net.learnable_):
        assert torch.equal(p.detach().view(torch.int32), b.data.view(torch.int32))
    for a, b in zip(opt.history_, s.history_):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(params[0].detach(), u["initial"][0])
    opt.step()                                       # the same tensors: the table is not rebuilt
    assert opt.table_builds_ == 1 and opt.iter_ == 2
    # the packed-operand cache of a convolution follows the step (the global post-step hook of flownet2_amd.functional)
    g = torch.Generator().manual_seed(5)
    w = (0.1 * torch.randn((32, 32, 3, 3), generator=g)).cuda().requires_grad_(True)
    bias = torch.zeros(32, device="cuda", requires_grad=True)
    x = torch.randn((2, 32, 16, 16), generator=g).cuda()
    assert Fn.conv_route_name(x.shape, w, 1, 1) is not None          # a route with a packed operand
    opt2 = fsolver.CaffeOptimizer([w, bias], SolverParameter('type: "SGD" base_lr: 0.5 lr_policy: "fixed" momentum: 0.9'))
    with torch.no_grad():
        before = Fn.conv_mfma_relu(x, w, bias, 1, 1).clone()
    w.grad, bias.grad = torch.ones_like(w), torch.ones_like(bias)
    opt2.step()
    with torch.no_grad():
        after = Fn.conv_mfma_relu(x, w, bias, 1, 1).clone()
        Fn.invalidate_weight_caches()
        repacked = Fn.conv_mfma_relu(x, w, bias, 1, 1).clone()
    assert torch.equal(after, repacked) and not torch.equal(after, before)
