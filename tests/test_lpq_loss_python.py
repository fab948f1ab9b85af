"""LpqLoss through the Python layers: functional.lpq_loss under torch.autograd, nets.multiscale_loss(loss=("lpq", ...)) against the
per-scale loop and loss=None against today's call, and a TRAIN prototxt whose LpqLoss layer switches episode between two Solver steps."""
import numpy as np
import pytest
import torch

import lpq_cases as LC
import lpq_ref as LR
from flownet2_amd import functional as Fn
from flownet2_amd import layers, nets, solver as fsolver
from flownet2_amd.graph_backend import backend_of
from flownet2_amd.solver import SolverParameter
from test_lpq_loss_host import TRAIN_NET

pytestmark = pytest.mark.gpu


def _check(what, got, ref, bnd):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    fin = ~np.isnan(ref)
    assert np.all(np.abs(got - ref)[fin] <= np.asarray(bnd, np.float64)[fin]), what


@pytest.mark.parametrize("two", [True, False], ids=["two_bottoms", "one_bottom"])
@pytest.mark.parametrize("pq", [(2.0, 0.2, 0.0), (0.8, 0.6, 1e-3), (1.0, 1.0, 0.0)], ids=lambda c: "p%g_q%g_pe%g" % c)
def test_functional_lpq_loss_under_autograd(pq, two):
    p, q, pe = pq
    b0, b1 = LC.make_inputs((2, 3, 9, 8), two, seed=21)
    t0 = torch.from_numpy(b0).cuda().requires_grad_(True)
    t1 = torch.from_numpy(b1).cuda().requires_grad_(True) if two else None
    loss = Fn.lpq_loss(t0, t1, p=p, q=q, p_epsilon=pe, l2_prescale_by_channels=True, normalize_by_num_entries=True)
    assert loss.shape == () and loss.requires_grad
    (loss * 0.75).backward()
    B = LR.bound(b0, b1, p, q, pe, 1e-2, True, True, 0.75)
    _check("loss", float(loss.detach()), B["ref"]["loss"], B["loss"])
    _check("bottom[0].grad", t0.grad.cpu().numpy(), B["ref"]["d0"], B["d0"])
    if two:
        _check("bottom[1].grad", t1.grad.cpu().numpy(), B["ref"]["d1"], B["d1"])
    with pytest.raises(ValueError, match="expected a CUDA"):
        Fn.lpq_loss(torch.zeros(1, 1, 2, 2), p=2.0, q=0.2)                  # no CPU path, no fall-back


def _flows_and_gt(seed=5, H=128, W=192):
    g = torch.Generator().manual_seed(seed)
    flows = {s: (torch.randn(2, 2, H >> s, W >> s, generator=g) * 0.3).cuda() for s in nets.LOSS_WEIGHTS}
    gt = (torch.randn(2, 2, H, W, generator=g) * 4).cuda()
    gt[0, :, :5, :7] = float("nan")
    return flows, gt


def test_multiscale_loss_lpq_is_the_per_scale_loop():
    flows, gt = _flows_and_gt()
    spec = ("lpq", 2.0, 0.2, 0.0, 1e-2)
    leaves = {s: f.clone().requires_grad_(True) for s, f in flows.items()}
    assert backend_of(Fn).has_multi_lpq_loss
    total = nets.multiscale_loss(leaves, gt, Fn, loss=spec)
    total.backward()
    # the loop, by hand: the same Downsample, one lpq_loss per scale, the weighted sum in list order
    loop = {s: f.clone().requires_grad_(True) for s, f in flows.items()}
    want = torch.zeros((), device="cuda")
    for s, w in nets.LOSS_WEIGHTS.items():
        tgt = Fn.downsample(gt * (1.0 / nets.FLOW_SCALE), loop[s].shape[2], loop[s].shape[3])
        want = want + torch.tensor(w, dtype=torch.float32, device="cuda") * Fn.lpq_loss(loop[s], tgt, p=2.0, q=0.2, p_epsilon=0.0, q_epsilon=1e-2,
                                                                                         normalize_by_num_entries=True)
    want.backward()
    assert torch.equal(total.detach(), want.detach())
    for s in flows:
        assert torch.equal(leaves[s].grad, loop[s].grad), s
    # a backend without the one-launch form takes the loop inside multiscale_loss: the same bits again
    class Single:
        downsample, lpq_loss = staticmethod(Fn.downsample), staticmethod(Fn.lpq_loss)
    again = nets.multiscale_loss({s: f.clone() for s, f in flows.items()}, gt, Single(), loss=spec)
    assert float(again) == float(total.detach())
    # and against ref64 at the finest scale
    s0 = 2
    tgt = Fn.downsample(gt * (1.0 / nets.FLOW_SCALE), flows[s0].shape[2], flows[s0].shape[3]).cpu().numpy()
    B = LR.bound(flows[s0].cpu().numpy(), tgt, 2.0, 0.2, 0.0, 1e-2, False, True, np.float32(nets.LOSS_WEIGHTS[s0]))
    _check("finest scale grad", leaves[s0].grad.cpu().numpy(), B["ref"]["d0"], B["d0"])
    with pytest.raises(ValueError, match="loss: None or"):
        nets.multiscale_loss(flows, gt, Fn, loss=("l1",))


def test_loss_none_is_todays_call():
    flows, gt = _flows_and_gt(seed=6)
    a = {s: f.clone().requires_grad_(True) for s, f in flows.items()}
    b = {s: f.clone().requires_grad_(True) for s, f in flows.items()}
    la, lb = nets.multiscale_loss(a, gt, Fn), nets.multiscale_loss(b, gt, Fn, None, None)
    la.backward(), lb.backward()
    assert torch.equal(la.detach(), lb.detach()) and all(torch.equal(a[s].grad, b[s].grad) for s in flows)
    want, _ = Fn.l1_loss_multi([flows[s] for s in nets.LOSS_WEIGHTS],
                               [Fn.downsample(gt * (1.0 / nets.FLOW_SCALE), flows[s].shape[2], flows[s].shape[3]) for s in nets.LOSS_WEIGHTS],
                               list(nets.LOSS_WEIGHTS.values()), l2_per_location=True, normalize_by_num_entries=True)
    assert torch.equal(la.detach(), want)
    f0 = flows[next(iter(nets.LOSS_WEIGHTS))]
    assert torch.equal(nets.final_flow_loss(f0, gt, Fn, 0.05), nets.final_flow_loss(f0, gt, Fn, 0.05, loss=None))
    lp = nets.final_flow_loss(f0, gt, Fn, 0.05, loss=("lpq", 2.0, 0.5))
    tgt = Fn.downsample(gt * 0.05, f0.shape[2], f0.shape[3]).cpu().numpy()
    B = LR.bound(f0.cpu().numpy(), tgt, 2.0, 0.5, 0.0, 1e-2, False, True)
    _check("final_flow_loss, lpq", float(lp), B["ref"]["loss"], B["loss"])


def test_train_prototxt_switches_episode_between_two_solver_steps():
    text = 'base_lr: 0.01 lr_policy: "fixed" max_iter: 10 type: "SGD" momentum: 0.9 net_param { %s }' % TRAIN_NET
    before = layers.LayerRegistry.LayerTypeList()
    torch.manual_seed(0)
    s = fsolver.get_solver(SolverParameter(text), device="cuda", extra_layers=("LpqLoss",))
    assert layers.LayerRegistry.LayerTypeList() == before
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 6, 8, generator=g)
    gt = torch.randn(2, 2, 6, 8, generator=g) * 3
    gt[1, :, 2, 3] = float("nan")
    net = s.net
    for it, (p, q) in enumerate([(1.0, 1.0), (2.0, 0.2)]):                 # lpq_loss_param of TRAIN_NET: episode 0, then episode 1 from iteration 1
        s.Step(1, lambda: {"img": img, "gt": gt})
        assert net.iter() == it and s.iter == it + 1
        layer = net.layer_by_name("loss")
        assert layer.pq_ == (p, pytest.approx(q))
        flow, tgt = net.blobs["flow"].data.cpu().numpy(), net.blobs["gt"].data.cpu().numpy()
        B = LR.bound(flow, tgt, p, q, 0.0, 1e-2, False, True, 1.0)
        _check("loss of step %d" % it, float(net.blobs["loss"].data), B["ref"]["loss"], B["loss"])
        _check("flow diff of step %d" % it, net.blobs["flow"].diff.cpu().numpy(), B["ref"]["d0"], B["d0"])
        assert layer.normalize_coeff() == float(B["ref"]["norm"])
