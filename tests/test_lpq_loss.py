"""LpqLoss kernels (csrc/lpq_loss.hip) through the C ABI of include/flownet2_hip_lpq_loss.h: every check against lpq_ref.ref64 within
lpq_ref.bound, bits against lpq_ref.ref32 where no powf runs, the 0 / 0 NaN where the header says, agreement with the L1Loss kernel at
p = 2, q = 0.5, reproducibility, the one-launch form against the single calls, and refusals that write nothing."""
import functools

import numpy as np
import pytest
import torch

import lpq_cases as LC
import lpq_ref as LR
from flownet2_amd import ops

pytestmark = pytest.mark.gpu

TOP_DIFF = 0.75
SENTINEL = 0x5A


def _dev(a, offset=0):
    """A device copy of float32 array `a` that starts `offset` floats into its (256-byte aligned) allocation."""
    if a is None:
        return None
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def _empty(shape, offset=0):
    buf = torch.empty(int(np.prod(shape)) + offset, dtype=torch.float32, device="cuda")
    return buf[offset:].view(shape)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    shape, two, _, _, _ = LC.SHAPES[name]
    b0, b1 = LC.make_inputs(shape, two, seed=sorted(LC.SHAPES).index(name))
    for a in (b0, b1):
        if a is not None:
            a.setflags(write=False)
    return b0, b1


@functools.lru_cache(maxsize=None)
def _reference(name, pq):
    """ref64 and its bound, computed once per (shape, p, q) and shared."""
    _, _, prescale, normalize, _ = LC.SHAPES[name]
    b0, b1 = _inputs(name)
    p, q, pe = pq
    return LR.bound(b0, b1, p, q, pe, LC.Q_EPS, prescale, normalize, TOP_DIFF)


def _run(name, pq):
    """One forward + backward in fresh allocations -> host results."""
    shape, two, prescale, normalize, off = LC.SHAPES[name]
    b0, b1 = _inputs(name)
    p, q, pe = pq
    one, _, _ = LC.sizes()
    t0, t1 = _dev(b0, off), _dev(b1, off)
    ws = torch.zeros(one, dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    d0, d1 = _empty(shape, off), (_empty(shape, off) if two else None)
    assert LC.forward(t0, t1, loss, shape, p, q, pe, LC.Q_EPS, prescale, normalize, ws, one) == LC.OK
    assert LC.backward(t0, t1, TOP_DIFF, d0, d1, shape, p, q, pe, LC.Q_EPS, prescale, normalize, ws, one) == LC.OK
    torch.cuda.synchronize()
    head = ws[:8].view(torch.float32).cpu().numpy()
    return {"loss": loss.cpu().numpy()[0], "ws_loss": head[0], "norm": head[1], "d0": d0.cpu().numpy(), "d1": d1.cpu().numpy() if two else None}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_close(what, got, ref, bnd):
    """Every element: NaN exactly where the reference has NaN, everything else within its bound."""
    got, ref, bnd = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bnd, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN at other elements than the reference"
    fin = ~np.isnan(ref)
    err = np.abs(got - ref)[fin]
    worst = float((err / np.maximum(bnd[fin], 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max |err| {float(err.max()) if err.size else 0.0:.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bnd[fin]), f"{what}: error up to {worst:.3f} x its bound"


@pytest.mark.parametrize("pq", LC.PQ_CASES, ids=lambda c: "p%g_q%g_pe%g" % c)
@pytest.mark.parametrize("name", list(LC.SHAPES))
def test_against_ref64(name, pq):
    shape, two, prescale, normalize, off = LC.SHAPES[name]
    b0, b1 = _inputs(name)
    p, q, pe = pq
    B = _reference(name, pq)
    r = B["ref"]
    got = _run(name, pq)
    assert _bits(got["loss"]) == _bits(got["ws_loss"])
    _check_close("loss", got["loss"], r["loss"], B["loss"])
    _check_close("normalize_coeff", got["norm"], r["norm"], B["norm"])
    _check_close("bottom[0] diff", got["d0"], r["d0"], B["d0"])
    if two:
        _check_close("bottom[1] diff", got["d1"], r["d1"], B["d1"])
    # the 0 / 0 NaN: unmasked elements with d == 0 when p_eps == 0 and p is none of 0, 1, 2 -- there and nowhere else
    want_nan = (r["ok"] & (r["d"] == 0)) if (pe == 0 and p not in (0.0, 1.0, 2.0)) else np.zeros(shape, bool)
    assert np.array_equal(np.isnan(got["d0"]), want_nan)
    if pq == (0.8, 0.6, 0.0):
        assert want_nan.sum() > 0
    masked = ~r["ok"]
    assert masked.sum() >= 2 and np.all(_bits(got["d0"])[masked] == 0)
    if pq in LC.NO_POWF:
        r32 = LR.ref32(b0, b1, p, q, pe, LC.Q_EPS, prescale, normalize, TOP_DIFF)
        assert _bits(got["loss"]) == _bits(r32["loss"]) and _bits(got["norm"]) == _bits(r32["norm"])
        assert np.array_equal(_bits(got["d0"]), _bits(r32["d0"]))
        if two:
            assert np.array_equal(_bits(got["d1"]), _bits(r32["d1"]))
    # a second run in other allocations: the same bits
    again = _run(name, pq)
    for k in ("loss", "norm", "d0", "d1"):
        if got[k] is not None:
            assert np.array_equal(_bits(got[k]), _bits(again[k])), k


def _l1_bound(b0, b1, q_eps, prescale, normalize, top_diff):
    """The same operation count for the l2_per_location L1Loss kernel (csrc/l1loss.hip): d d in place of powf(|d|, 2), sqrtf (1 ulp = 2 U)
    in place of powf(., 0.5), loss = float(dot) / norm, ds = ((e / base) 0.5) alpha, g = (2 d) (w ds)."""
    U, gamma = LR.U, LR.gamma
    r = LR.ref64(b0, b1, 2.0, 0.5, 0.0, q_eps, prescale, normalize, top_diff)
    C = b0.shape[1]
    e_d = U if b1 is not None else 0.0
    e_x = (1 + e_d) ** 2 * (1 + U) ** 3 - 1
    e_b = (1 + e_x) * (1 + gamma(max(C - 1, 0))) * (1 + U) - 1
    e_v = (1 - e_b) ** -0.5 * (1 + 2 * U) - 1
    e_n = gamma(2) if normalize else 0.0
    e_l = (1 + e_v) * (1 + U) ** 3 / (1 - e_n) - 1
    e_a = (1 + U) / (1 - e_n) - 1
    e_ds = (1 + e_v) * (1 + e_a) * (1 + U) ** 2 / (1 - e_b) - 1
    e_g = (1 + e_ds) * (1 + U) ** 2 * (1 + e_d) * (1 + U) - 1
    return {"loss": abs(r["loss"]) * e_l + LR.TINY, "d0": np.abs(r["d0"]) * e_g + LR.TINY}


@pytest.mark.parametrize("name", list(LC.SHAPES))
def test_p2_q_half_is_the_l1loss_kernel(name):
    """p = 2, q = 0.5, p_eps = 0 is L1Loss{l2_per_location, epsilon = q_eps}: fn2_l1loss_forward / _backward on the same blobs agree within
    the sum of the two kernels' bounds."""
    shape, two, prescale, normalize, off = LC.SHAPES[name]
    b0, b1 = _inputs(name)
    B = _reference(name, (2.0, 0.5, 0.0))
    got = _run(name, (2.0, 0.5, 0.0))
    params = ops.l1_params(True, prescale, normalize, LC.Q_EPS, 0.0)
    t0, t1 = _dev(b0), _dev(b1)
    loss, ws = ops.l1loss_forward(params, t0, t1)
    d0, d1 = ops.l1loss_backward(params, t0, t1, TOP_DIFF, ws)
    L = _l1_bound(b0, b1, LC.Q_EPS, prescale, normalize, TOP_DIFF)
    assert abs(float(loss) - float(got["loss"])) <= B["loss"] + L["loss"]
    assert float(ws[:8].view(torch.float32)[1]) == float(got["norm"])
    err = np.abs(d0.cpu().numpy().astype(np.float64) - got["d0"])
    assert np.all(err <= B["d0"] + L["d0"]), float((err / (B["d0"] + L["d0"])).max())
    if two:
        assert np.all(np.abs(d1.cpu().numpy().astype(np.float64) - got["d1"]) <= B["d0"] + L["d0"])


MULTI_SHAPES = [(2, 2, 6 << k, 8 << k) for k in range(5)]          # [2,2,6,8] doubling to [2,2,96,128]
MULTI_WEIGHTS = [0.32, 0.08, 0.02, 0.01, 0.005]


@pytest.mark.parametrize("pq", [(2.0, 0.2, 0.0), (0.8, 0.6, 1e-3)], ids=lambda c: "p%g_q%g_pe%g" % c)
def test_multi_equals_single_calls(pq):
    p, q, pe = pq
    n = len(MULTI_SHAPES)
    one, multi, sync_bytes = LC.sizes(n)
    ins = [LC.make_inputs(s, True, seed=100 + k) for k, s in enumerate(MULTI_SHAPES)]
    b0s, b1s = [_dev(a) for a, _ in ins], [_dev(b) for _, b in ins]
    total_diff = torch.tensor([1.75], device="cuda")
    ws = torch.zeros(multi, dtype=torch.uint8, device="cuda")
    sync = torch.zeros(sync_bytes, dtype=torch.uint8, device="cuda")
    losses, total = torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
    d0s, d1s = [_empty(s) for s in MULTI_SHAPES], [_empty(s) for s in MULTI_SHAPES]
    for _ in range(2):                                  # twice: the counters are left at zero
        assert LC.forward_multi(b0s, b1s, MULTI_SHAPES, MULTI_WEIGHTS, p, q, pe, LC.Q_EPS, False, True, losses, total, ws, multi, sync) == LC.OK
    assert LC.backward_multi(b0s, b1s, d0s, d1s, MULTI_SHAPES, MULTI_WEIGHTS, p, q, pe, LC.Q_EPS, False, True, total_diff, ws, multi) == LC.OK
    torch.cuda.synchronize()
    assert not sync.any()
    want_total = np.float32(0)
    for k, s in enumerate(MULTI_SHAPES):
        ws1 = torch.zeros(one, dtype=torch.uint8, device="cuda")
        loss1 = torch.zeros(1, device="cuda")
        e0, e1 = _empty(s), _empty(s)
        assert LC.forward(b0s[k], b1s[k], loss1, s, p, q, pe, LC.Q_EPS, False, True, ws1, one) == LC.OK
        top_diff = np.float32(MULTI_WEIGHTS[k]) * np.float32(1.75)
        assert LC.backward(b0s[k], b1s[k], top_diff, e0, e1, s, p, q, pe, LC.Q_EPS, False, True, ws1, one) == LC.OK
        torch.cuda.synchronize()
        assert _bits(loss1.cpu().numpy())[0] == _bits(losses.cpu().numpy())[k]
        assert torch.equal(ws1[:8], ws[k * one:k * one + 8])
        assert np.array_equal(_bits(e0.cpu().numpy()), _bits(d0s[k].cpu().numpy())), k
        assert np.array_equal(_bits(e1.cpu().numpy()), _bits(d1s[k].cpu().numpy())), k
        want_total = np.float32(want_total + np.float32(np.float32(MULTI_WEIGHTS[k]) * loss1.cpu().numpy()[0]))
    assert _bits(total.cpu().numpy())[0] == _bits(want_total)
    # and the result itself, at the largest scale, against ref64
    B = LR.bound(ins[-1][0], ins[-1][1], p, q, pe, LC.Q_EPS, False, True, float(np.float32(MULTI_WEIGHTS[-1]) * np.float32(1.75)))
    _check_close("multi loss", losses.cpu().numpy()[-1], B["ref"]["loss"], B["loss"])
    _check_close("multi bottom[0] diff", d0s[-1].cpu().numpy(), B["ref"]["d0"], B["d0"])


def test_refused_calls_write_nothing():
    shape = (2, 2, 5, 7)
    one, multi, sync_bytes = LC.sizes(2)
    mk = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    count = int(np.prod(shape)) * 4
    bufs = {"b0": mk(count), "b1": mk(count), "loss": mk(4), "d0": mk(count), "d1": mk(count), "ws": mk(multi), "sync": mk(sync_bytes),
            "losses": mk(8), "total": mk(4)}
    cases = LC.refusals(bufs["b0"], bufs["b1"], bufs["loss"], bufs["d0"], bufs["d1"], bufs["ws"], one, bufs["sync"], bufs["losses"], bufs["total"])
    assert len(cases) >= 40
    for label, want, call in cases:
        assert call() == want, label
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == SENTINEL).all()), k
