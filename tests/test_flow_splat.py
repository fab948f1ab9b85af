"""Forward warping (csrc/flow_splat.hip) on the GPU against the restatements of tests/flow_splat_ref.py: bit for bit wherever no expf is
evaluated away from 0, inside the float64 bound otherwise; against the image gradient of FlowWarp, which it generalises; sinks of the
flow (more sources on a cell than the sorted list holds); exact cases; how far one NaN reaches; what must not change a bit; the range-map
occlusion and the interpolated frame.

Largest observed share of the float64 bound (softmax, random metric in [-4, 0], the five shapes): see profiles/flow_splat.md."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import flow_splat_ref as R
from flownet2_amd import _lib, ops
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import FLOW_SPLAT_COL as COL, FLOW_SPLAT_K as K
from unsup_loss_ref import Bnd

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(1, 1, 1, 1), (1, 1, 3, 5), (2, 3, 7, 67), (3, 2, 16, 64), (1, 3, 37, 70)]
MODES = {"sum": ("none", False), "average": ("none", True), "linear": ("linear", True), "softmax": ("softmax", True)}
TIMES = (1.0, 0.5, -0.25)
COUNTS = [COL[n] for n in ("PIXELS", "MASKED", "NONFINITE", "OUTSIDE", "SPLATTED", "HOLES")]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def case(shape, seed=11):
    values, flow, metric, valid = R.random_case(shape, seed)
    rng = np.random.RandomState(seed + 1)
    g, gw = rng.uniform(-1, 1, values.shape).astype(F), rng.uniform(-1, 1, metric.shape).astype(F)
    return values, flow, metric, valid, g, gw


def metric_of(mode, metric, zero_softmax=True):
    imp = MODES[mode][0]
    if imp == "softmax" and zero_softmax:
        return np.zeros_like(metric)
    return R.metric_for(imp, metric)


@functools.lru_cache(maxsize=None)
def reference(shape, mode, t, with_valid, zero_softmax=True):
    """The float32 restatement of a random case, forward and backward, computed once."""
    values, flow, metric, valid, g, gw = case(shape)
    imp, norm = MODES[mode]
    f = R.forward32(values, flow, metric_of(mode, metric, zero_softmax), valid if with_valid else None, t=t, importance=imp, normalize=norm)
    return f, f.backward(g, gw)


def device_run(values, flow, metric, valid, g, gw, t, imp, norm, fill=ops.FILL_ZERO):
    res, out, den, hole, status = ops.flow_splat_forward(dev(values), dev(flow), dev(metric) if imp != "none" else None, dev(valid), t=t,
                                                         importance=imp, normalize=norm, fill_value=fill, hole=True, status=True)
    grads = ops.flow_splat_backward(dev(g), dev(gw), dev(values), dev(flow), dev(metric) if imp != "none" else None, dev(valid), out, den, t=t,
                                    importance=imp, normalize=norm)
    torch.cuda.synchronize()
    return host(res), host(out), host(den), host(hole), host(status), [host(x) for x in grads]


def with_fill(f, out, fill):
    if fill == ops.FILL_ZERO or not f.normalize:
        return out
    return np.where(f.hole == 1, np.array([R.FILL_NAN_BITS], np.uint32).view(F)[0], out)


def assert_not_empty(f, shape):
    if shape[2] * shape[3] >= 15:
        rows = f.rows()[-1]
        assert rows[COL["SPLATTED"]] >= 0.5 * rows[COL["PIXELS"]] and rows[COL["HOLES"]] <= rows[COL["PIXELS"]] / 3.0


# ---- bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_equals_the_float32_restatement_bit_for_bit(shape, mode):
    values, flow, metric, valid, g, gw = case(shape)
    imp, norm = MODES[mode]
    z = metric_of(mode, metric)
    for t in TIMES:
        for with_valid in (False, True):
            f, want_grads = reference(shape, mode, t, with_valid)
            if not with_valid:
                assert_not_empty(f, shape)
            for fill in (ops.FILL_ZERO, ops.FILL_NAN):
                res, out, den, hole, status, grads = device_run(values, flow, z, valid if with_valid else None, g, gw, t, imp, norm, fill)
                where = (mode, t, with_valid, fill)
                assert same(out, with_fill(f, f.out, fill)), where
                assert same(den, f.weight) and same(hole, f.hole) and same(status, f.status), where
                want = f.rows()
                assert np.array_equal(res[:, COUNTS], want[:, COUNTS]) and np.array_equal(res[:, COL["WEIGHT_MAX"]], want[:, COL["WEIGHT_MAX"]]), where
                for name, a, b in zip(("values", "flow", "metric"), grads, want_grads):
                    assert (a is None and b is None) or same(a, b), where + (name,)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_softmax_with_a_random_metric_lies_within_the_float64_bound(shape):
    values, flow, metric, valid, g, gw = case(shape)
    f32, _ = reference(shape, "softmax", 0.5, True, False)
    f64 = R.forward64(f32)
    res, out, den, hole, status, grads = device_run(values, flow, metric, valid, g, gw, 0.5, "softmax", True)
    assert same(status, f32.status) and same(hole, f32.hole) and np.array_equal(res[:, COUNTS], f32.rows()[:, COUNTS])
    share = 0.0
    for name, got, want in [("out", out, f64.out), ("weight", den, f64.weight)] + list(zip(("dvalues", "dflow", "dmetric"), grads, f64.backward(g, gw))):
        err = np.abs(got.astype(np.float64) - want.v)
        assert np.all(np.isfinite(want.e)) and np.all(err <= want.e), (name, float(np.max(err - want.e)))
        share = max(share, float(np.max(np.where(want.e > 0, err / np.where(want.e > 0, want.e, 1.0), 0.0))))
    print("flow_splat softmax %s: largest share of the float64 bound %.3f" % (ids(shape), share))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_weight_sum_is_the_exact_sum_of_the_weight_plane(shape):
    values, flow, metric, valid, g, gw = case(shape)
    res, _, den, _, _ = ops.flow_splat_forward(dev(values), dev(flow), dev(metric), None, t=0.5, importance="softmax", normalize=True)
    res, den = host(res), host(den).astype(np.float64)
    for n in range(shape[0]):
        exact, size = math.fsum(den[n].ravel()), den[n].size
        assert abs(res[n, COL["WEIGHT_SUM"]] - exact) <= size * 2.0 ** -53 * math.fsum(np.abs(den[n]).ravel())
        assert res[n, COL["WEIGHT_MAX"]] == den[n].max()
    assert abs(res[-1, COL["WEIGHT_SUM"]] - math.fsum(res[:-1, COL["WEIGHT_SUM"]])) <= shape[0] * 2.0 ** -53 * math.fsum(res[:-1, COL["WEIGHT_SUM"]])


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_sum_is_the_image_gradient_of_flow_warp(shape):
    """Independent of the restatement: the existing operation's gradient, which sorts up to 24 sources per cell."""
    values, flow, _, _, _, _ = case(shape)
    f, _ = reference(shape, "sum", 1.0, False)
    per_cell = np.zeros(shape[2] * shape[3], np.int64)
    for d in f.dec:
        cells = np.unique(np.stack([np.repeat(np.arange(d.S.size), 4), d.o.T.reshape(-1)]), axis=1)[1]
        per_cell = np.maximum(per_cell, np.bincount(cells, minlength=per_cell.size))
    assert per_cell.max() <= 24
    img = torch.zeros(shape, device="cuda", requires_grad=True)
    fl = dev(flow)
    want, = torch.autograd.grad(Fn.flow_warp(img, fl), img, dev(values))
    got = Fn.flow_splat(dev(values), fl, mode="sum")
    assert same(host(got), host(want))


# ---- sinks ---------------------------------------------------------------------------------------------------------------------------
def _sink(shape, target, seed):
    N, C_, H, W = shape
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(F)
    flow = np.stack([target[0] - xs, target[1] - ys])[None].astype(F) + rng.uniform(0.05, 0.45, (1, 2, H, W)).astype(F)
    return rng.uniform(-1, 1, shape).astype(F), flow, rng.uniform(0, 2, (N, 1, H, W)).astype(F)


@pytest.mark.parametrize("shape,target,sources", [((1, 1, 8, 8), (3.0, 4.0), 64), ((1, 2, 6, 5), (2.0, 2.0), 30)], ids=["64-on-a-cell", "30-on-a-cell"])
def test_a_sink_keeps_the_ascending_order(shape, target, sources):
    values, flow, z = _sink(shape, target, 31)
    f = R.forward32(values, flow, z, importance="linear", normalize=True)
    d = f.dec[0]
    assert d.S.size == sources and np.all(d.o[0] == int(target[1]) * shape[3] + int(target[0]))      # every source on one top-left cell
    g = np.ones(shape, F)
    want_grads = f.backward(g, None)

    def run(v, fl, zz):
        res, out, den, hole, status, grads = device_run(v, fl, zz, None, np.ones(v.shape, F), None, 1.0, "linear", True)
        return out, den, grads
    out, den, grads = run(values, flow, z)
    assert same(out, f.out) and same(den, f.weight)
    for a, b in zip(grads, want_grads):
        assert same(a, b)
    # in a batch of three with two random samples, and on a second run
    rv, rf, rz, _ = R.random_case((2,) + shape[1:], 32, lo_metric=-2.0)
    bv, bf, bz = np.concatenate([rv[:1], values, rv[1:]]), np.concatenate([rf[:1], flow, rf[1:]]), np.concatenate([-rz[:1], z, -rz[1:]])
    for _ in range(2):
        bout, bden, bgrads = run(bv, bf, bz)
        assert same(bout[1:2], out) and same(bden[1:2], den)
        for a, b in zip(bgrads, grads):
            assert same(a[1:2], b)


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------
def test_exact_cases():
    rng = np.random.RandomState(41)
    v = rng.uniform(-1, 1, (2, 3, 9, 13)).astype(F)
    zero = np.zeros((2, 2, 9, 13), F)
    res, out, den, hole, status = (host(x) for x in ops.flow_splat_forward(dev(v), dev(zero), hole=True, status=True))
    assert same(out, v) and np.all(den == 1) and not hole.any() and np.all(status == R.SPLATTED) and res[-1, COL["HOLES"]] == 0
    shift = zero.copy()
    shift[:, 0] = 2
    for t, cols in ((1.0, 2), (0.5, 1)):
        res, out, den, hole, _ = (host(x) for x in ops.flow_splat_forward(dev(v), dev(shift), t=t, hole=True))
        assert same(out[..., cols:], v[..., :-cols]) and np.all(out[..., :cols] == 0) and np.all(hole[..., :cols] == 1) and not hole[..., cols:].any()
        assert np.all(res[:2, COL["OUTSIDE"]] == 9 * cols) and np.all(res[:2, COL["HOLES"]] == 9 * cols)
    # targets on the last row and column: clamped taps that coincide
    edge = zero.copy()
    ys, xs = np.mgrid[0:9, 0:13].astype(F)
    edge[:, 0], edge[:, 1] = 12.5 - xs, 8.25 - ys
    f = R.forward32(v, edge, normalize=True)
    res, out, den, hole, status, grads = device_run(v, edge, None, None, np.ones_like(v), None, 1.0, "none", True)
    assert same(out, f.out) and same(den, f.weight) and den[0, 0, 8, 12] == 9 * 13 and res[0, COL["HOLES"]] == 9 * 13 - 1
    for a, b in zip(grads, f.backward(np.ones_like(v), None)):
        assert (a is None and b is None) or same(a, b)
    assert not grads[1].any()                                  # the clamped pairs cancel exactly


# ---- poison ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["flow", "metric", "src_valid"])
def test_one_nan_removes_exactly_that_source(what):
    shape = (2, 3, 16, 64)
    values, flow, metric, valid, g, gw = case(shape)
    valid = np.ones_like(valid)
    n, y, x = 1, 7, 33
    masked = valid.copy()
    masked[n, 0, y, x] = 0
    base = device_run(values, flow, metric, masked, g, gw, 0.5, "softmax", True)
    poisoned = {"flow": flow, "metric": metric, "src_valid": valid}
    poisoned = {k: v.copy() for k, v in poisoned.items()}
    poisoned[what][n, 0, y, x] = np.nan
    got = device_run(values, poisoned["flow"], poisoned["metric"], poisoned["src_valid"], g, gw, 0.5, "softmax", True)
    if what == "src_valid":                                    # NaN != 0: the source takes part, as with a one
        base = device_run(values, flow, metric, valid, g, gw, 0.5, "softmax", True)
    for k in (1, 2, 3):
        assert same(got[k], base[k])
    status = base[4].copy()
    if what != "src_valid":
        assert status[n, 0, y, x] == R.MASKED
        status[n, 0, y, x] = R.NONFINITE
    assert same(got[4], status)
    for a, b in zip(got[5], base[5]):
        assert same(a, b)


def test_one_nan_value_reaches_its_four_tap_cells_only():
    shape = (2, 3, 16, 64)
    values, flow, metric, valid, g, gw = case(shape)
    base = device_run(values, flow, metric, None, g, gw, 1.0, "softmax", False)
    f, _ = R.forward32(values, flow, metric, None, importance="softmax"), None
    n = 0
    k = f.dec[n].S.size // 2                                   # a SPLATTED source in the middle of the map
    y, x = divmod(int(f.dec[n].S[k]), 64)
    cells = set(int(c) for c in f.dec[n].o[:, k])
    bad = values.copy()
    bad[n, 1, y, x] = np.nan
    got = device_run(bad, flow, metric, None, g, gw, 1.0, "softmax", False)
    changed = np.nonzero(bits(got[1]) != bits(base[1]))
    assert set(zip(*changed)) <= {(n, 1, c // 64, c % 64) for c in cells} and len(changed[0]) >= 1
    assert same(got[2], base[2]) and same(got[3], base[3]) and same(got[4], base[4])
    assert same(got[5][0], base[5][0])                         # raw numerator: the gradient for values does not read values
    for i in (1, 2):
        moved = np.nonzero(bits(got[5][i]) != bits(base[5][i]))
        assert set(zip(moved[0], moved[2], moved[3])) <= {(n, y, x)}


# ---- invariance ------------------------------------------------------------------------------------------------------------------------
def _raw_forward(values, flow, metric, valid, t, imp, norm, want, offset):
    """The C entry point itself, every pointer `offset` floats (bytes for the status) past a 16-byte boundary."""
    N, C_, H, W = values.shape

    def buf(shape, dtype=torch.float32, src=None):
        n = int(np.prod(shape))
        flat = torch.empty(n + 4, dtype=dtype, device="cuda")[offset:offset + n]
        if src is not None:
            flat.copy_(torch.from_numpy(np.ascontiguousarray(src)).reshape(-1))
        return flat
    ptr = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None
    v, fl = buf(values.shape, src=values), buf(flow.shape, src=flow)
    z = buf(metric.shape, src=metric) if metric is not None else None
    m = buf(valid.shape, src=valid) if valid is not None else None
    out, den, hole = (buf(s) if w else None for s, w in zip((values.shape, (N, 1, H, W), (N, 1, H, W)), want[:3]))
    status = buf((N, 1, H, W), torch.uint8) if want[3] else None
    results = torch.empty((N + 1, K), dtype=torch.float64, device="cuda")
    ws = torch.empty(ops.flow_splat_sizes(N, C_, H, W)[0], dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().fn2_flow_splat_forward(ptr(v), ptr(fl), ptr(z), ptr(m), N, C_, H, W, C.c_float(t), R.IMPORTANCE[imp], int(norm),
                                                 ops.FILL_NAN, ptr(results), ptr(out), ptr(den), ptr(hole), ptr(status), ptr(ws), ws.numel(),
                                                 None))
    torch.cuda.synchronize()
    shapes = (values.shape, (N, 1, H, W), (N, 1, H, W), (N, 1, H, W))
    return [host(results)] + [None if b is None else host(b).reshape(s) for b, s in zip((out, den, hole, status), shapes)]


def test_what_must_not_change_a_bit():
    shape = (3, 2, 16, 64)
    values, flow, metric, valid, g, gw = case(shape)
    full = _raw_forward(values, flow, metric, None, 0.5, "softmax", True, (1, 1, 1, 1), 0)
    ones = _raw_forward(values, flow, metric, np.ones_like(valid), 0.5, "softmax", True, (1, 1, 1, 1), 0)
    moved = _raw_forward(values, flow, metric, None, 0.5, "softmax", True, (1, 1, 1, 1), 1)
    for a, b, c in zip(full, ones, moved):
        assert same(a, b) and same(a, c)
    for want in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 0, 0)):
        part = _raw_forward(values, flow, metric, None, 0.5, "softmax", True, want, 0)
        assert same(part[0], full[0])
        for a, b in zip(part[1:], full[1:]):
            assert a is None or same(a, b)
    # a sample alone has the bits it has in the batch
    alone = _raw_forward(values[1:2], flow[1:2], metric[1:2], None, 0.5, "softmax", True, (1, 1, 1, 1), 0)
    assert same(alone[0][0], full[0][1])
    for a, b in zip(alone[1:], full[1:]):
        assert same(a, b[1:2])


def test_autograd_function_and_report():
    shape = (2, 3, 7, 67)
    values, flow, metric, valid, g, gw = case(shape)
    f, want = reference(shape, "linear", 0.5, True)
    v, fl, z = (dev(a).requires_grad_() for a in (values, flow, -metric))
    out, den, hole = Fn.flow_splat(v, fl, z, t=0.5, mode="linear", src_valid=dev(valid), weight=True, hole=True)
    assert same(host(out.detach()), f.out) and same(host(den.detach()), f.weight) and same(host(hole), f.hole) and not hole.requires_grad
    (out * dev(g)).sum().add((den * dev(gw)).sum()).backward()
    for t_, b in zip((v, fl, z), want):
        assert same(host(t_.grad), b)
    rep = Fn.flow_splat_report(dev(values), dev(flow), dev(-metric), t=0.5, mode="linear", src_valid=dev(valid))
    assert np.array_equal(rep.rows[:, COUNTS], f.rows()[:-1, COUNTS]) and same(host(rep.status), f.status)
    s = rep.summary()
    assert s["pixels"] == 2 * 7 * 67 and abs(s["splatted"] + s["outside"] + s["masked"] + s["nonfinite"] - 1) < 1e-12 and s["mode"] == "linear"
    raw = Fn.flow_splat(dev(values), dev(flow), dev(-metric), t=0.5, mode="linear", normalize=False, src_valid=dev(valid))
    assert same(host(raw), np.stack([n.reshape(3, 7, 67) for n in f.num]))


# ---- range occlusion and interpolation ---------------------------------------------------------------------------------------------------
def test_range_occlusion_finds_the_disoccluded_band_and_nothing_else():
    N, H, W = 2, 12, 20
    fw = np.zeros((N, 2, H, W), F)
    fw[:, 0] = 3                                               # everything moves 3 px to the right: columns 0..2 of frame 1 are new
    bw = -fw
    occ_fw, occ_bw, range_fw, range_bw = (host(x) for x in Fn.flow_range_occlusion(dev(fw), dev(bw)))
    band_bw = np.zeros((N, 1, H, W), F)
    band_bw[..., :3] = 1                                        # nothing of frame 0 maps to the first three columns of frame 1
    band_fw = np.zeros((N, 1, H, W), F)
    band_fw[..., -3:] = 1                                       # and nothing of frame 1 maps to the last three of frame 0
    assert same(occ_bw, band_bw) and same(occ_fw, band_fw)
    assert same(range_bw, 1 - band_bw) and same(range_fw, 1 - band_fw)
    m = Fn.flow_metrics(dev(fw), dev(fw), occ=dev(occ_fw)).summary()
    assert m["epe"] == 0


def test_interpolation_of_a_translation():
    rng = np.random.RandomState(51)
    H, W = 10, 24
    wide = rng.uniform(0, 255, (1, 3, H, W + 2)).astype(F)
    img0, img1 = wide[..., 2:].copy(), wide[..., :-2].copy()   # the content moves 2 px to the right from frame 0 to frame 1
    fw = np.zeros((1, 2, H, W), F)
    fw[:, 0] = 2
    bw = -fw
    mid = host(Fn.flow_interpolate(dev(img0), dev(img1), dev(fw), dev(bw), 0.5, alpha=0.0))
    want = wide[..., 1:-1]                                      # the image moved by one pixel
    both = slice(1, W - 1)                                      # columns that both splats reach
    assert same(mid[..., both], want[..., both])
    # the default alpha: z from the device's own flow_warp and eager ops, the splats and the blend inside the float64 bound
    t = 0.25
    got = host(Fn.flow_interpolate(dev(img0), dev(img1), dev(fw), dev(bw), t))
    with torch.no_grad():
        z0 = host(-20.0 * (dev(img0) - Fn.flow_warp(dev(img1), dev(fw))).abs().mean(dim=1, keepdim=True) / 255.0)
        z1 = host(-20.0 * (dev(img1) - Fn.flow_warp(dev(img0), dev(bw))).abs().mean(dim=1, keepdim=True) / 255.0)
    a = R.forward64(R.forward32(img0, fw, z0, t=t, importance="softmax"))
    b = R.forward64(R.forward32(img1, bw, z1, t=1.0 - t, importance="softmax"))
    w0, w1 = Bnd(np.float64(F(1.0 - t))), Bnd(np.float64(F(t)))
    den = w0 * a.weight + w1 * b.weight
    num = w0 * a.out + w1 * b.out
    frame = num / den
    pos = den.v[0, 0] - den.e[0, 0] > 0
    assert pos.sum() >= (W - 4) * H
    err = np.abs(got.astype(np.float64) - frame.v)[..., pos]
    assert np.all(err <= frame.e[..., pos]), float(np.max(err - frame.e[..., pos]))
