"""Forward warping (splatting), everything that needs no GPU: the binding tables, the host-only entry point and the header's refusals; the
two restatements of include/flownet2_hip_flow_splat.h against each other (and fma32 against exact rationals); the float64 gradients
against torch.autograd of a float64 torch restatement (index_put_ with accumulate=True); FlowSplat.summary by hand; the Python refusals,
the backend flags, the package's names and the training script's flag."""
import ctypes as C
import importlib.util
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import flow_splat_ref as R
from flownet2_amd import _lib, evaluate, nets
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import FLOW_SPLAT_COL as COL, FLOW_SPLAT_COLUMNS as COLUMNS, FLOW_SPLAT_K as K
from flownet2_amd.graph_backend import GraphBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = [(1, 1, 1, 1), (1, 1, 3, 5), (2, 3, 7, 67), (3, 2, 16, 64), (1, 3, 37, 70)]      # those of tests/test_flow_splat.py
WANT = ["fn2_flow_splat_sizes", "fn2_flow_splat_forward", "fn2_flow_splat_backward"]
MODES = {"sum": ("none", False), "average": ("none", True), "linear": ("linear", True), "softmax": ("softmax", True)}


# ---- the header, the binding, sizes and refusals ----------------------------------------------------------------------------------
def test_header_declares_exactly_three_functions_in_tables_of_their_own():
    with open(os.path.join(_lib.INCLUDE_DIR, "flownet2_hip_flow_splat.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert re.findall(r"\b(fn2_\w+)\s*\(", body) == WANT and list(_lib.FLOW_SPLAT_EXPORTS) == WANT
    assert list(_lib.FLOW_SPLAT_PROTOTYPES) == WANT and "typedef struct" not in body
    assert all(hasattr(_lib.lib(), name) for name in WANT)
    pinned = set(_lib.PROTOTYPES) | set(_lib.EXPORTS) | set(_lib.CENSUS_LOSS_PROTOTYPES) | set(_lib.FLOW_CONSISTENCY_PROTOTYPES)
    assert not set(WANT) & pinned and not set(_lib.FLOW_SPLAT_CONSTANTS) & (set(_lib.CONSTANTS) | set(_lib.CENSUS_LOSS_CONSTANTS))
    assert len(_lib.PROTOTYPES) == 193 and len(_lib.CONSTANTS) == 49 and len(_lib.EXPORTS) == 159 and len(_lib._STRUCTS) == 11
    assert COLUMNS == ("PIXELS", "MASKED", "NONFINITE", "OUTSIDE", "SPLATTED", "HOLES", "WEIGHT_SUM", "WEIGHT_MAX") and K == 8
    want = {"FN2_FLOW_SPLAT_" + n: i for i, n in enumerate(COLUMNS + ("K",))}
    want.update({"FN2_FLOW_SPLAT_IMPORTANCE_" + n: i for i, n in enumerate(("NONE", "LINEAR", "SOFTMAX"))})
    want.update({"FN2_FLOW_SPLAT_STATUS_" + n: i for i, n in enumerate(("MASKED", "NONFINITE", "OUTSIDE", "SPLATTED"))})
    assert _lib.FLOW_SPLAT_CONSTANTS == want
    proto = _lib.FLOW_SPLAT_PROTOTYPES
    assert proto["fn2_flow_splat_forward"][0] is C.c_int and len(proto["fn2_flow_splat_forward"][1]) == 20
    assert proto["fn2_flow_splat_forward"][1][8:12] == [C.c_float, C.c_int, C.c_int, C.c_int]
    assert len(proto["fn2_flow_splat_backward"][1]) == 19 and proto["fn2_flow_splat_backward"][1][12:15] == [C.c_float, C.c_int, C.c_int]
    assert len(proto["fn2_flow_splat_sizes"][1]) == 6
    # the two fills are the existing constants of the main header
    assert _lib.CONSTANTS["FN2_FILL_ZERO"] == 1 and _lib.CONSTANTS["FN2_FILL_NAN"] == 2


def _ws_bytes(N, H, W):
    chunks = min(max((H * W + 1023) // 1024, 1), 128)
    return 8 * K * N * chunks + 2 * 4 * N * H * W + N * H * W      # partial rows, list heads and links, a status plane


def test_sizes():
    sizes = _lib.lib().fn2_flow_splat_sizes
    nbytes, k = C.c_size_t(77), C.c_int(-1)
    for (H, W) in ((1, 1), (3, 5), (37, 70), (320, 448), (384, 768)):
        for N in (1, 3):
            assert sizes(N, 3, H, W, C.byref(nbytes), C.byref(k)) == R.OK and (nbytes.value, k.value) == (_ws_bytes(N, H, W), K)
    nbytes = C.c_size_t(77)
    for shape in ((0, 3, 5, 7), (1, 0, 5, 7), (1, 3, -5, 7), (1, 3, 5, 0), (1, 1, 1 << 15, 1 << 15), (1 << 10, 2, 1 << 10, 1 << 10),
                  (1 << 9, 4, 1 << 10, 1 << 10), (1 << 10, 1, 1 << 10, 1 << 10)):
        assert sizes(*shape, C.byref(nbytes), None) == R.INVALID and nbytes.value == 77
    assert sizes(1, 3, 5, 7, None, None) == R.OK


def _refusals():
    """(label, expected status, what the error string must name, thunk) for every call the header says is refused on the host.  The
    pointers are host memory: a refusal comes before any launch and writes nothing, so nothing dereferences them."""
    S = (2, 3, 5, 7)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    L = _lib.lib()
    out = []

    def fwd(label, want, names, shape=S, nbytes=None, **kw):
        a = dict(values=p, flow=p, metric=p, src_valid=None, t=1.0, importance=R.SOFTMAX, normalize=1, fill=1, results=p, out=p, weight=p,
                 hole=None, status=None, ws=p)
        a.update(kw)
        nb = _ws_bytes(shape[0], shape[2], shape[3]) if nbytes is None else nbytes
        out.append((label + " (forward)", want, names, lambda: L.fn2_flow_splat_forward(
            a["values"], a["flow"], a["metric"], a["src_valid"], *shape, C.c_float(a["t"]), a["importance"], a["normalize"], a["fill"],
            a["results"], a["out"], a["weight"], a["hole"], a["status"], a["ws"], nb if nb > 0 else 0, None)))

    def bwd(label, want, names, shape=S, **kw):
        a = dict(out_diff=p, weight_diff=None, values=p, flow=p, metric=p, src_valid=None, out=p, weight=p, t=1.0, importance=R.SOFTMAX,
                 normalize=1, values_diff=p, flow_diff=p, metric_diff=p)
        a.update(kw)
        out.append((label + " (backward)", want, names, lambda: L.fn2_flow_splat_backward(
            a["out_diff"], a["weight_diff"], a["values"], a["flow"], a["metric"], a["src_valid"], a["out"], a["weight"], *shape,
            C.c_float(a["t"]), a["importance"], a["normalize"], a["values_diff"], a["flow_diff"], a["metric_diff"], None)))

    def both(label, want, names, **kw):
        fwd(label, want, names, **kw)
        bwd(label, want, names, **kw)

    for k in ("values", "flow"):
        both(k + " NULL", R.INVALID, k, **{k: None})
    fwd("results NULL", R.INVALID, "results", results=None)
    bwd("out_diff NULL", R.INVALID, "out_diff", out_diff=None)
    bwd("weight NULL", R.INVALID, "weight", weight=None)
    bwd("out NULL with normalize", R.INVALID, "out", out=None)
    bwd("metric_diff with NONE", R.INVALID, "metric_diff", importance=R.NONE)
    for label, shape in (("N = 0", (0, 3, 5, 7)), ("N < 0", (-2, 3, 5, 7)), ("C = 0", (2, 0, 5, 7)), ("H = 0", (2, 3, 0, 7)), ("W < 0", (2, 3, 5, -7))):
        both(label, R.INVALID, "shape", shape=shape)
    both("2^31 elements", R.INVALID, "2^31", shape=(1 << 10, 2, 1 << 10, 1 << 10))
    both("2^31 elements by the flow's two planes", R.INVALID, "2^31", shape=(1 << 10, 1, 1 << 10, 1 << 10))
    both("H W alone is 2^30", R.INVALID, "2^31", shape=(1, 1, 1 << 15, 1 << 15))
    both("every extent the largest int", R.INVALID, "2^31", shape=(2 ** 31 - 1, 4, 2 ** 31 - 1, 2 ** 31 - 1))
    for label, t in (("NaN", float("nan")), ("+Inf", float("inf")), ("-Inf", float("-inf"))):
        both("t " + label, R.INVALID, "t =", t=t)
    for v in (-1, 3, 99):
        both("importance %d" % v, R.INVALID, "importance", importance=v)
    for v in (-1, 2):
        both("normalize %d" % v, R.INVALID, "normalize", normalize=v)
    for v in (R.LINEAR, R.SOFTMAX):
        both("metric NULL with importance %d" % v, R.INVALID, "metric", metric=None, importance=v)
    for v in (0, 3, -1):
        fwd("fill %d" % v, R.INVALID, "fill", fill=v)
    fwd("workspace NULL", R.WORKSPACE, "workspace", ws=None)
    fwd("workspace one byte short", R.WORKSPACE, "workspace", nbytes=_ws_bytes(2, 5, 7) - 1)
    fwd("workspace of no bytes", R.WORKSPACE, "workspace", nbytes=-1)
    return out


def test_every_refusal_of_the_header():
    cases = _refusals()
    assert len(cases) >= 50
    for label, want, names, thunk in cases:
        got = thunk()
        text = _lib.lib().fn2_last_error_string().decode()
        assert got == want, (label, got, text)
        assert text.startswith("flow_splat_") and names in text, (label, text)


# ---- the restatements -------------------------------------------------------------------------------------------------------------
def test_fma32_is_one_rounding():
    rng = np.random.RandomState(5)
    a, b = rng.uniform(-2, 2, 400).astype(F), rng.uniform(-2, 2, 400).astype(F)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.uniform(-1e-6, 1e-6, 400))).astype(F)      # cancellation: where two roundings show
    c[:100] = rng.uniform(-2, 2, 100).astype(F)
    got = R.fma32(a, b, c)
    for i in range(400):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], F(-np.inf)), np.nextafter(got[i], F(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), i
    # the case a double rounding gets wrong: 1 + 2^-11 + 2^-24 + 2^-60 lies just above a float32 midpoint and must round up
    assert R.fma32(F(1 + 2.0 ** -12), F(1 + 2.0 ** -12), F(2.0 ** -60)) == F(1 + 2.0 ** -11 + 2.0 ** -23)


def _shares(f):
    rows = f.rows()[-1]
    return rows[COL["SPLATTED"]] / rows[COL["PIXELS"]], rows[COL["HOLES"]] / rows[COL["PIXELS"]]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_random_cases_are_not_empty_and_the_restatements_agree(shape):
    """The shares the GPU tests rely on (at least half of the sources SPLATTED, at most a third of the cells holes where H W >= 15), and
    float32 within the float64 bound for every mode, forward and backward."""
    values, flow, metric, valid = R.random_case(shape, 11)
    rng = np.random.RandomState(12)
    g, gw = rng.uniform(-1, 1, values.shape).astype(F), rng.uniform(-1, 1, metric.shape).astype(F)
    for mode, (imp, norm) in MODES.items():
        for t in (1.0, 0.5, -0.25):
            f32 = R.forward32(values, flow, R.metric_for(imp, metric), None, t=t, importance=imp, normalize=norm)
            if shape[2] * shape[3] >= 15:
                splatted, holes = _shares(f32)
                assert splatted >= 0.5 and holes <= 1.0 / 3.0, (mode, t, splatted, holes)
            f64 = R.forward64(f32)
            pairs = [(f32.out, f64.out), (f32.weight, f64.weight)] + list(zip(f32.backward(g, gw), f64.backward(g, gw)))
            for a, b in pairs:
                if a is None:
                    assert b is None
                    continue
                assert np.all(np.isfinite(b.e)) and np.all(np.abs(a.astype(np.float64) - b.v) <= b.e), (mode, t)


def _torch_restatement(values, flow, metric, f32, G, GW):
    """The gradients of sum(out G) + sum(weight GW) by torch.autograd on float64: bilinear push with index_put_(accumulate=True); the
    statuses and the tap corners are those of the float32 decision."""
    N, C_, H, W = values.shape
    v = torch.tensor(values, dtype=torch.float64, requires_grad=True)
    fl = torch.tensor(flow, dtype=torch.float64, requires_grad=True)
    z = torch.tensor(metric, dtype=torch.float64, requires_grad=True)
    total = torch.zeros((), dtype=torch.float64)
    for n in range(N):
        d = f32.dec[n]
        S = torch.tensor(d.S)
        xs, ys = torch.tensor(d.xs[d.S], dtype=torch.float64), torch.tensor(d.ys[d.S], dtype=torch.float64)
        x2 = xs + float(F(f32.t)) * fl[n, 0].reshape(-1)[S]
        y2 = ys + float(F(f32.t)) * fl[n, 1].reshape(-1)[S]
        al, be = x2 - torch.tensor(d.ixL, dtype=torch.float64), y2 - torch.tensor(d.iyT, dtype=torch.float64)
        w = [(1 - al) * (1 - be), al * (1 - be), (1 - al) * be, al * be]
        e = {R.NONE: torch.ones_like(al), R.LINEAR: z[n, 0].reshape(-1)[S], R.SOFTMAX: torch.exp(z[n, 0].reshape(-1)[S])}[f32.imp]
        num, den = torch.zeros((C_, H * W), dtype=torch.float64), torch.zeros(H * W, dtype=torch.float64)
        vs = v[n].reshape(C_, -1)[:, S]
        for k in range(4):
            o = torch.tensor(d.o[k])
            num = num.index_put((torch.arange(C_)[:, None].expand(C_, o.numel()), o[None, :].expand(C_, o.numel())), vs * (w[k] * e)[None, :],
                                accumulate=True)
            den = den.index_put((o,), w[k] * e, accumulate=True)
        pos = torch.tensor(f32.pos[n])
        out = torch.where(pos[None, :], num / torch.where(pos, den, torch.ones_like(den))[None, :], torch.zeros_like(num)) if f32.normalize else num
        total = total + (out * torch.tensor(G[n].reshape(C_, -1), dtype=torch.float64)).sum()
        total = total + (den * torch.tensor(GW[n].reshape(-1), dtype=torch.float64)).sum()
    dv, df, dz = torch.autograd.grad(total, (v, fl, z), allow_unused=True)
    return dv.numpy(), df.numpy(), None if dz is None else dz.numpy()


@pytest.mark.parametrize("shape", SHAPES[1:4], ids=lambda s: "x".join(map(str, s)))
def test_float64_gradients_equal_autograd(shape):
    values, flow, metric, valid = R.random_case(shape, 21)
    flow[..., -1] = np.abs(flow[..., -1]) * 0.01 + 0.25           # last column: sources that land on the clamped taps
    rng = np.random.RandomState(22)
    g, gw = rng.uniform(-1, 1, values.shape).astype(F), rng.uniform(-1, 1, metric.shape).astype(F)
    for mode, (imp, norm) in list(MODES.items()) + [("softmax raw", ("softmax", False))]:
        for t in (1.0, -0.25):
            z = R.metric_for(imp, metric)
            f32 = R.forward32(values, flow, z, valid, t=t, importance=imp, normalize=norm)
            got = R.forward64(f32).backward(g, gw)
            want = _torch_restatement(values, flow, z, f32, g, gw)
            for name, a, b in zip(("values", "flow", "metric"), got, want):
                if a is None:
                    assert b is None or not np.any(b), (mode, name)
                    continue
                assert np.allclose(a.v, b, rtol=1e-10, atol=1e-10), (mode, t, name, np.max(np.abs(a.v - b)))
            assert np.any(got[1].v != 0)


def test_hand_cases():
    one = np.ones((1, 1, 3, 4), F)
    zero = np.zeros((1, 2, 3, 4), F)
    f = R.forward32(one * 3, zero)
    assert np.array_equal(f.out, one * 3) and np.array_equal(f.weight, one) and not f.hole.any() and np.all(f.status == R.SPLATTED)
    fl = zero.copy()
    fl[:, 0] = 2
    f = R.forward32(np.arange(12, dtype=F).reshape(1, 1, 3, 4), fl)
    assert np.array_equal(f.out[0, 0], np.array([[0, 0, 0, 1], [0, 0, 4, 5], [0, 0, 8, 9]], F))
    rows = f.rows()[0]
    assert rows[COL["OUTSIDE"]] == 6 and rows[COL["HOLES"]] == 6 and rows[COL["SPLATTED"]] == 6 and rows[COL["WEIGHT_SUM"]] == 6
    # a source on the last column with a fractional offset: both x taps are the last column, the weights add up, the x gradient cancels
    fl = zero.copy()
    fl[0, 0, 1, 3] = 0.25
    f = R.forward32(one, fl)
    assert np.array_equal(f.weight, one)
    dv, df, dz = f.backward(np.ones_like(one))
    assert df[0, 0, 1, 3] == 0 and dz is None and np.array_equal(dv, one)
    # masked, non-finite and negative-linear sources
    valid = np.ones((1, 1, 3, 4), F)
    valid[0, 0, 0, 0] = 0
    fl = zero.copy()
    fl[0, 1, 0, 1] = np.inf
    z = np.ones((1, 1, 3, 4), F)
    z[0, 0, 0, 2] = -1
    z[0, 0, 0, 3] = np.nan
    f = R.forward32(one, fl, z, valid, importance="linear", normalize=True, fill_nan=True)
    assert list(f.status[0, 0, 0]) == [R.MASKED, R.NONFINITE, R.NONFINITE, R.NONFINITE] and np.isnan(f.out[0, 0, 0]).all()
    assert np.array_equal(f.out[0, 0, 1:], one[0, 0, 1:]) and f.rows()[0][COL["HOLES"]] == 4


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_summary_by_hand():
    def row(**kw):
        out = np.zeros(K)
        for k, v in kw.items():
            out[COL[k]] = v
        return out
    s = evaluate.FlowSplat([row(PIXELS=100, SPLATTED=70, OUTSIDE=20, MASKED=6, NONFINITE=4, HOLES=25, WEIGHT_SUM=70.0, WEIGHT_MAX=3.5),
                            row(PIXELS=100, SPLATTED=100, HOLES=5, WEIGHT_SUM=100.0, WEIGHT_MAX=2.0)], t=0.5, mode="softmax")
    assert len(s) == 2
    assert s.summary() == {"splatted": 0.85, "outside": 0.1, "masked": 0.03, "nonfinite": 0.02, "holes": 0.15, "weight_mean": 0.85,
                           "weight_max": 3.5, "pixels": 200, "samples": 2, "t": 0.5, "mode": "softmax"}
    empty = evaluate.FlowSplat().summary()
    assert empty["pixels"] == 0 and np.isnan(empty["splatted"]) and np.isnan(empty["weight_max"])
    with pytest.raises(ValueError, match="rows must be"):
        evaluate.FlowSplat(np.zeros((2, K + 1)))
    assert evaluate.FLOW_SPLAT_STATUS == {"MASKED": 0, "NONFINITE": 1, "OUTSIDE": 2, "SPLATTED": 3}


def test_python_refusals_need_no_device():
    v, fl, z = torch.zeros(1, 3, 4, 5), torch.zeros(1, 2, 4, 5), torch.zeros(1, 1, 4, 5)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.flow_splat(v, fl)
    with pytest.raises(ValueError, match="mode must be"):
        Fn.flow_splat(v, fl, mode="max")
    with pytest.raises(ValueError, match="needs a metric"):
        Fn.flow_splat(v, fl, mode="softmax")
    with pytest.raises(ValueError, match="fill must be"):
        Fn.flow_splat(v, fl, fill=1.0)
    with pytest.raises(RuntimeError, match="src_valid gets no gradient"):
        Fn.flow_splat(v, fl, src_valid=z.clone().requires_grad_())
    with pytest.raises(ValueError, match="mode must be"):
        Fn.flow_splat_report(v, fl, mode="max")
    with pytest.raises(RuntimeError, match="not differentiable"):
        Fn.flow_range_occlusion(fl.clone().requires_grad_(), fl)
    with pytest.raises(ValueError, match=r"\[N,2,H,W\]"):
        Fn.flow_range_occlusion(fl, v)
    with pytest.raises(ValueError, match="threshold"):
        Fn.flow_range_occlusion(fl, fl, threshold=float("nan"))
    with pytest.raises(ValueError, match="t = "):
        Fn.flow_interpolate(v, v, fl, fl, 1.5)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.flow_range_occlusion(fl, fl)


def test_backend_flags_names_and_the_occ_argument():
    assert "flow_splat" in GraphBackend.FORWARDED and "flow_range_occlusion" in GraphBackend.FORWARDED
    assert nets.backend_of(Fn).has_flow_splat

    class NoSplat:
        unsupervised_loss = staticmethod(lambda *a, **k: None)
        flow_consistency = staticmethod(lambda *a, **k: None)
    assert not GraphBackend(NoSplat()).has_flow_splat and GraphBackend(NoSplat()).has_unsupervised_loss
    fl = {2: torch.zeros(1, 2, 4, 4)}
    img = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no flow_range_occlusion"):
        nets.unsupervised_loss(fl, fl, img, img, NoSplat(), occ="range")
    with pytest.raises(ValueError, match="occ must be"):
        nets.unsupervised_loss(fl, fl, img, img, Fn, occ="ranges")
    import flownet2_amd
    for name in ("flow_splat", "flow_splat_report", "flow_range_occlusion", "flow_interpolate", "FlowSplat"):
        assert name in flownet2_amd.__all__ and getattr(flownet2_amd, name) is not None
    assert flownet2_amd.flow_splat is Fn.flow_splat and flownet2_amd.FlowSplat is evaluate.FlowSplat


def test_the_scripts_take_the_new_flags():
    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    ap = load("train_pipeline").build_parser()
    assert ap.parse_args([]).unsup_occ == "consistency"
    assert ap.parse_args(["--unsupervised", "--unsup-occ", "range"]).unsup_occ == "range"
    with pytest.raises(SystemExit):
        ap.parse_args(["--unsup-occ", "splat"])
    interp = load("interpolate_flownet")
    a = interp.build_parser().parse_args(["frames.txt", "out"])
    assert interp.times_of(a) == [0.5] and a.batch == 1 and a.alpha == 20.0
    a = interp.build_parser().parse_args(["frames.txt", "out", "--factor", "4"])
    assert interp.times_of(a) == [0.25, 0.5, 0.75]
    with pytest.raises(SystemExit):
        interp.times_of(interp.build_parser().parse_args(["frames.txt", "out", "--times", "1.5"]))
