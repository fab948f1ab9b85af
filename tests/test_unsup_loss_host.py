"""The unsupervised loss, everything that needs no GPU: the two restatements of include/flownet2_hip_unsup_loss.h against each other, the
float64 gradient against torch.autograd of a float64 torch restatement with clamped taps, the header's refusals and the host-only entry
point, the binding tables, UnsupLoss.summary and the training script's argument parser."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import unsup_loss_ref as R
from flownet2_amd import _lib, evaluate, nets
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import UNSUP_LOSS_COL as COL, UNSUP_LOSS_COLUMNS as COLUMNS, UNSUP_LOSS_K as K
from flownet2_amd.graph_backend import GraphBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = [(2, 3, 5, 7), (3, 1, 7, 67), (2, 3, 16, 64), (2, 3, 36, 60), (1, 2, 1, 9), (1, 2, 9, 1)]      # those of tests/test_unsup_loss.py


def _inputs(shape, kind, seed=3):
    img0, img1 = R.make_images(shape, seed)
    fw, bw = R.make_flows(shape, seed, "large" if kind == "large" else "small")
    occ_fw, occ_bw = R.make_occ(shape, seed)
    arrays = [img0, img1, fw, bw, occ_fw, occ_bw]
    if kind == "nonfinite":
        R.poison(arrays, seed)
    return arrays


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", ["small", "large", "nonfinite"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_two_restatements_agree(shape, kind, order):
    arrays = _inputs(shape, kind)
    for p in (R.params(smooth_order=order, **R.EXACT), R.params(smooth_order=order)):
        a, b = R.ref32(*arrays, p, 0.75), R.ref64(*arrays, p, 0.75)
        assert np.array_equal(a["rows"][:, :, R.COUNT_COLUMNS], b["rows"][:, :, R.COUNT_COLUMNS])
        rows = a["rows"][:, :, R.COUNT_COLUMNS[:5]]
        assert np.array_equal(rows[..., 0], rows[..., 1:].sum(-1))                  # PIXELS = COUNTED + OCCLUDED + OUTSIDE + NONFINITE
        err, bnd = np.abs(a["rows"] - b["rows"]), b["rows_bound"]
        assert np.isfinite(bnd).all() and np.all(err <= bnd)
        assert abs(float(a["loss"]) - b["loss"]) <= b["loss_bound"]
        for d in range(2):
            assert np.isfinite(a["diff"][d]).all() and np.isfinite(b["diff_bound"][d]).all()
            assert np.all(np.abs(a["diff"][d] - b["diff"][d]) <= b["diff_bound"][d])
            # the bound is worth something: a small fraction of the largest gradient at almost every element (tiny poisoned cases may
            # have no gradient left at all)
            assert np.median(b["diff_bound"][d]) <= 1e-2 * np.abs(b["diff"][d]).max() or not b["diff"][d].any()


def test_ordered_sum_is_the_sum():
    rng = np.random.default_rng(0)
    for H, W in ((5, 7), (16, 64), (36, 60), (1, 9), (67, 131)):
        v = rng.random((2, H, W)).astype(F)
        assert R.chunks(H * W) == min(-(-H * W // 1024), 128)
        assert abs(R.ordered_sum(v, H, W) - v.astype(np.float64).sum()) <= 2 * H * W * 2.0 ** -53 * v.sum()
    ones = np.ones((1, 36, 60), F)
    assert R.ordered_sum(ones, 36, 60) == 36 * 60


def _torch_loss(arrays, p, leaves):
    """The loss of the header as a float64 torch graph of the two flows (`leaves`: float64 tensors), every decision and tap index taken
    from decide: bilinear interpolation with clamped taps, psi = (t^2 + eps^2)^gamma, exp(-edge mean_c |dI|) weights, means over the
    counted pixels and over the terms."""
    img0, img1, fw, bw, occ_fw, occ_bw = arrays
    T = lambda a: torch.from_numpy(np.where(np.isfinite(a) & (np.abs(a) <= 1e9), a, 0).astype(np.float64))
    (eps_d, gam_d), (eps_s, gam_s) = ((float(F(e)), float(F(g))) for e, g in (p["charbonnier"], p["smooth_charbonnier"]))
    edge, order, mult = float(F(p["edge_weight"])), p["smooth_order"], float(F(p["flow_mult"]))
    psi = lambda t, eps, gam: (t * t + eps * eps) ** gam

    def shift(h, axis, k):
        out = torch.zeros_like(h)
        n = h.shape[axis]
        if abs(k) < n:
            src = slice(0, n - k) if k > 0 else slice(-k, n)
            dst = slice(k, n) if k > 0 else slice(0, n + k)
            idx = lambda sl: tuple(sl if i == axis else slice(None) for i in range(h.dim()))
            out[idx(dst)] = h[idx(src)]
        return out

    total = 0.0
    for (Ia, Io, a32, occ), leaf in zip(((img0, img1, fw, occ_fw), (img1, img0, bw, occ_bw)), leaves):
        N, Cc, H, W = Ia.shape
        dec = R.decide(Ia, Io, a32, occ, p)
        ixL, ixR, iyT, iyB = (torch.from_numpy(t.astype(np.int64)) for t in dec["taps"])
        a = leaf * mult
        x2 = a[:, 0] + torch.arange(W, dtype=torch.float64)[None, None, :]
        y2 = a[:, 1] + torch.arange(H, dtype=torch.float64)[None, :, None]
        al, be = x2 - ixL, y2 - iyT
        n_idx = torch.arange(N)[:, None, None]
        e = 0.0
        for c in range(Cc):
            o = T(Io[:, c])
            tap = lambda iy, ix: o[n_idx, iy, ix]
            warped = (1 - al) * (1 - be) * tap(iyT, ixL) + al * (1 - be) * tap(iyT, ixR) + (1 - al) * be * tap(iyB, ixL) + al * be * tap(iyB, ixR)
            e = e + psi(T(Ia[:, c]) - warped, eps_d, gam_d)
        counted = torch.from_numpy(dec["cls"] == 0)
        data = torch.where(counted, e, torch.zeros_like(e)).sum() / max(int(counted.sum()), 1)
        smooth, terms = 0.0, 0
        for k, axis in enumerate((2, 1)):
            valid = torch.from_numpy(dec["terms"][k])
            s = [(shift(f, axis, 1) - 2 * f) + shift(f, axis, -1) if order == 2 else shift(f, axis, -1) - f for f in (a[:, 0], a[:, 1])]
            term = psi(s[0], eps_s, gam_s) + psi(s[1], eps_s, gam_s)
            if edge != 0:
                g = sum((shift(T(Ia[:, c]), axis, -1) - (shift(T(Ia[:, c]), axis, 1) if order == 2 else T(Ia[:, c]))).abs() for c in range(Cc))
                term = torch.exp(-edge * g / Cc) * term
            smooth = smooth + torch.where(valid, term, torch.zeros_like(term)).sum()
            terms += int(valid.sum())
        total = total + float(F(p["data_weight"])) * data + float(F(p["smooth_weight"])) * smooth / max(terms, 1)
    return total


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", ["small", "large", "nonfinite"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (3, 1, 7, 67), (2, 3, 16, 64), (1, 2, 1, 9), (1, 2, 9, 1)], ids=lambda s: "x".join(map(str, s)))
def test_float64_gradient_equals_autograd(shape, kind, order):
    arrays = _inputs(shape, kind, seed=4)
    p = R.params(smooth_order=order, flow_mult=1.25, data_weight=0.75)
    want = R.ref64(*arrays, p, 1.0)
    clean = lambda a: np.where(np.isfinite(a) & (np.abs(a) <= 1e9), a, 0).astype(np.float64)
    leaves = [torch.from_numpy(clean(arrays[2])).requires_grad_(True), torch.from_numpy(clean(arrays[3])).requires_grad_(True)]
    loss = _torch_loss(arrays, p, leaves)
    loss.backward()
    assert abs(float(loss.detach()) - want["loss"]) <= 1e-12 * abs(want["loss"])
    for d in range(2):
        got, ref = leaves[d].grad.numpy(), want["diff"][d]
        scale = np.abs(ref).max()
        assert scale > 0 and np.abs(got - ref).max() <= 1e-11 * scale, f"direction {d}: {np.abs(got - ref).max():.3e} of {scale:.3e}"


def test_restatement_by_hand_on_one_row():
    """[1,1,1,4], zero flow but a = +1 at x = 1, order 1, gamma 0.5, eps 0: the data term is |I0 - I1 sampled|, the smoothness terms are
    |du| between neighbours.  I0 = (0, 1, 2, 3), I1 = (0, 2, 4, 6): d = (0, 1 - 4, 2 - 4, 3 - 6); the flows differ by 1 across two terms."""
    img0 = np.array([0, 1, 2, 3], F).reshape(1, 1, 1, 4)
    img1 = np.array([0, 2, 4, 6], F).reshape(1, 1, 1, 4)
    fw = np.zeros((1, 2, 1, 4), F)
    fw[0, 0, 0, 1] = 1
    p = R.params(charbonnier=(0.0, 0.5), smooth_charbonnier=(0.0, 0.5), edge_weight=0.0, smooth_order=1)
    r = R.ref32(img0, img1, fw, p=p)
    row = r["rows"][0, 0]
    assert row[COL["COUNTED"]] == 4 and row[COL["DATA_SUM"]] == 0 + 3 + 2 + 3 and row[COL["SMOOTH_TERMS"]] == 3 and row[COL["SMOOTH_SUM"]] == 2
    assert r["loss"] == F(8 / 4 + 2 / 3) and not r["rows"][1].any()
    # d loss / d u at x = 1: data -(d / |d|) dI1/dx / 4 = -(-1)(2) / 4; smoothness (sign(+1) - sign(-1)) / 3
    assert abs(r["diff"][0][0, 0, 0, 1] - (0.5 + 2 / 3)) <= 4 * R.U
    occluded = R.ref32(img0, img1, fw, occ_fw=np.array([0, np.nan, 1, 0], F).reshape(1, 1, 1, 4), p=p)["rows"][0, 0]
    assert occluded[COL["OCCLUDED"]] == 2 and occluded[COL["COUNTED"]] == 2 and occluded[COL["DATA_SUM"]] == 3 and occluded[COL["SMOOTH_TERMS"]] == 3


# ---- the header, the binding, sizes and refusals ----------------------------------------------------------------------------------
def test_header_declares_exactly_what_the_library_exports_in_tables_of_their_own():
    with open(os.path.join(_lib.INCLUDE_DIR, "flownet2_hip_unsup_loss.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    want = ["fn2_unsup_loss_sizes", "fn2_unsup_loss_forward", "fn2_unsup_loss_backward"]
    assert re.findall(r"\b(fn2_\w+)\s*\(", body) == want and list(_lib.UNSUP_LOSS_EXPORTS) == want
    assert list(_lib.UNSUP_LOSS_PROTOTYPES) == want and "typedef struct" not in body
    assert all(hasattr(_lib.lib(), name) for name in want)
    # the names are in their own tables and in none of the pinned ones
    assert not set(want) & set(_lib.PROTOTYPES) and not set(_lib.UNSUP_LOSS_CONSTANTS) & set(_lib.CONSTANTS)
    assert len(_lib.CONSTANTS) == 49 and len(_lib.PROTOTYPES) == 193
    assert not any("unsup" in c.lower() for c in _lib._STRUCTS)
    assert COLUMNS == ("PIXELS", "COUNTED", "OCCLUDED", "OUTSIDE", "NONFINITE", "DATA_SUM", "SMOOTH_TERMS", "SMOOTH_SUM") and K == 8
    assert _lib.UNSUP_LOSS_CONSTANTS == {"FN2_UNSUP_LOSS_" + n: i for i, n in enumerate(COLUMNS + ("K",))}
    proto = _lib.UNSUP_LOSS_PROTOTYPES
    assert proto["fn2_unsup_loss_forward"][0] is C.c_int and len(proto["fn2_unsup_loss_forward"][1]) == 24
    assert len(proto["fn2_unsup_loss_backward"][1]) == 24 and proto["fn2_unsup_loss_forward"][1][10:19] == [C.c_float] * 7 + [C.c_int, C.c_float]


def test_sizes_are_those_of_the_cut():
    for (H, W), chunks in (((1, 1), 1), ((5, 7), 1), ((32, 32), 1), ((32, 33), 2), ((36, 60), 3), ((320, 448), 128), ((384, 768), 128)):
        assert R.chunks(H * W) == chunks
        for N in (1, 3):
            assert R.sizes(N, H, W) == (8 * K * 2 * N * chunks, K)
    nbytes = C.c_size_t(77)
    assert _lib.lib().fn2_unsup_loss_sizes(0, 5, 7, C.byref(nbytes), None) == R.INVALID and nbytes.value == 77
    assert _lib.lib().fn2_unsup_loss_sizes(1, 1 << 15, 1 << 15, C.byref(nbytes), None) == R.INVALID and nbytes.value == 77
    assert _lib.lib().fn2_unsup_loss_sizes(1, 5, 7, None, None) == R.OK


def _refusals(bufs, ws_bytes):
    """(label, expected status, what the error string must name, thunk) for every call the header says is refused on the host."""
    S, nan = (2, 3, 5, 7), float("nan")
    out = []

    def add(label, want, names, backward=None, shape=S, ws=bufs["ws"], nbytes=ws_bytes, **kw):
        blobs = {k: bufs[k] for k in ("img0", "img1", "fw", "bw", "occ_fw", "occ_bw", "results", "loss", "fw_diff", "bw_diff")}
        p = R.params()
        for k, v in kw.items():
            if k in blobs:
                blobs[k] = v
            else:
                p[k] = v
        six = [blobs[k] for k in ("img0", "img1", "fw", "bw", "occ_fw", "occ_bw")]
        fwd = lambda: R.forward(*six, shape, p, blobs["results"], blobs["loss"], ws, nbytes)
        bwd = lambda: R.backward(*six, shape, p, blobs["results"], None, blobs["fw_diff"], blobs["bw_diff"])
        if backward is not True:
            out.append((label + " (forward)", want, names, "unsup_loss_forward:", fwd))
        if backward is not False and want != R.WORKSPACE:
            out.append((label + " (backward)", want, names, "unsup_loss_backward:", bwd))

    for k in ("img0", "img1", "fw", "results"):
        add(k + " NULL", R.INVALID, k, **{k: None})
    add("fw_diff NULL", R.INVALID, "fw_diff", backward=True, fw_diff=None)
    add("bw_diff without a bw", R.INVALID, "bw_diff", backward=True, bw=None)
    for label, shape in (("N = 0", (0, 3, 5, 7)), ("N < 0", (-2, 3, 5, 7)), ("H = 0", (2, 3, 0, 7)), ("W < 0", (2, 3, 5, -7))):
        add(label, R.INVALID, "shape", shape=shape)
    add("C = 0", R.INVALID, "channels", shape=(2, 0, 5, 7))
    add("C = 5", R.INVALID, "channels", shape=(2, 5, 5, 7))
    add("2^31 elements", R.INVALID, "2^31", shape=(1 << 10, 2, 1 << 10, 1 << 10))
    add("2^31 elements by the channels", R.INVALID, "2^31", shape=(1 << 9, 4, 1 << 10, 1 << 10))
    add("H W alone is 2^30", R.INVALID, "2^31", shape=(1, 1, 1 << 15, 1 << 15))
    add("every extent the largest int", R.INVALID, "2^31", shape=(2 ** 31 - 1, 4, 2 ** 31 - 1, 2 ** 31 - 1))
    for k in ("data_weight", "smooth_weight", "edge_weight"):
        add(k + " NaN", R.INVALID, k, **{k: nan})
        add(k + " < 0", R.INVALID, k, **{k: -0.5})
    for k, eps, gam in (("charbonnier", "eps_d", "gamma_d"), ("smooth_charbonnier", "eps_s", "gamma_s")):
        add(eps + " NaN", R.INVALID, eps, **{k: (nan, 0.45)})
        add(eps + " < 0", R.INVALID, eps, **{k: (-1e-3, 0.45)})
        add(gam + " NaN", R.INVALID, gam, **{k: (1e-3, nan)})
        add(gam + " = 0", R.INVALID, gam, **{k: (1e-3, 0.0)})
        add(gam + " < 0", R.INVALID, gam, **{k: (1e-3, -0.45)})
    add("smooth_order 0", R.INVALID, "smooth_order", smooth_order=0)
    add("smooth_order 3", R.INVALID, "smooth_order", smooth_order=3)
    add("flow_mult NaN", R.INVALID, "flow_mult", flow_mult=nan)
    add("workspace NULL", R.WORKSPACE, "workspace", ws=None)
    add("workspace too small", R.WORKSPACE, "workspace", nbytes=ws_bytes - 1)
    return out


def test_every_host_refusal_writes_nothing_and_names_the_argument():
    """Refusals are decided before any launch, so they need no device: the pointers are host buffers that nobody dereferences."""
    ws_bytes, _ = R.sizes(2, 5, 7)
    buf = lambda n: (C.c_ubyte * n)(*([0x5A] * n))
    bufs = {k: buf(4 * 2 * c * 5 * 7) for k, c in (("img0", 3), ("img1", 3), ("fw", 2), ("bw", 2), ("occ_fw", 1), ("occ_bw", 1), ("fw_diff", 2), ("bw_diff", 2))}
    bufs.update(results=buf(8 * 2 * 3 * K), loss=buf(4), ws=buf(ws_bytes))
    cases = _refusals(bufs, ws_bytes)
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels) and len(labels) >= 60
    for label, want, names, prefix, thunk in cases:
        assert thunk() == want, label
        text = _lib.lib().fn2_last_error_string().decode()
        assert text.startswith(prefix) and names in text, (label, text)
    for k, b in bufs.items():
        assert bytes(b) == b"\x5a" * len(b), k


def test_python_refusals_need_no_device():
    z = torch.zeros(1, 3, 4, 5)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.unsupervised_loss(z, z, torch.zeros(1, 2, 4, 5))
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.unsupervised_loss_report(z, z, torch.zeros(1, 2, 4, 5))
    with pytest.raises(RuntimeError, match="gets no gradient"):
        Fn.unsupervised_loss(z.clone().requires_grad_(True), z, torch.zeros(1, 2, 4, 5))
    assert "unsupervised_loss" in GraphBackend.FORWARDED and "flow_consistency" in GraphBackend.FORWARDED
    assert nets.backend_of(Fn).has_unsupervised_loss

    class Bare:
        pass
    assert not GraphBackend(Bare()).has_unsupervised_loss
    with pytest.raises(RuntimeError, match="no unsupervised_loss op"):
        nets.unsupervised_loss({2: z}, {2: z}, z, z, GraphBackend(Bare()))
    with pytest.raises(ValueError, match="occ must be"):
        nets.unsupervised_loss({2: z}, {2: z}, z, z, Fn, occ="census")
    import flownet2_amd
    assert flownet2_amd.unsupervised_loss is Fn.unsupervised_loss and flownet2_amd.unsupervised_loss_report is Fn.unsupervised_loss_report
    assert flownet2_amd.UnsupLoss is evaluate.UnsupLoss
    assert {"unsupervised_loss", "unsupervised_loss_report", "UnsupLoss"} <= set(flownet2_amd.__all__)


def test_summary_by_hand():
    def row(**kw):
        out = np.zeros(K)
        for k, v in kw.items():
            out[COL[k]] = v
        return out
    fw = [row(PIXELS=100, COUNTED=50, OCCLUDED=30, OUTSIDE=15, NONFINITE=5, DATA_SUM=25.0, SMOOTH_TERMS=180, SMOOTH_SUM=9.0),
          row(PIXELS=100, COUNTED=100, DATA_SUM=50.0, SMOOTH_TERMS=180, SMOOTH_SUM=27.0)]
    u = evaluate.UnsupLoss(fw, None, loss=1.5, data_weight=2.0, smooth_weight=0.5)
    s = u.summary()
    assert len(u) == 2 and s["samples"] == 2 and s["loss"] == 1.5 and s["data_weight"] == 2.0 and s["smooth_weight"] == 0.5
    assert s["fw"] == {"data_mean": 0.5, "smooth_mean": 0.1, "counted": 0.75, "occluded": 0.15, "outside": 0.075, "nonfinite": 0.025, "pixels": 200}
    assert s["bw"]["pixels"] == 0 and np.isnan(s["bw"]["data_mean"]) and np.isnan(s["bw"]["counted"])
    with pytest.raises(ValueError, match="must be"):
        evaluate.UnsupLoss(np.zeros((2, K + 1)))
    with pytest.raises(ValueError, match="backward rows"):
        evaluate.UnsupLoss(np.zeros((2, K)), np.zeros((1, K)))


def test_the_training_script_takes_the_new_flags():
    spec = importlib.util.spec_from_file_location("train_pipeline", os.path.join(ROOT, "scripts", "train_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    a = ap.parse_args([])
    assert a.unsupervised is False and a.unsup_smooth == 1.0 and a.unsup_order == 2 and a.unsup_no_occlusion is False and a.loss == "l1"
    a = ap.parse_args(["--unsupervised", "--unsup-smooth", "0.25", "--unsup-order", "1", "--unsup-no-occlusion", "--batch", "2", "--iters", "2"])
    assert a.unsupervised and a.unsup_smooth == 0.25 and a.unsup_order == 1 and a.unsup_no_occlusion and (a.batch, a.iters) == (2, 2)
    with pytest.raises(SystemExit):
        ap.parse_args(["--unsup-order", "3"])
