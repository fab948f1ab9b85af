"""The other cores of the family at training size: one FlowNetS (6 and 12 input channels), FlowNet-SD and fusion-net training step with
PRODUCTION routing against the pinned fp64 comparator (oracle/fp64_graph.train_reference), with the bounds of BASELINE config 4
(tests/test_train_parity.py): their backward passes reach what FlowNetC's never runs -- convolutions without activation (interconv*), small
output channel counts at high resolution (fusion deconv1 / deconv0 / interconv1 / interconv0, the 32- and 16-channel predict_flow heads),
Concat blobs with other channel splits, 3x3 / 2 encoders at full and half resolution, first layers with 6, 11 and 12 input channels, and
FlowNetS's 7x7 stem without the conv1 -> conv2 ReLU chain.

On the host: train_reference of every core evaluated on its own recorded ReLU branches gives the very gradients of the unpinned graph (every
activated layer is recorded exactly once), and the FN2_TRACE_CONV / relu_chain hooks."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import fp64_graph  # noqa: E402

# case: (batch, height, width) -- the training geometry each GPU test runs at (the host check of tests/test_conv_backward_routes.py too)
CASES = {"S6": (4, 320, 448), "S12": (2, 320, 448), "SD": (4, 320, 448), "fusion": (2, 320, 448)}
KIND = {"S6": "S", "S12": "S", "SD": "SD", "fusion": "fusion"}

# (case, layer): (parts of its training step no own kernel computes, why).  Exactly what
# tests/test_conv_backward_routes.py::test_family_training_graphs_have_an_own_backward_for_every_layer_but_the_allow_listed finds by
# descriptor; on the GPU these are the only library calls of the step (Fn.LIBRARY_FALLBACKS, "bwd on the library" lines).
LIBRARY_LAYERS = {
    ("SD", "conv0"): (("weight",), "6 input channels: the weight-gradient kernels need 16 channels on both sides "
                                   "(fn2_conv_backward_weights_supported); no data gradient is needed (its bottom is the input blob)"),
    ("SD", "interconv5"): (("forward",), "1026 input channels on a 10x14 map: Winograd and the direct kernel need a map width that is a "
                                         "multiple of 4, the small-map kernel a channel count that is a multiple of 8 -- the forward and with "
                                         "it both gradients are the library's (at 768x384 and 1024x448 the map is 12x24 / 14x32: Winograd)"),
    ("fusion", "conv0"): (("weight",), "11 input channels: the weight-gradient kernels need 16 channels on both sides "
                                       "(fn2_conv_backward_weights_supported); no data gradient is needed (its bottom is the input blob)"),
}


def _flow_field(rng, N, H, W, scale):
    """A smooth flow [N, 2, H, W] in pixels: coarse normal noise bilinearly up-sampled."""
    coarse = torch.from_numpy((rng.standard_normal((N, 2, max(1, H // 32), max(1, W // 32))) * scale).astype(np.float32))
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)


def _pair(rng, N, H, W):
    a = rng.integers(0, 256, (N, 3, H, W)).astype(np.float32)
    b = np.clip(np.roll(a, (3, -5), (2, 3)) + rng.normal(0, 2, a.shape), 0, 255).astype(np.float32)
    return [torch.from_numpy(im) * (1.0 / 255.0) - 0.43 for im in (a, b)]


def case_inputs(case, seed=4):
    """(parameters {name: fp32 CPU tensor}, input blob [N, C, H, W], ground truth [N, 2, H, W] in pixels with 5 % NaN) of a case, the
    input channels in the ranges the stacked FlowNet2 graph feeds them (nets.flownet2_deploy_forward): pre-processed images, the
    second image warped by a flow, flows in pixels (/ 20 into FlowNetS), their norms, brightness errors."""
    from flownet2_amd import nets
    N, H, W = CASES[case]
    rng = np.random.default_rng(seed)
    a, b = _pair(rng, N, H, W)
    cnorm = lambda t: t.pow(2).sum(1, keepdim=True).sqrt()
    warped = lambda: a + torch.from_numpy(rng.normal(0, 0.03, a.shape).astype(np.float32))
    if case == "S6":
        P, x = nets.init_params("S", seed=0, in_channels=6), torch.cat([a, b], 1)
    elif case == "S12":
        f, w = _flow_field(rng, N, H, W, 5.0), warped()
        P, x = nets.init_params("S", seed=0, in_channels=12), torch.cat([a, b, w, f / 20.0, cnorm(a - w)], 1)
    else:
        prefix = fp64_graph.PREFIX[KIND[case]]
        P = {k: v for k, v in nets.init_params_flownet2(seed=0).items() if k.startswith(prefix)}
        if case == "SD":
            x = torch.cat([a, b], 1)
        else:
            f_sd = _flow_field(rng, N, H, W, 5.0)
            f_css = f_sd + _flow_field(rng, N, H, W, 1.0)
            x = torch.cat([a, f_sd, f_css, cnorm(f_sd), cnorm(f_css), cnorm(a - warped()), cnorm(a - warped())], 1)
    gt = (_flow_field(rng, N, H, W, 5.0) + torch.from_numpy(rng.normal(0, 0.5, (N, 2, H, W)).astype(np.float32))).numpy()
    gt[np.broadcast_to(rng.random((N, 1, H, W)) < 0.05, gt.shape)] = np.nan
    return P, x.contiguous(), torch.from_numpy(gt)


def step_loss(kind, P, x, gt, backend):
    """The training step train_reference(kind, ...) evaluates, on `backend` (functional = the product's kernels)."""
    from flownet2_amd import nets
    prefix = fp64_graph.PREFIX[kind]
    Pc = nets._Prefixed(P, prefix) if prefix else P
    if kind == "S":
        return nets.multiscale_loss(nets.flownet_s_core(Pc, x, backend), gt, backend)
    core = nets.flownet_sd_core if kind == "SD" else nets.fusion_core
    return nets.final_flow_loss(core(Pc, x, backend), gt, backend, nets.FINAL_FLOW_GT_SCALE[kind])


def activated_layers(kind, in_channels=6):
    """Names of the layers with a leaky ReLU: every convolution / deconvolution but the predict_flow heads (Convolution*), the
    upsample_flow deconvolutions and SD / fusion's interconv* layers."""
    from flownet2_amd import nets
    table = nets.layer_table(kind, in_channels) if kind in ("C", "S") else (nets._SD_TABLE if kind == "SD" else nets._FUSE_TABLE)
    return [t[0] for t in table if not t[0].startswith(("Convolution", "upsample_flow", "interconv"))]


def max_rel(grads, ref):
    """Per parameter max|g - r| / max|r|: an error confined to a border row or one channel group that the relative L2 averages away."""
    return {k: float((grads[k].detach().cpu().double() - r).abs().max()) / max(float(r.abs().max()), 1e-300) for k, r in ref.items()}


# ---------------------------------------------------------------------------------------------------------------------------------------
# host


@pytest.mark.parametrize("kind,cin", [("C", 3), ("S", 6), ("S", 12), ("SD", 6), ("fusion", 11)])
def test_train_reference_on_its_own_branches_is_the_unpinned_graph(kind, cin):
    """Batch 1 @128x128 in fp64 on the CPU: train_reference evaluated on the ReLU branches recorded from its own run computes the same loss and
    the same gradient bits (a pinned leaky ReLU is x or x * slope, as leaky_relu computes it), every activated layer of the core is recorded exactly once (none
    left over, none twice), and every parameter of the core gets a gradient -- SD / fusion through their single final-flow loss too."""
    from flownet2_amd import nets
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    rng = np.random.default_rng(7)
    N, H, W = 1, 128, 128          # (the coarsest loss level of C / S: 2x2 -- the oracle's Downsample refuses 1x1)
    if kind == "C":
        P = nets.init_params("C", seed=1)
        inputs = tuple(torch.from_numpy(rng.integers(0, 256, (N, 3, H, W)).astype(np.float32)) for _ in range(2))
    elif kind == "S":
        P = nets.init_params("S", seed=1, in_channels=cin)
        inputs = (torch.from_numpy(rng.standard_normal((N, cin, H, W)).astype(np.float32) * 0.3),)
    else:
        prefix = fp64_graph.PREFIX[kind]
        P = {k: v for k, v in nets.init_params_flownet2(seed=1).items() if k.startswith(prefix)}
        inputs = (torch.from_numpy(rng.standard_normal((N, cin, H, W)).astype(np.float32) * 0.3),)
    gt = torch.from_numpy((rng.standard_normal((N, 2, H, W)) * 3).astype(np.float32))
    gt[:, :, :3, :5] = float("nan")
    with fp64_graph.record_relu_branches() as rec:
        loss, g = fp64_graph.train_reference(kind, P, inputs, gt, device="cpu")
    names = [n for n, _ in rec.branches]
    expected = activated_layers(kind, cin) + (["relu"] if kind == "C" else [])
    assert sorted(names) == sorted(expected) and len(set(names)) == len(names), names
    loss_p, g_p = fp64_graph.train_reference(kind, P, inputs, gt, device="cpu", masks=rec.branches)
    assert loss_p == loss and math.isfinite(loss)
    assert set(g) == set(g_p) == set(P)
    for k in g:
        assert torch.equal(g[k], g_p[k]), k
        assert float(g[k].abs().max()) > 0, k
    # a mask of the wrong layer is refused, not silently used
    swapped = [(names[1] if n == names[0] else names[0] if n == names[1] else n, m) for n, m in rec.branches]
    with pytest.raises(AssertionError):
        fp64_graph.train_reference(kind, P, inputs, gt, device="cpu", masks=swapped)


def test_trace_conv_keeps_the_relu_chain():
    """FN2_TRACE_CONV=1 (the nets._trace_route listener) must not drop relu_chain: a chain producer handed to a backend without the stem kernel is refused
    as without tracing (it used to be dropped silently -- the consumer then folded the ReLU derivative the producer applied again)."""
    from flownet2_amd import nets
    x, P = torch.randn(1, 3, 16, 16), {"conv1.w": torch.randn(8, 3, 7, 7) * 0.1, "conv1.b": torch.zeros(8)}
    for trace in (False, True):
        with nets.listening(nets._trace_route) if trace else contextlib.nullcontext():
            with pytest.raises(RuntimeError, match="relu_chain"):
                nets.conv_forward(x, P["conv1.w"], P["conv1.b"], 2, 3, True, None, relu_chain=(1, {"masked": False, "slope": nets.NEG_SLOPE}))
            y = nets.conv_forward(x, P["conv1.w"], P["conv1.b"], 2, 3, True, None)
        ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x, P["conv1.w"], P["conv1.b"], stride=2, padding=3), nets.NEG_SLOPE)
        assert torch.equal(y, ref)


def test_relu_chain_consumer_without_a_producer_is_refused():
    """The consumer end of a relu_chain pair (bit 1) refuses to run when no producer (bit 0) registered in the same cell during this forward:
    it would fold a ReLU derivative that the layer in front applies again in its own backward."""
    from flownet2_amd import functional as Fn
    x, w = torch.randn(1, 4, 8, 8, requires_grad=True), torch.randn(8, 4, 3, 3, requires_grad=True)
    run = lambda xx, ww, bb: torch.nn.functional.conv2d(xx, ww, bb, stride=1, padding=1)
    cell = {"masked": False, "slope": 0.1}
    with pytest.raises(RuntimeError, match="not a chain producer"):
        Fn._OwnForwardConv.apply(x, w, None, run, 1, 1, 0.1, True, False, None, (2, cell))
    y = Fn._OwnForwardConv.apply(x, w, None, run, 1, 1, 0.1, True, False, None, (1, cell))
    assert cell.get("armed") and torch.equal(y.detach(), run(x, w, None).detach())


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU

# max-elementwise bound per parameter, max|g - r| <= MAX_REL * max|r| against the same-branch fp64 graph.  Measured (the library's fp32
# kernels on the same graph in brackets): worst S6 1.7e-6 (1.4e-6), S12 2.2e-6 (1.3e-6), SD 7.7e-6 (8.8e-6) and fusion 6.0e-6 (5.8e-6)
# on conv0's weights (the allow-listed library weight gradient; SD's bias of upsample_flow6to5, a sum over 4 x 2 x 10 x 14 values with
# cancellation: 7.6e-6 (6.7e-6), its relative L2 9.4e-6 against config 4's 1e-5 (library 6.5e-6))
MAX_REL = 2e-5

# Against the PLAIN fp64 graph (its own ReLU signs) the few units whose pre-activation is within rounding of zero dominate: each one that an
# fp32 run puts on the other side changes its whole upstream gradient, the more the coarser its layer (SD's conv6_1: 4 x 5 x 7 positions
# feed Convolution1's bias).  Every case is bounded in units: the own run may put no more units on the other side of the fp64 graph's
# than twice the library fp32 run does, plus 16 (a few units per 10^7: SD 14 own, 6 library of 85 M; the library's count changes from run
# to run).  Config 4 also bounds the values (every parameter 2e-3, all of them together twice the
# library's); a case where the library's fp32 kernels land as far as that has its bounds here, with what was measured (the library's figure
# changes from run to run: its units near zero are not always the same):
PLAIN_LIKE_THE_LIBRARY = {
    # case: (worst parameter, all parameters together, why)
    "S6": (8e-3, 8e-4, "conv1.w 3.9e-3 from the plain graph, the library's fp32 kernels 3.2e-3; all together 4.9e-4, library 3.9e-4 "
                       "(1.9e-6 and 4.3e-7 on the same branch)"),
    "SD": (8e-3, 8e-4, "Convolution1.b 3.9e-3 from the plain graph, the library's fp32 kernels 1.7e-4 .. 4.1e-3 in three runs; all "
                       "together 2.9e-4, library 2.5e-5 .. 2.0e-4 (4.5e-6 and 4.4e-7 on the same branch)"),
}


def _library_lines(text, P, prefix):
    """(layer, 'forward' | 'data' | 'weight') of every 'library fallback:' line of FN2_TRACE_FALLBACK, by the weight's shape."""
    by_shape = {}
    for k, v in P.items():
        if k.endswith(".w"):
            by_shape.setdefault(tuple(v.shape), []).append(k[len(prefix):-2])
    out = []
    for line in text.splitlines():
        if not line.startswith("library fallback:"):
            continue
        shape = tuple(int(t) for t in line.rsplit("weight (", 1)[1].rstrip(")").split(",") if t.strip())
        names = by_shape.get(shape, ["?"])
        assert len(names) == 1, ("ambiguous weight shape", line, names)
        head = line.split(" bottom ")[0]
        parts = ["forward"] if "backward" not in head else [p for p in ("data", "weight") if head.endswith(p) or (" %s " % p) in head + " "]
        out += [(names[0], p) for p in parts]
    return out


def _run_case(case):
    from flownet2_amd import functional as Fn
    kind = KIND[case]
    prefix = fp64_graph.PREFIX[kind]
    dev = torch.device("cuda:0")
    P, x, gt = case_inputs(case)
    Pd = {k: v.to(dev).requires_grad_(True) for k, v in P.items()}
    xd, gtd = x.to(dev), gt.to(dev)

    def run():
        for v in Pd.values():
            v.grad = None
        loss = step_loss(kind, Pd, xd, gtd, Fn)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach())

    allowed = {name: parts for (c, name), (parts, _why) in LIBRARY_LAYERS.items() if c == case}
    expected = sorted((name, p) for name, parts in allowed.items() for p in parts)
    run()                                                   # first use: the kernels time their tile variants
    before = Fn.LIBRARY_FALLBACKS[0]
    os.environ["FN2_TRACE_BWD"], os.environ["FN2_TRACE_FALLBACK"] = "1", "1"
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), fp64_graph.record_relu_branches() as rec:
            loss = run()
    finally:
        os.environ.pop("FN2_TRACE_BWD", None)
        os.environ.pop("FN2_TRACE_FALLBACK", None)
    fallbacks = Fn.LIBRARY_FALLBACKS[0] - before
    text = buf.getvalue()
    bwd_lines = [l for l in text.splitlines() if l.startswith("bwd on the library")]
    grads = {k: v.grad.detach().clone() for k, v in Pd.items()}
    loss2 = run()                                           # bit-reproducible
    not_same = [k for k, v in Pd.items() if not torch.equal(v.grad, grads[k])]

    names = [n for n, _ in rec.branches]
    loss_p, g_p = fp64_graph.train_reference(kind, P, (x,), gt, device=dev, masks=rec.branches)
    with fp64_graph.record_relu_branches() as rec64:
        loss64, g64 = fp64_graph.train_reference(kind, P, (x,), gt, device=dev)
    with fp64_graph.record_relu_branches() as rec_lib:
        _, g_lib = fp64_graph.train_reference(kind, P, (x,), gt, device=dev, dtype=torch.float32)
    g_lib_p = fp64_graph.train_reference(kind, P, (x,), gt, device=dev, masks=rec_lib.branches)[1]
    pinned, plain = fp64_graph.grad_agreement(grads, g_p), fp64_graph.grad_agreement(grads, g64)
    lib_pinned, lib_plain = fp64_graph.grad_agreement(g_lib, g_lib_p), fp64_graph.grad_agreement(g_lib, g64)
    mx, lib_mx = max_rel(grads, g_p), max_rel(g_lib, g_lib_p)
    flips, units = fp64_graph.relu_sign_flips(rec.branches, rec_lib.branches)
    flips64, lib_flips64 = fp64_graph.relu_sign_flips(rec.branches, rec64.branches)[0], fp64_graph.relu_sign_flips(rec_lib.branches, rec64.branches)[0]
    N, H, W = CASES[case]
    lines = ["parameter gradients, %s training step (%s), batch %d @%dx%d, %d input channels (tests/test_train_parity_family.py)" % (
                 case, kind, N, W, H, x.shape[1]),
             "parameter                         rel L2: own | same-branch  library | same-branch  own | plain  library | plain"
             "   max rel: own | same-branch  library | same-branch"]
    for k in sorted(pinned["per_param"], key=lambda q: -pinned["per_param"][q]):
        lines.append("%-32s  %.2e                 %.2e                 %.2e       %.2e            %.2e                 %.2e" %
                     (k, pinned["per_param"][k], lib_pinned["per_param"][k], plain["per_param"][k], lib_plain["per_param"][k], mx[k], lib_mx[k]))
    lines.append("all parameters together           %.2e                 %.2e                 %.2e       %.2e" %
                 (pinned["all"], lib_pinned["all"], plain["all"], lib_plain["all"]))
    lines.append("median parameter                  %.2e                 %.2e                 %.2e       %.2e" %
                 (pinned["median"], lib_pinned["median"], plain["median"], lib_plain["median"]))
    worst_mx = max(mx, key=mx.get)
    lines.append("worst max rel: own %.2e (%s; library %.2e), bound %.0e; loss: own %.9g, same-branch fp64 %.9g, plain fp64 %.9g; ReLU units on "
                 "different sides in the own and the library run: %d of %d, own and plain fp64: %d, library and plain fp64: %d; library calls of the "
                 "step: %d (allow-listed: %s)" % (mx[worst_mx], worst_mx, lib_mx[worst_mx], MAX_REL, loss, loss_p, loss64, flips, units, flips64,
                                                   lib_flips64, fallbacks, sorted(allowed)))
    report = "\n".join(lines)
    print(report)                                           # (pytest -s shows the table of a passing case; a failing one shows it anyway)

    # every activated layer recorded once, every parameter has a gradient, the step is bit-reproducible
    assert sorted(names) == sorted(activated_layers(kind, x.shape[1])) and len(set(names)) == len(names), names
    assert set(grads) == set(g_p) == set(g64) == set(P)
    assert loss2 == loss and not not_same, (loss, loss2, not_same)
    # library calls: exactly the allow-listed layers (one count per layer: forward, or its backward), nothing else
    assert fallbacks == len(allowed), (fallbacks, sorted(allowed), text[-2000:])
    assert sorted(_library_lines(text, P, prefix)) == expected, (_library_lines(text, P, prefix), expected)
    assert len(bwd_lines) == sum(1 for parts in allowed.values() if "forward" not in parts), bwd_lines
    # (1) rounding only, config 4's bounds
    assert abs(loss - loss_p) <= 1e-6 * max(1.0, abs(loss_p)), (loss, loss_p)
    bad = {k: v for k, v in pinned["per_param"].items() if v > 1e-5}
    assert not bad, bad
    assert pinned["all"] <= 3e-6 and pinned["median"] <= 3e-6, (pinned["all"], pinned["median"])
    bad = {k: (v, lib_mx[k]) for k, v in mx.items() if v > MAX_REL}
    assert not bad, bad
    # (2) the plain fp64 graph, bounded by the library's fp32 kernels on it
    assert abs(loss - loss64) <= 1e-5 * max(1.0, abs(loss64)), (loss, loss64)
    assert flips64 <= 2 * lib_flips64 + 16, (flips64, lib_flips64)
    worst_bound, all_bound, _why = PLAIN_LIKE_THE_LIBRARY.get(case, (2e-3, 2.0 * lib_plain["all"] + 1e-5, None))
    assert plain["worst"] <= worst_bound and plain["all"] <= all_bound, (plain["worst_name"], plain["worst"], lib_plain["worst"], plain["all"],
                                                                         lib_plain["all"])


@pytest.mark.gpu
def test_flownets_6ch_training_step_matches_fp64():
    _run_case("S6")


@pytest.mark.gpu
def test_flownets_12ch_training_step_matches_fp64():
    _run_case("S12")


@pytest.mark.gpu
def test_flownetsd_training_step_matches_fp64():
    _run_case("SD")


@pytest.mark.gpu
def test_fusion_training_step_matches_fp64():
    _run_case("fusion")


@pytest.mark.gpu
def test_trace_conv_training_step_has_the_bits_of_the_untraced_one():
    """FN2_TRACE_CONV=1 used to drop conv1's relu_chain: conv2 still folded conv1's ReLU derivative into its data gradient and conv1's backward
    applied it a second time (slope 0.01 instead of 0.1 on negative activations).  A FlowNetC step with the stem chain active, traced and
    untraced: the same gradient bits."""
    from flownet2_amd import functional as Fn, nets
    g = torch.Generator(device="cuda").manual_seed(13)
    a = torch.rand(2, 3, 128, 192, device="cuda", generator=g) - 0.43
    b = torch.rand(2, 3, 128, 192, device="cuda", generator=g) - 0.43
    gt = torch.randn(2, 2, 128, 192, device="cuda", generator=g) * 3
    P = {k: v.cuda().requires_grad_(True) for k, v in nets.init_params("C", seed=5).items()}
    assert nets._stem_chain(P, torch.cat([a, b], 0), nets.backend_of(Fn))[0] is not None       # the chain is what this test is about

    def grads(trace):
        for v in P.values():
            v.grad = None
        with nets.listening(nets._trace_route) if trace else contextlib.nullcontext():
            loss = nets.multiscale_loss(nets.flownet_c_core(P, a, b, Fn), gt, Fn)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: v.grad.clone() for k, v in P.items()}

    l0, g0 = grads(False)
    l1, g1 = grads(True)
    assert l0 == l1
    bad = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not bad, bad


@pytest.mark.gpu
def test_the_layer_seam_sees_the_16_activated_layers_of_flownetc_on_the_product_path():
    """nets.listening around flownet_c_core on flownet2_amd.functional at [2, 3, 128, 192] (the stem chain active in training): one no_grad
    forward (every Concat written in place, the fused correlation + ReLU) and one training forward (the in-place producers as autograd
    functions) each show the 16 activated layers of tests/test_train_parity.py exactly once, and no layer leaves the own kernels.  In the
    training graph the order is the stock graph's; without autograd the fused correlation is issued in front of conv_redir."""
    from flownet2_amd import functional as Fn, nets
    expected = ["conv1", "conv2", "conv3", "conv_redir", "relu", "conv3_1", "conv4", "conv4_1", "conv5", "conv5_1", "conv6", "conv6_1",
                "deconv5", "deconv4", "deconv3", "deconv2"]
    g = torch.Generator(device="cuda").manual_seed(13)
    a = torch.rand(2, 3, 128, 192, device="cuda", generator=g) - 0.43
    b = torch.rand(2, 3, 128, 192, device="cuda", generator=g) - 0.43
    P = {k: v.cuda().requires_grad_(True) for k, v in nets.init_params("C", seed=5).items()}
    assert nets._stem_chain(P, torch.cat([a, b], 0), nets.backend_of(Fn))[0] is not None
    before = Fn.LIBRARY_FALLBACKS[0]
    seen = {}
    for mode, grad in (("no_grad", False), ("training", True)):
        names = seen[mode] = []
        with torch.set_grad_enabled(grad), nets.listening(lambda name, y, info: info["act"] and names.append(name)):
            flows = nets.flownet_c_core(P, a, b, Fn)
        assert flows[2].requires_grad == grad
    torch.cuda.synchronize()
    assert seen["training"] == expected, seen["training"]
    assert seen["no_grad"] == expected[:3] + ["relu", "conv_redir"] + expected[5:], seen["no_grad"]
    assert Fn.LIBRARY_FALLBACKS[0] == before
