"""Wiring checks of the FlowNet2 stack that do not depend on kernels (CPU): the units the sub-networks hand to the fusion net."""
import pytest
import torch

from flownet2_amd import nets


class _Stub:
    """Backend stand-in: identity-like ops that record what they were fed."""

    def __init__(self):
        self.nearest_inputs = []

    def resample(self, x, h, w, type=2, antialias=True):
        if type == 1:
            self.nearest_inputs.append(x)
        return torch.nn.functional.interpolate(x, size=(h, w), mode="nearest")

    def flow_warp(self, img, flow):
        return img

    def channel_norm(self, x):
        return x.pow(2).sum(1, keepdim=True).sqrt()


def test_fusion_inputs_carry_pixels(monkeypatch):
    """FlowNetCSS predicts px/20 (x FLOW_SCALE), FlowNet-SD predicts px/0.05 (x SD_FLOW_SCALE = 0.05, NOT x 20 x 0.05): with
    every sub-network returning ones, the two NEAREST Resample inputs of the fusion stage are 20 and 0.05."""
    ones = lambda n, h, w: torch.ones(n, 2, h // 4, w // 4)
    monkeypatch.setattr(nets, "flownet_c_core", lambda P, a, b, be, towers=None: {2: ones(a.shape[0], a.shape[2], a.shape[3])})
    monkeypatch.setattr(nets, "flownet_s_core", lambda P, x, be=None: {2: ones(x.shape[0], x.shape[2], x.shape[3])})
    monkeypatch.setattr(nets, "flownet_sd_core", lambda P, x, be: ones(x.shape[0], x.shape[2], x.shape[3]))
    seen = {}

    def fusion(P, x, be):
        seen["x"] = x
        return torch.zeros(x.shape[0], 2, x.shape[2], x.shape[3])

    monkeypatch.setattr(nets, "fusion_core", fusion)
    be = _Stub()
    img = torch.rand(1, 3, 64, 64) * 255
    nets.flownet2_deploy_forward({}, img, img, be)
    css, sd = be.nearest_inputs
    assert torch.allclose(css, torch.full_like(css, nets.FLOW_SCALE)) and nets.FLOW_SCALE == 20.0
    assert torch.allclose(sd, torch.full_like(sd, 0.05)) and nets.SD_FLOW_SCALE == 0.05
    x = seen["x"]                                   # [img0(3), flow_sd(2), flow_css(2), |flow_sd|, |flow_css|, err_sd, err_css]
    assert x.shape[1] == 11
    assert torch.allclose(x[:, 3:5], torch.full_like(x[:, 3:5], 0.05)) and torch.allclose(x[:, 5:7], torch.full_like(x[:, 5:7], 20.0))


def test_training_graph_helpers_have_the_gradients_of_plain_slices_and_cat():
    """nets._SplitTowers / _StackedAndFirstTower / _ConcatInPlace (round 5: the training graph's tower split and in-place Concats) against the
    torch ops they replace -- same values, same gradients (CPU, float64)."""
    import torch
    from flownet2_amd import nets
    g = torch.Generator().manual_seed(0)
    x = torch.randn(6, 3, 4, 5, generator=g, dtype=torch.float64, requires_grad=True)
    wa, wb = torch.randn(3, 3, 4, 5, generator=g, dtype=torch.float64), torch.randn(3, 3, 4, 5, generator=g, dtype=torch.float64)
    a, b = nets._SplitTowers.apply(x * 1.0)
    (a * wa).sum().add((b * wb).sum()).backward()
    got = x.grad.clone(); x.grad = None
    y = x * 1.0
    ((y[:3] * wa).sum() + (y[3:] * wb).sum()).backward()
    assert torch.equal(got, x.grad); x.grad = None
    # the stacked batch for the next layer AND its first tower for the skip connection
    full, first = nets._StackedAndFirstTower.apply(x * 1.0)
    wf = torch.randn(6, 3, 4, 5, generator=g, dtype=torch.float64)
    ((full * wf).sum() + (first * wa).sum()).backward()
    got = x.grad.clone(); x.grad = None
    y = x * 1.0
    ((y * wf).sum() + (y[:3] * wa).sum()).backward()
    assert torch.allclose(got, x.grad, rtol=0, atol=1e-15); x.grad = None
    # Concat of producers that wrote their slices of one blob
    blob = torch.zeros(2, 7, 3, 3, dtype=torch.float64)

    class Into(torch.autograd.Function):            # a producer in the style of functional._OwnForwardConv(into=...)
        @staticmethod
        def forward(ctx, t, c0):
            blob.data[:, c0:c0 + t.shape[1]] = t * 2.0        # like the kernels: a write autograd's version counter does not see
            return blob[:, c0:c0 + t.shape[1]]

        @staticmethod
        def backward(ctx, gg):
            return gg * 2.0, None
    p = torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    q = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    wc = torch.randn(2, 7, 3, 3, generator=g, dtype=torch.float64)
    out = nets._ConcatInPlace.apply(blob, Into.apply(p, 0), Into.apply(q, 3))
    assert torch.equal(out, torch.cat([p.detach() * 2, q.detach() * 2], 1))
    (out * wc).sum().backward()
    gp, gq = p.grad.clone(), q.grad.clone()
    p.grad = q.grad = None
    (torch.cat([p * 2.0, q * 2.0], 1) * wc).sum().backward()
    assert torch.equal(gp, p.grad) and torch.equal(gq, q.grad)


# ---------------------------------------------------------------------------------------------------------------------
# The backend adapter (nets.GraphBackend / backend_of) and the layer seam (nets.listening): every core at [1, C, 64, 64] on the CPU, on a
# minimal backend (the fp64 comparator's: every layer on the stock form) and on a fake one that offers the in-place forms.
# ---------------------------------------------------------------------------------------------------------------------
CORES = {"C": ("C", 3), "S6": ("S", 6), "S12": ("S", 12), "SD": ("SD", 6), "fusion": ("fusion", 11)}


def _core_case(case):
    """(parameters under bare layer names, input blob [1, C, 64, 64], names of the activated layers in table order)."""
    kind, cin = CORES[case]
    if kind in ("C", "S"):
        P, table = nets.init_params(kind, seed=2, in_channels=cin), nets.layer_table(kind, cin)
    else:
        prefix, table = ("netsd_", nets._SD_TABLE) if kind == "SD" else ("fuse_", nets._FUSE_TABLE)
        P = {k[len(prefix):]: v for k, v in nets.init_params_flownet2(seed=2).items() if k.startswith(prefix)}
    x = torch.randn(1, cin, 64, 64, generator=torch.Generator().manual_seed(3)) * 0.3
    return P, x, [t[0] for t in table if not t[0].startswith(("Convolution", "upsample_flow", "interconv"))]


def _run_core(case, P, x, be):
    """(names the listener saw on activated layers, in execution order; the core's flows as a list)."""
    kind = CORES[case][0]
    names = []
    with torch.no_grad(), nets.listening(lambda name, y, info: info["act"] and names.append(name)):
        if kind == "C":
            out = nets.flownet_c_core(P, x, torch.roll(x, (1, -2), (2, 3)), be)
        else:
            out = {"S": nets.flownet_s_core, "SD": nets.flownet_sd_core, "fusion": nets.fusion_core}[kind](P, x, be)
    return names, [out[s] for s in sorted(out)] if isinstance(out, dict) else [out]


class _InPlaceBackend:
    """A backend with the in-place forms of flownet2_amd.functional (convolution / deconvolution / upsample_flow / correlation + ReLU into a
    channel slice of a blob) on torch's CPU ops.  `decline`: layer names its own kernels answer None for; calls are counted by layer name."""

    def __init__(self, P, decline=()):
        from oracle import fp64_graph
        import collections
        self.names = {id(v): k[:-2] for k, v in P.items() if k.endswith(".w")}
        self.decline, self.calls = set(decline), collections.Counter()
        self.correlation = fp64_graph.backend64().correlation

    def _layer(self, what, fn, x, w, b, slope, act, out, out_c0, **geometry):
        name = self.names[id(w)]
        self.calls[(what, name, out is not None)] += 1
        if name in self.decline:
            return None
        y = fn(x, w, b, **geometry)
        y = torch.nn.functional.leaky_relu(y, slope) if act else y
        if out is None:
            return y
        out[:, out_c0:out_c0 + y.shape[1]] = y
        return out

    def conv_mfma_relu(self, x, w, b, stride, pad, slope=0.1, act=True, out=None, out_c0=0, relu_chain=None):
        assert relu_chain is None
        return self._layer("conv", torch.nn.functional.conv2d, x, w, b, slope, act, out, out_c0, stride=stride, padding=pad)

    def deconv_relu(self, x, w, b, slope=0.1, act=True, out=None, out_c0=0):
        return self._layer("deconv", torch.nn.functional.conv_transpose2d, x, w, b, slope, act, out, out_c0, stride=2, padding=1)

    def upsample_flow_deconv(self, x, w, b=None, out=None, out_c0=0):
        return self._layer("upsample", torch.nn.functional.conv_transpose2d, x, w, b, 0.0, False, out, out_c0, stride=2, padding=1)

    def correlation_relu_into(self, b0, b1, out, out_c0, slope, training=False, **kw):
        out[:, out_c0:] = torch.nn.functional.leaky_relu(self.correlation(b0, b1, **kw), slope)
        return out

    def lib_conv2d(self, x, w, b, stride, pad):
        self.calls[("lib_conv2d", self.names[id(w)])] += 1
        return torch.nn.functional.conv2d(x, w, b, stride=stride, padding=pad)

    def lib_conv_transpose2d(self, x, w, b, stride, pad):
        self.calls[("lib_conv_transpose2d", self.names[id(w)])] += 1
        return torch.nn.functional.conv_transpose2d(x, w, b, stride=stride, padding=pad)


_MINIMAL = {}


def _minimal_run(case):
    """The core on the minimal backend, computed once per case: (parameters, input, recorded names, flows)."""
    if case not in _MINIMAL:
        from oracle import fp64_graph
        P, x, activated = _core_case(case)
        names, flows = _run_core(case, P, x, fp64_graph.backend64())
        expected = activated[:4] + ["relu"] + activated[4:] if case == "C" else activated      # the correlation's ReLU: behind conv_redir
        assert names == expected, names
        _MINIMAL[case] = (P, x, names, flows)
    return _MINIMAL[case]


def _in_place_order(names):
    """With the fused correlation + ReLU the correlation is issued in front of conv_redir (it decides whether the [conv_redir | corr] blob is
    used at all), so "relu" comes before "conv_redir" in execution order: the one difference from the stock graph's order."""
    names = list(names)
    if "relu" in names:
        i, j = names.index("conv_redir"), names.index("relu")
        names[i], names[j] = names[j], names[i]
    return names


@pytest.mark.parametrize("case", list(CORES))
def test_the_seam_sees_every_activated_layer_exactly_once(case):
    """nets.listening over every core: on the minimal backend the recorded names are the activated layers of the core's table in execution
    order (plus "relu", the correlation's, for C); on a backend with the in-place forms -- every skip convolution, stage deconvolution and
    upsampled flow written into its Concat blob, the fused correlation + ReLU -- the same layers once each, and the same flow bits."""
    P, x, names, flows = _minimal_run(case)
    fake = _InPlaceBackend(P)
    names_ip, flows_ip = _run_core(case, P, x, fake)
    assert names_ip == _in_place_order(names), names_ip
    assert len(flows_ip) == len(flows) and all(torch.equal(a, b) for a, b in zip(flows_ip, flows))
    # the in-place forms did run: no library call, every skip convolution / stage deconvolution / upsampled flow asked for (and given) a slice
    assert not [k for k in fake.calls if k[0].startswith("lib_")], fake.calls
    into = {k[1] for k in fake.calls if k[2]}
    stages = [n for n in P if n.startswith("deconv")]
    assert len(stages) >= 2 and all(n[:-2] in into for n in stages if n.endswith(".w")), (into, stages)
    assert sum(1 for k in fake.calls if k[0] == "upsample" and k[2]) == len(stages) // 2
    assert sum(1 for k in fake.calls if k[0] == "conv" and k[2]) >= len(stages) // 2


# case: (declined skip convolution, declined stage deconvolution, a stage left without a blob, a stage that keeps its blob)
DECLINED = {"C": ("conv3_1", "deconv4", "deconv3", "deconv5"), "S6": ("conv3_1", "deconv4", "deconv3", "deconv5"),
            "S12": ("conv3_1", "deconv4", "deconv3", "deconv5"), "SD": ("conv3_1", "deconv4", "deconv3", "deconv5"),
            "fusion": ("conv1_1", "deconv0", "deconv1", None)}


@pytest.mark.parametrize("case", list(CORES))
def test_declining_is_per_layer(case):
    """The same fake declining one skip convolution (conv3_1; fusion: conv1_1 -- its stage falls back to the stock Concat) and one stage
    deconvolution (deconv4; fusion: deconv0 -- copied into the blob) only: the same names, the same bits, and exactly those two layers on
    the stock form (the library convolution)."""
    conv, deconv, no_blob, in_place = DECLINED[case]
    P, x, names, flows = _minimal_run(case)
    fake = _InPlaceBackend(P, decline=(conv, deconv))
    names_ip, flows_ip = _run_core(case, P, x, fake)
    assert names_ip == _in_place_order(names), names_ip
    assert all(torch.equal(a, b) for a, b in zip(flows_ip, flows))
    assert {k: v for k, v in fake.calls.items() if k[0].startswith("lib_")} == {("lib_conv2d", conv): 1, ("lib_conv_transpose2d", deconv): 1}
    assert fake.calls[("conv", conv, True)] == 1 and fake.calls[("conv", conv, False)] == 1                     # asked in place, then stock
    assert fake.calls[("deconv", deconv, True)] == 1 and fake.calls[("deconv", deconv, False)] == 1
    assert fake.calls[("deconv", no_blob, True)] == 0 and fake.calls[("deconv", no_blob, False)] == 1           # no blob: the stock Concat
    if in_place is not None:
        assert fake.calls[("deconv", in_place, True)] == 1 and fake.calls[("deconv", in_place, False)] == 0


def test_adapter_contract():
    from oracle import fp64_graph
    be = nets.backend_of(fp64_graph.backend64())
    assert isinstance(be, nets.GraphBackend) and nets.backend_of(be) is be and nets.backend_of(nets.backend_of(be)) is be
    assert nets.backend_of(None) is nets.backend_of(None)
    # None: the stock graph, on plain torch
    P, x, _names, flows = _minimal_run("S6")
    names, flows_none = _run_core("S6", P, x, None)
    assert names == _names and all(torch.equal(a, b) for a, b in zip(flows_none, flows))
    y = nets.conv_forward(x, P["conv1.w"], P["conv1.b"], 2, 3, True, None)
    assert torch.equal(y, torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x, P["conv1.w"], P["conv1.b"], stride=2, padding=3), nets.NEG_SLOPE))
    # an op the object lacks fails where the graph calls it, by name -- not when the adapter is built, not earlier in the graph
    P, x, _names, _flows = _minimal_run("C")
    seen = []
    with torch.no_grad(), nets.listening(lambda name, y, info: seen.append(name)):
        with pytest.raises(AttributeError, match="correlation"):
            nets.flownet_c_core(P, x, x, object())
    assert seen == ["conv1", "conv2", "conv3", "conv_redir"]
    with pytest.raises(AttributeError, match="channel_norm"):
        nets.backend_of(None).channel_norm(x)
