"""fn2_predict_upsample_flow_forward_into (csrc/flow_head.hip): the predict_flow gather and the upsample_flow behind it in one launch must
give the bits of the two entry points run back to back -- the flow, and the up-sampled slice of the Concat blob, whose other channels stay
untouched -- for every number of channel splits; and the decoder graph that uses it computes what it computed."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from flownet2_amd import nets

NS = (1, 3)
# 8, 130, 300 channels give 1 and 2 channel splits on these maps (a split needs 256 channels per doubling); 520 and 1030 give 4 and 8
CS = (8, 130, 300, 520, 1030)
MAPS = ((5, 7), (6, 8), (10, 14))


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def nsplit_of(N, C, H, W):
    from flownet2_amd import _lib
    L = _lib.lib()
    return int(L.fn2_predict_flow_conv_workspace_bytes(N, C, H, W)) // (4 * N * 18 * H * W)


@pytest.mark.gpu
def test_shapes_cover_every_split_count():
    seen = {nsplit_of(N, C, H, W) for N in NS for C in CS for (H, W) in MAPS}
    assert seen == {1, 2, 4, 8}
    assert {nsplit_of(N, C, H, W) for N in NS for C in CS[:3] for (H, W) in MAPS} == {1, 2}


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C", CS)
def test_one_launch_equals_the_two_entry_points_bitwise(C, N):
    from flownet2_amd import ops
    dv = lambda a: torch.from_numpy(a).cuda()
    for (H, W) in MAPS:
        x, w, b = dv(rnd((N, C, H, W), 1 + C)), dv(rnd((2, C, 3, 3), 2, 0.1)), dv(rnd((2,), 3))
        uw, ub = dv(rnd((2, 2, 4, 4), 4, 0.5)), dv(rnd((2,), 5))
        for bias, up_bias in ((b, ub), (None, None)):
            flow_ref = ops.predict_flow_conv_forward(x, w, bias)
            top_ref = torch.full((N, 9, 2 * H, 2 * W), float("nan"), device="cuda")            # poison: the channels outside the slice
            ops.upsample_flow_deconv_forward(flow_ref, uw, up_bias, out=top_ref, out_c0=3)
            top = torch.full((N, 9, 2 * H, 2 * W), float("nan"), device="cuda")
            flow = ops.predict_upsample_flow_forward(x, w, bias, uw, up_bias, top, 3)
            assert flow is not None, "the one-launch form declined a decoder shape"
            assert torch.equal(bits(flow), bits(flow_ref)), (N, C, H, W)
            assert torch.equal(bits(top[:, 3:5]), bits(top_ref[:, 3:5])), (N, C, H, W)
            assert torch.equal(bits(top), bits(top_ref)), (N, C, H, W)                          # NaN bits and all: nothing else was written
            assert bool(torch.isfinite(top[:, 3:5]).all()) and bool(torch.isnan(top[:, :3]).all()) and bool(torch.isnan(top[:, 5:]).all())


@pytest.mark.gpu
def test_functional_form_declines_under_autograd():
    from flownet2_amd import functional as Fn
    dv = lambda a: torch.from_numpy(a).cuda()
    x, w, b, uw, ub = dv(rnd((1, 8, 6, 8), 1)), dv(rnd((2, 8, 3, 3), 2)), dv(rnd((2,), 3)), dv(rnd((2, 2, 4, 4), 4)), dv(rnd((2,), 5))
    top = torch.zeros((1, 4, 12, 16), device="cuda")
    assert Fn.predict_upsample_flow(x, w.requires_grad_(True), b, uw, ub, top, 2) is None
    with torch.no_grad():
        flow = Fn.predict_upsample_flow(x, w, b, uw, ub, top, 2)
    assert torch.equal(bits(flow), bits(Fn.predict_flow_conv(x, w.detach(), b)))


def _torch_heads(fused):
    """A backend of plain torch ops with the flow heads' `out=` form; fused: how predict_upsample_flow answers (None: it has none)."""
    calls = []

    def predict_flow_conv(x, w, b=None):
        calls.append("predict")
        return F.conv2d(x, w, b, padding=1)

    def upsample_flow_deconv(x, w, b=None, out=None, out_c0=0):
        calls.append("upsample")
        y = F.conv_transpose2d(x, w, b, stride=2, padding=1)
        if out is None:
            return y
        out[:, out_c0:out_c0 + 2] = y
        return out[:, out_c0:out_c0 + 2]

    ns = types.SimpleNamespace(predict_flow_conv=predict_flow_conv, upsample_flow_deconv=upsample_flow_deconv)
    if fused is not None:
        def predict_upsample_flow(x, w, b, uw, ub, out, out_c0):
            calls.append("fused")
            if not fused:
                return None
            flow = F.conv2d(x, w, b, padding=1)
            out[:, out_c0:out_c0 + 2] = F.conv_transpose2d(flow, uw, ub, stride=2, padding=1)
            return flow
        ns.predict_upsample_flow = predict_upsample_flow
    return ns, calls


@pytest.mark.parametrize("fused", (None, False, True))
def test_head_into_stage_is_the_composition_of_the_two_ops(fused):
    """nets._head_into_stage on the host: with a Concat blob and no autograd the flow is up-sampled into the blob's last two channels --
    by the backend's one-launch form, or where it has none or declines, by the two ops; with autograd, or without a blob, nothing but
    predict_flow runs."""
    from flownet2_amd.graph_backend import backend_of
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    P = {"p.w": r(2, 6, 3, 3), "p.b": r(2), "d.w": r(6, 3, 4, 4), "d.b": r(3), "u.w": r(2, 2, 4, 4), "u.b": r(2)}
    x, s = r(2, 6, 5, 7), r(2, 4, 10, 14)
    want_flow = F.conv2d(x, P["p.w"], P["p.b"], padding=1)
    want_up = F.conv_transpose2d(want_flow, P["u.w"], P["u.b"], stride=2, padding=1)
    obj, calls = _torch_heads(fused)
    be = backend_of(obj)
    blob = torch.full((2, 4 + 3 + 2, 10, 14), 7.0)
    with torch.no_grad():
        flow, up = nets._head_into_stage(P, x, "p", (blob, s), "d", "u", be)
    assert up is True and torch.equal(flow, want_flow) and torch.equal(blob[:, 7:], want_up) and bool((blob[:, :7] == 7).all())
    assert calls == {None: ["predict", "upsample"], False: ["fused", "predict", "upsample"], True: ["fused"]}[fused]
    # no blob, or a gradient to carry: the head alone, the stage up-samples as before
    del calls[:]
    with torch.no_grad():
        flow, up = nets._head_into_stage(P, x, "p", s, "d", "u", be)
    assert up is False and torch.equal(flow, want_flow) and calls == ["predict"]
    del calls[:]
    Pg = dict(P, **{"u.w": P["u.w"].clone().requires_grad_(True)})
    flow, up = nets._head_into_stage(Pg, x, "p", (blob, s), "d", "u", be)
    assert up is False and calls == ["predict"]


def test_flownetc_graph_on_the_cpu_oracle_backend_is_unchanged():
    """deploy_forward("C") of a 64x64 pair on the CPU oracle backend: the decoder with _head_into_stage gives the bits of the decoder that
    calls predict_flow and leaves the up-sampling to the stage (the graph before the one-launch form)."""
    from oracle import backend as cpu_backend
    rng = np.random.default_rng(0)
    P = nets.init_params("C", seed=0, device="cpu")
    img0 = torch.from_numpy(rng.integers(0, 256, (1, 3, 64, 64)).astype(np.float32))
    img1 = torch.from_numpy(rng.integers(0, 256, (1, 3, 64, 64)).astype(np.float32))
    with torch.no_grad():
        got = nets.deploy_forward("C", P, img0, img1, cpu_backend)
        keep = nets._head_into_stage
        nets._head_into_stage = lambda P, x, pname, skip, dname, uname, be: (be.predict_flow(x, P, pname), False)
        try:
            want = nets.deploy_forward("C", P, img0, img1, cpu_backend)
        finally:
            nets._head_into_stage = keep
    assert got.shape == (1, 2, 64, 64) and bool(torch.isfinite(got).all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
