"""FlowWarp (csrc/flow_warp.hip) against the fp64 statement of the reference (ref_torch64.flow_warp / flow_warp_backward), on every
launch branch of the host functions.

Sample positions are rounded to fp32 in both (flow_warp_layer.cu:73-74); after that the reference is fp64.  Elementwise bounds,
u = 2^-24, A = the fp64 sum of |terms| of an element, m = their number:
  * forward:        |hip - ref| <= 8u * sum_k w_k |p_k|;  outside pixels hold exactly the fill value (+0.0 or the bits 0xFFE00000)
  * image gradient: |hip - ref| <= (m + 8)u * A;          cells no source reaches hold exactly +0.0
  * flow gradient:  |hip - ref| <= (2C + 8)u * A;         pixels whose sample falls outside hold exactly +0.0
NaN patterns must be equal and infinities identical (0 * NaN and 0 * Inf poison, as in the reference).

The backward host function picks its form by channel count: C <= 8 one gather group with the flow gradient fused into it, 9-16 two
gather groups and a flow kernel with plain stores, > 16 gather groups of 8 and a flow gradient summed with float atomics after a
memset.  The gather sorts up to kWarpListMax = 24 candidate sources per cell (a fixed summation order: bit-reproducible) and walks
the lists in list order beyond that (sinks: bound only).  Tests marked gpu need the MI355X; the others check the fp64 statement
itself on the CPU.
"""
import numpy as np
import pytest
import torch

import oracle
import ref_torch64 as R
from flownet2_amd import functional, ops
from flownet2_amd.layers import Blob, LayerParameter, LayerRegistry

U = 2.0 ** -24
LIST_MAX = 24                                        # kWarpListMax, flow_warp.hip
NAN_FILL_BITS = 0xFFE00000                           # flow_warp_layer.cu:372-375
PROPS = [(True, True), (True, False), (False, True)]
CHANNELS = [1, 3, 8, 9, 16, 17, 33, 256]


def rand(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def positions(flow):
    """fp32 sample positions and the in-image mask, [N,H,W] each (the kernels' arithmetic)."""
    x2, y2 = R._positions_fp32(torch.from_numpy(np.ascontiguousarray(flow)))
    x2, y2 = x2.numpy(), y2.numpy()
    W, H = flow.shape[3], flow.shape[2]
    with np.errstate(invalid="ignore"):
        inside = (x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H)
    return x2, y2, inside


def candidates(flow):
    """Per target cell, the number of sources the gather collects: sources whose top-left tap is the cell or its left / upper /
    upper-left neighbour (the four lists warp_bwd_gather walks).  [N,H,W]"""
    N, _, H, W = flow.shape
    x2, y2, inside = positions(flow)
    heads = np.zeros((N, H + 1, W + 1), np.int64)     # one row / column of zero padding in front
    for n in range(N):
        ix = np.where(inside[n], x2[n], 0).astype(np.int64)
        iy = np.where(inside[n], y2[n], 0).astype(np.int64)
        np.add.at(heads[n], (iy[inside[n]] + 1, ix[inside[n]] + 1), 1)
    return heads[:, 1:, 1:] + heads[:, 1:, :-1] + heads[:, :-1, 1:] + heads[:, :-1, :-1]


def bounded(got, ref, bound, what, exact_zero=None):
    """Elementwise |got - ref| <= bound where ref is finite; equal NaN patterns; identical infinities; exactly +0.0 where exact_zero.
    Returns the worst error-to-bound ratio."""
    got = np.asarray(got, np.float64)
    ref, bound = np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN pattern differs at {np.argwhere(gn != rn)[:5].tolist()}"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{what}: infinities differ"
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all(), f"{what}: non-finite value where the fp64 reference is finite"
    err = np.abs(got[fin] - ref[fin])
    b = bound[fin]
    bad = err > b
    if bad.any():
        i = np.argmax(np.where(bad, err - b, -np.inf))
        where = np.argwhere(fin)[i].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements over the bound; at {where}: |{got[fin][i]!r} - {ref[fin][i]!r}| = "
                             f"{err[i]:.3e} > {b[i]:.3e}")
    if exact_zero is not None:
        z = np.broadcast_to(exact_zero, got.shape)
        assert (bits(got[z]) == 0).all(), f"{what}: {int((bits(got[z]) != 0).sum())} elements that must be exactly +0.0 are not"
    ratio = float((err / np.where(b > 0, b, 1)).max()) if err.size else 0.0
    print(f"flow_warp ratio {what}: {ratio:.3g}")
    return ratio


def ref_forward(img, flow, fill):
    """(fp64 forward, its bound) with fp32 positions; fill only matters outside, which is checked bitwise."""
    ti, tf = torch.from_numpy(np.ascontiguousarray(img)).double(), torch.from_numpy(np.ascontiguousarray(flow))
    with np.errstate(invalid="ignore"):
        ref = R.flow_warp(ti, tf, fill, fp32_positions=True).numpy()
        bound = 8 * U * R.flow_warp(ti.abs(), tf, 0.0, fp32_positions=True).numpy()
    return ref, bound


def check_forward(img, flow, fill, out, what):
    ref, bound = ref_forward(img, flow, np.nan if fill == ops.FILL_NAN else 0.0)
    _, _, inside = positions(flow)
    out = np.asarray(out)
    outside = np.broadcast_to(~inside[:, None], out.shape)
    want = NAN_FILL_BITS if fill == ops.FILL_NAN else 0
    assert (bits(out[outside]) == want).all(), f"{what}: outside pixels do not hold exactly the fill value"
    ins = ~outside
    return bounded(out[ins], ref[ins], bound[ins], what)


def check_backward(img, flow, g, prop, di, df, what, ref=None):
    """Bounds of both gradients of one (propagate_image, propagate_flow) run; a gradient that is not propagated must be all +0.0."""
    rdi, rdf, adi, mdi, adf, _ = ref if ref is not None else R.flow_warp_backward(img, flow, g)
    C = img.shape[1]
    _, _, inside = positions(flow)
    r = {}
    if prop[0]:
        r["di"] = bounded(di, rdi.numpy(), (mdi.numpy() + 8) * U * adi.numpy(), what + " image grad", exact_zero=mdi.numpy() == 0)
    else:
        assert (bits(di) == 0).all(), f"{what}: image grad not propagated but not +0.0"
    if prop[1]:
        r["df"] = bounded(df, rdf.numpy(), (2 * C + 8) * U * adf.numpy(), what + " flow grad", exact_zero=~inside[:, None])
    else:
        assert (bits(df) == 0).all(), f"{what}: flow grad not propagated but not +0.0"
    return r


def run_backward(img, flow, g, prop):
    di, df = ops.flow_warp_backward(dev(img), dev(flow), dev(g), *prop)
    return host(di), host(df)


def check_all_props(img, flow, g, what, fused_identity=True):
    """The three (propagate_image, propagate_flow) forms against one fp64 reference.  With fused_identity (C <= 16 and no cell
    beyond kWarpListMax): df of (True, True) -- fused into the gather for C <= 8 -- is bit-identical to the flow kernel's df of
    (False, True), and di of (True, True) to di of (True, False)."""
    with np.errstate(invalid="ignore", over="ignore"):
        ref = R.flow_warp_backward(img, flow, g)
    outs = {p: run_backward(img, flow, g, p) for p in PROPS}
    for p in PROPS:
        check_backward(img, flow, g, p, *outs[p], f"{what} prop={p}", ref=ref)
    if fused_identity:
        assert np.array_equal(bits(outs[(True, True)][1]), bits(outs[(False, True)][1])), f"{what}: fused and separate df differ"
        assert np.array_equal(bits(outs[(True, True)][0]), bits(outs[(True, False)][0])), f"{what}: di depends on propagate_flow"
    return outs, ref


def border_field(N, H, W, seed, scale=3.0):
    """A random flow with planted samples in the clamped last column / row, at integer positions and on the last cell."""
    flow = rand((N, 2, H, W), seed, scale)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    rng = np.random.default_rng(seed + 1)
    for n in range(N):
        pick = rng.random((H, W))
        col = pick < 0.15                                                  # x2 in [W-1, W)
        flow[n, 0][col] = (W - 1) - xs[col] + rng.random(int(col.sum())).astype(np.float32) * 0.999
        row = (pick >= 0.15) & (pick < 0.3)                                # y2 in [H-1, H)
        flow[n, 1][row] = (H - 1) - ys[row] + rng.random(int(row.sum())).astype(np.float32) * 0.999
        integ = (pick >= 0.3) & (pick < 0.4)                               # integer positions (zero-weight taps)
        flow[n][:, integ] = np.round(flow[n][:, integ])
        if W == 1:                                                         # a one-column plane: keep most samples inside
            flow[n, 0][pick < 0.8] = rng.random(int((pick < 0.8).sum())).astype(np.float32) * 0.999
        if H == 1:
            flow[n, 1][pick < 0.8] = rng.random(int((pick < 0.8).sum())).astype(np.float32) * 0.999
    return flow


# ---- the fp64 statement itself (CPU) ---------------------------------------------------------------------------------------------

def test_backward_statement_is_fp64_autograd_inside():
    """Dyadic flows make fp32 and fp64 positions equal, so the statement must equal autograd of ref_torch64.flow_warp: the image
    gradient everywhere, the flow gradient wherever the sample is outside or not in the clamped last row / column."""
    N, C, H, W = 2, 3, 7, 9
    rng = np.random.default_rng(20)
    img, g = rand((N, C, H, W), 21), rand((N, C, H, W), 22)
    flow = (np.round(rng.uniform(-4, 4, (N, 2, H, W)) * 64) / 64).astype(np.float32)
    x2, y2, inside = positions(flow)
    interior = inside & (x2 < W - 1) & (y2 < H - 1)
    assert interior.sum() > 30 and (~inside).sum() > 10 and (inside & ~interior).sum() > 5
    ti = torch.from_numpy(img).double().requires_grad_()
    tf = torch.from_numpy(flow).double().requires_grad_()
    R.flow_warp(ti, tf).backward(torch.from_numpy(g).double())
    di, df, adi, mdi, adf, mdf = R.flow_warp_backward(img, flow, g)
    np.testing.assert_allclose(di.numpy(), ti.grad.numpy(), rtol=1e-12, atol=1e-12)
    keep = np.broadcast_to((interior | ~inside)[:, None], df.shape)
    np.testing.assert_allclose(df.numpy()[keep], tf.grad.numpy()[keep], rtol=1e-12, atol=1e-12)
    # A and m: every inside source adds four terms per channel; 2C flow terms per inside pixel
    assert mdi.numpy()[:, 0].sum() == 4 * inside.sum()
    assert (adi.numpy() >= np.abs(di.numpy())).all() and (adf.numpy() >= np.abs(df.numpy())).all()
    assert np.array_equal(mdf.numpy()[:, 0], np.where(inside, 2 * C, 0))
    # the propagate switches zero their gradient only
    di2, df2 = R.flow_warp_backward(img, flow, g, propagate_image=False)[:2]
    assert (di2 == 0).all() and torch.equal(df2, df)
    di3, df3 = R.flow_warp_backward(img, flow, g, propagate_flow=False)[:2]
    assert (df3 == 0).all() and torch.equal(di3, di)


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 2, 1, 9), (1, 2, 9, 1), (1, 3, 1, 1)])
def test_backward_statement_equals_oracle_at_the_border(shape):
    """With clamped taps (last row / column, H = 1, W = 1 planes) the statement and the C oracle (fp32, reference order) agree
    within the bounds the GPU tests use, and the forward with fp32 positions agrees with the oracle's forward."""
    N, C, H, W = shape
    img, g = rand(shape, 23), rand(shape, 24)
    flow = border_field(N, H, W, 25)
    x2, y2, inside = positions(flow)
    assert (inside & ((x2 >= W - 1) | (y2 >= H - 1))).any()
    odi, odf = oracle.flow_warp_backward(img, flow, g)
    rdi, rdf, adi, mdi, adf, _ = R.flow_warp_backward(img, flow, g)
    bounded(odi, rdi.numpy(), (mdi.numpy() + 8) * U * adi.numpy(), "oracle image grad", exact_zero=mdi.numpy() == 0)
    bounded(odf, rdf.numpy(), (2 * C + 8) * U * adf.numpy(), "oracle flow grad", exact_zero=~inside[:, None])
    for fill in (oracle.FILL_ZERO, oracle.FILL_NAN):
        check_forward(img, flow, fill, oracle.flow_warp_forward(img, flow, fill), f"oracle forward fill={fill}")


def test_candidate_count_matches_the_lists():
    """The host candidate count the sink tests rely on, against a direct count of sources with a tap on the cell."""
    N, H, W = 1, 6, 7
    flow = border_field(N, H, W, 26, 2.0)
    x2, y2, inside = positions(flow)
    direct = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            if inside[0, y, x]:
                ix, iy = int(x2[0, y, x]), int(y2[0, y, x])
                for cell in {(iy, ix), (iy, min(ix + 1, W - 1)), (min(iy + 1, H - 1), ix), (min(iy + 1, H - 1), min(ix + 1, W - 1))}:
                    direct[cell] += 1
    assert np.array_equal(candidates(flow)[0], direct)


# ---- GPU: channel forms ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_backward_channel_forms(C):
    N, H, W = 2, 13, 17
    img, g = rand((N, C, H, W), 30), rand((N, C, H, W), 31)
    flow = border_field(N, H, W, 32)
    assert candidates(flow).max() <= LIST_MAX
    check_all_props(img, flow, g, f"C={C}", fused_identity=C <= 16)


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("fill", [ops.FILL_ZERO, ops.FILL_NAN])
def test_forward_channel_forms(C, fill):
    N, H, W = 2, 13, 17
    img = rand((N, C, H, W), 33)
    flow = border_field(N, H, W, 34)
    check_forward(img, flow, fill, host(ops.flow_warp_forward(dev(img), dev(flow), fill)), f"forward C={C} fill={fill}")


# ---- GPU: sinks ------------------------------------------------------------------------------------------------------------------

def _guard(flow, boxes, keep):
    """Send every source not in `keep` whose top-left tap falls in one of the cell boxes (y0, y1, x0, x1, inclusive) outside the
    image, so that only the planted sources reach the lists the sink cells read."""
    x2, y2, inside = positions(flow)
    ix, iy = np.where(inside, x2, -1).astype(np.int64), np.where(inside, y2, -1).astype(np.int64)
    for (y0, y1, x0, x1) in boxes:
        hit = inside & (iy >= y0) & (iy <= y1) & (ix >= x0) & (ix <= x1) & ~keep
        flow[:, 0][hit] = 1e4


def sink_field(kind, N=2, H=20, W=24, seed=40):
    """kind 'blocks': a 4x6 and a 5x5 block of sources that all sample one point inside a single cell (24 and 25 candidates at the
    four cells around it); kind 'lists': 6 and then 7 sources on the lists of each of four neighbouring cells (24 and 28 candidates
    at the lower-right one).  Returns (flow, {sink cell: candidates}); the rest of the field is random."""
    flow = rand((N, 2, H, W), seed, 2.5)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    keep = np.zeros((N, H, W), bool)
    boxes, sinks = [], {}
    if kind == "blocks":
        for (r0, c0, bh, bw), (py, px) in (((12, 2, 4, 6), (4.5, 5.25)), ((1, 12, 5, 5), (14.25, 17.75))):
            sl = (slice(r0, r0 + bh), slice(c0, c0 + bw))
            flow[:, 0][:, sl[0], sl[1]] = px - xs[sl]
            flow[:, 1][:, sl[0], sl[1]] = py - ys[sl]
            keep[:, sl[0], sl[1]] = True
            cy, cx = int(py), int(px)
            boxes.append((cy - 1, cy + 1, cx - 1, cx + 1))
            sinks[(cy, cx)] = bh * bw
    else:
        srcs = [(y, x) for y in range(0, 4) for x in range(W)] + [(y, x) for y in range(H - 3, H) for x in range(W)]
        it = iter(srcs)
        for (y0, x0), k in (((5, 4), 6), ((12, 15), 7)):
            for dy in (0, 1):
                for dx in (0, 1):
                    for j in range(k):
                        sy, sx = next(it)
                        fy, fx = 0.1 + 0.8 * j / k, 0.85 - 0.7 * j / k       # distinct points inside cell (y0 + dy, x0 + dx)
                        flow[:, 0, sy, sx] = np.float32(x0 + dx + fx) - np.float32(sx)
                        flow[:, 1, sy, sx] = np.float32(y0 + dy + fy) - np.float32(sy)
                        keep[:, sy, sx] = True
            boxes.append((y0 - 1, y0 + 2, x0 - 1, x0 + 2))
            sinks[(y0 + 1, x0 + 1)] = 4 * k
    _guard(flow, boxes, keep)
    return flow, sinks


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["blocks", "lists"])
@pytest.mark.parametrize("C", CHANNELS)
def test_backward_sinks(kind, C):
    flow, sinks = sink_field(kind)
    N, _, H, W = flow.shape
    cnt = candidates(flow)
    for (cy, cx), k in sinks.items():
        assert (cnt[:, cy, cx] == k).all(), (kind, (cy, cx), cnt[:, cy, cx], k)
    assert sorted(sinks.values())[0] == LIST_MAX and (cnt > LIST_MAX).any()         # both the sorted and the overflow path
    assert cnt[cnt <= LIST_MAX].max() == LIST_MAX
    img, g = rand((N, C, H, W), 41), rand((N, C, H, W), 42)
    outs, ref = check_all_props(img, flow, g, f"sink {kind} C={C}", fused_identity=False)
    di2, df2 = run_backward(img, flow, g, (True, True))
    check_backward(img, flow, g, (True, True), di2, df2, f"sink {kind} C={C} rerun", ref=ref)
    di1, df1 = outs[(True, True)]
    sorted_cells = np.broadcast_to((cnt <= LIST_MAX)[:, None], di1.shape)
    assert np.array_equal(bits(di1)[sorted_cells], bits(di2)[sorted_cells]), "image grad not reproducible where <= 24 sources meet"
    if C <= 16:
        assert np.array_equal(bits(df1), bits(df2)), "flow grad (plain stores) not reproducible"
        assert np.array_equal(bits(df1), bits(outs[(False, True)][1]))
    assert np.array_equal(bits(di1)[sorted_cells], bits(outs[(True, False)][0])[sorted_cells])


# ---- GPU: positions at the edges ---------------------------------------------------------------------------------------------------

def edge_field(N, H, W, seed):
    """Planted positions: integer x2 / y2, u = -0.0 at x = 0, x2 and y2 in [W-1, W) / [H-1, H) including the largest float below
    W (H), x2 and y2 just below 0 (outside), x2 = W exactly (outside).  Asserts on the host that the fp32 sums land there."""
    flow = rand((N, 2, H, W), seed, 1.5)
    below_w, below_h = np.nextafter(np.float32(W), np.float32(0)), np.nextafter(np.float32(H), np.float32(0))
    plant = []
    for y in range(H):
        for x in range(W):
            k = (y * W + x) % 9
            u = v = None
            if k == 0:
                u, v = np.float32(np.round(flow[0, 0, y, x])), np.float32(np.round(flow[0, 1, y, x]))
            elif k == 1 and x == 0:
                u, v = np.float32(-0.0), np.float32(-0.0)
            elif k == 2:
                u = below_w - np.float32(x)
            elif k == 3:
                v = below_h - np.float32(y)
            elif k == 4:
                u = np.float32(W - 1) - np.float32(x) + np.float32(0.5)
            elif k == 5:
                u = -np.float32(x) - np.float32(2.0 ** -30) if x == 0 else np.nextafter(-np.float32(x), np.float32(-np.inf))
            elif k == 6:
                v = -np.float32(y) - np.float32(2.0 ** -30) if y == 0 else np.nextafter(-np.float32(y), np.float32(-np.inf))
            elif k == 7:
                u = np.float32(W) - np.float32(x)
            if u is not None:
                flow[:, 0, y, x] = u
            if v is not None:
                flow[:, 1, y, x] = v
            plant.append((k, y, x))
    x2, y2, inside = positions(flow)
    for k, y, x in plant:
        if k == 2:
            assert x2[0, y, x] == below_w
        elif k == 3:
            assert y2[0, y, x] == below_h
        elif k in (5, 6):
            assert (x2 if k == 5 else y2)[0, y, x] < 0 and not inside[0, y, x]
        elif k == 7:
            assert x2[0, y, x] == W and not inside[0, y, x]
        elif k == 1 and x == 0:
            assert x2[0, y, x] == 0 and inside[0, y, x] == (0 <= y2[0, y, x] < H)
    return flow


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 9, 7, 11), (1, 3, 1, 13), (1, 3, 13, 1), (2, 17, 1, 1), (1, 17, 5, 6)])
def test_edge_positions(shape):
    N, C, H, W = shape
    flow = edge_field(N, H, W, 50)
    img, g = rand(shape, 51), rand(shape, 52)
    for fill in (ops.FILL_ZERO, ops.FILL_NAN):
        check_forward(img, flow, fill, host(ops.flow_warp_forward(dev(img), dev(flow), fill)), f"edges {shape} forward fill={fill}")
    check_all_props(img, flow, g, f"edges {shape}", fused_identity=C <= 16 and candidates(flow).max() <= LIST_MAX)


# ---- GPU: non-finite values --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 9, 17])
def test_nonfinite_flows(C):
    N, H, W = 2, 8, 10
    flow = rand((N, 2, H, W), 60, 2.0)
    bad = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32)
    rng = np.random.default_rng(61)
    for n in range(N):
        for ch in range(2):
            m = rng.random((H, W)) < 0.3
            flow[n, ch][m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    _, _, inside = positions(flow)
    assert (~inside).sum() > 20 and inside.sum() > 20
    img, g = rand((N, C, H, W), 62), rand((N, C, H, W), 63)
    for fill in (ops.FILL_ZERO, ops.FILL_NAN):
        check_forward(img, flow, fill, host(ops.flow_warp_forward(dev(img), dev(flow), fill)), f"non-finite flow C={C} fill={fill}")
    check_all_props(img, flow, g, f"non-finite flow C={C}", fused_identity=C <= 16)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 9, 17])
def test_nonfinite_image_and_grad(C):
    """NaN / Inf in the image at taps of zero weight (integer positions) and in warped_diff: the NaN pattern follows fp64."""
    N, H, W = 1, 9, 11
    flow = np.round(rand((N, 2, H, W), 70, 2.0))                           # integer positions: TR, BL, BR weigh 0 (unless clamped)
    flow[:, :, ::3] += np.float32(0.5)                                     # some half-way positions
    img, g = rand((N, C, H, W), 71), rand((N, C, H, W), 72)
    x2, y2, inside = positions(flow)
    rng = np.random.default_rng(73)
    planted = 0
    for y, x in zip(*np.nonzero(inside[0])):
        if rng.random() < 0.25 and x2[0, y, x] == int(x2[0, y, x]) and int(x2[0, y, x]) + 1 < W:
            c = int(rng.integers(0, C))
            img[0, c, int(y2[0, y, x]), int(x2[0, y, x]) + 1] = np.float32([np.nan, np.inf, -np.inf][planted % 3])   # TR: weight 0
            planted += 1
    m = rng.random(g.shape) < 0.03
    g[m] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, int(m.sum()))]
    # an infinite g whose sample sits exactly on the clamped last column / row: its zero-weight tap coincides with a weighted one,
    # and the reference's separate Inf * 0 term makes that cell NaN
    for (y, x), (py, px) in (((1, 2), (4, W - 1)), ((2, 5), (H - 1, 3)), ((6, 1), (H - 1, W - 1)), ((7, 7), (3.5, W - 1))):
        flow[0, 0, y, x], flow[0, 1, y, x] = np.float32(px - x), np.float32(py - y)
        g[0, :, y, x] = np.float32(np.inf) if y % 2 else np.float32(-np.inf)
    assert planted >= 3 and m.sum() >= 3
    for fill in (ops.FILL_ZERO, ops.FILL_NAN):
        out = host(ops.flow_warp_forward(dev(img), dev(flow), fill))
        assert np.isnan(out).any()
        check_forward(img, flow, fill, out, f"non-finite image C={C} fill={fill}")
    outs, _ = check_all_props(img, flow, g, f"non-finite image/grad C={C}", fused_identity=C <= 16)
    assert np.isnan(outs[(True, True)][0]).any() and np.isnan(outs[(True, True)][1]).any()


# ---- GPU: grid-stride branches (N * groups > 65535) ------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1025, 256, 2, 2), (65537, 1, 2, 2)])
def test_forward_grid_stride(shape):
    N, C, H, W = shape
    assert N * ((C + 3) // 4) > 65535
    img, flow = rand(shape, 80), rand((N, 2, H, W), 81, 0.8)
    check_forward(img, flow, ops.FILL_NAN, host(ops.flow_warp_forward(dev(img), dev(flow), ops.FILL_NAN)), f"forward grid-stride {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2049, 256, 2, 2), (65537, 1, 2, 2)])
def test_backward_grid_stride(shape):
    """(2049, 256): gather and flow kernel with N * ceil(C/8) > 65535; (65537, 1): N > 65535 turns the fused flow gradient off and
    adds the memset in front of the flow kernel."""
    N, C, H, W = shape
    assert N * ((C + 7) // 8) > 65535
    img, g, flow = rand(shape, 82), rand(shape, 83), rand((N, 2, H, W), 84, 0.8)
    check_all_props(img, flow, g, f"grid-stride {shape}", fused_identity=C <= 16)


# ---- GPU: production shapes ------------------------------------------------------------------------------------------------------

def smooth_flow(N, H, W, seed, amp=6.0):
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    f = np.zeros((N, 2, H, W), np.float32)
    for n in range(N):
        for c in range(2):
            a, b, p, q = rng.uniform(0.5, 3, 4)
            f[n, c] = amp * np.sin(2 * np.pi * (a * xs + p)) * np.cos(2 * np.pi * (b * ys + q))
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("flow_kind", ["smooth", "iid"])
def test_production_image_blob(flow_kind):
    N, C, H, W = 8, 3, 320, 448
    flow = smooth_flow(N, H, W, 90) if flow_kind == "smooth" else rand((N, 2, H, W), 91, 4.0)
    img, g = rand((N, C, H, W), 92), rand((N, C, H, W), 93)
    check_forward(img, flow, ops.FILL_ZERO, host(ops.flow_warp_forward(dev(img), dev(flow))), f"production {flow_kind} forward")
    cnt = candidates(flow)
    outs, ref = check_all_props(img, flow, g, f"production {flow_kind}", fused_identity=bool(cnt.max() <= LIST_MAX))
    di2, df2 = run_backward(img, flow, g, (True, True))
    sorted_cells = np.broadcast_to((cnt <= LIST_MAX)[:, None], di2.shape)
    assert np.array_equal(bits(outs[(True, True)][0])[sorted_cells], bits(di2)[sorted_cells])
    assert np.array_equal(bits(outs[(True, True)][1]), bits(df2))


@pytest.mark.gpu
def test_production_feature_blob():
    N, C, H, W = 4, 256, 48, 96
    flow = smooth_flow(N, H, W, 94, 3.0)
    img, g = rand((N, C, H, W), 95), rand((N, C, H, W), 96)
    check_forward(img, flow, ops.FILL_ZERO, host(ops.flow_warp_forward(dev(img), dev(flow))), "production feature forward")
    check_all_props(img, flow, g, "production feature", fused_identity=False)


# ---- GPU: wrappers and the C ABI -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("needs", PROPS)
def test_functional_autograd(needs):
    N, C, H, W = 2, 3, 9, 12
    img, flow, g = rand((N, C, H, W), 100), border_field(N, H, W, 101), rand((N, C, H, W), 102)
    ti, tf = dev(img).requires_grad_(needs[0]), dev(flow).requires_grad_(needs[1])
    out = functional.flow_warp(ti, tf)
    assert torch.equal(out.detach(), ops.flow_warp_forward(dev(img), dev(flow)))
    out.backward(dev(g))
    di, df = run_backward(img, flow, g, needs)
    for t, want, need in ((ti, di, needs[0]), (tf, df, needs[1])):
        if need:
            assert np.array_equal(bits(host(t.grad)), bits(want))
        else:
            assert t.grad is None


@pytest.mark.gpu
@pytest.mark.parametrize("propagate_down", [(True, True), (True, False), (False, True), (False, False)])
def test_layer_backward_gpu(propagate_down):
    N, C, H, W = 2, 9, 9, 12
    img, flow, g = rand((N, C, H, W), 103), border_field(N, H, W, 104), rand((N, C, H, W), 105)
    layer = LayerRegistry.CreateLayer(LayerParameter(name="warp", type="FlowWarp"))
    bottom, top = [Blob.from_tensor(dev(img)), Blob.from_tensor(dev(flow))], [Blob()]
    layer.SetUp(bottom, top)
    layer.Forward(bottom, top)
    top[0].mutable_gpu_diff().copy_(dev(g))
    layer.Backward_gpu(top, list(propagate_down), bottom)
    di, df = run_backward(img, flow, g, propagate_down)
    assert np.array_equal(bits(bottom[0].cpu_diff()), bits(di)) and np.array_equal(bits(bottom[1].cpu_diff()), bits(df))
    check_backward(img, flow, g, propagate_down, di, df, f"layer {propagate_down}")


@pytest.mark.gpu
def test_cabi_contract():
    from flownet2_amd import _lib
    L = _lib.lib()
    N, C, H, W = 2, 5, 6, 7
    img, flow, g = dev(rand((N, C, H, W), 110)), dev(rand((N, 2, H, W), 111)), dev(rand((N, C, H, W), 112))
    di = torch.full((N, C, H, W), 7.0, device="cuda")
    df = torch.full((N, 2, H, W), 7.0, device="cuda")
    p = ops._ptr
    nbytes = L.fn2_flow_warp_backward_workspace_bytes(N, C, H, W)
    assert nbytes == 4 * 2 * N * H * W
    short = torch.empty(nbytes - 4, dtype=torch.uint8, device="cuda")                  # one int short, from the torch allocator
    assert L.fn2_flow_warp_backward(p(img), p(flow), p(g), p(di), p(df), N, C, H, W, 1, 1, p(short), nbytes - 4, ops._stream()) == -3
    full = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert L.fn2_flow_warp_backward(p(img), p(flow), p(g), p(di), p(df), N, C, H, W, 1, 1, None, nbytes, ops._stream()) == -3
    torch.cuda.synchronize()
    assert (di == 7.0).all() and (df == 7.0).all()                                     # refused calls write nothing
    out = torch.full((N, C, H, W), 7.0, device="cuda")
    for fill in (0, 3, -1):
        assert L.fn2_flow_warp_forward(p(img), p(flow), p(out), N, C, H, W, fill, ops._stream()) == -1
    # N = 0: nothing to do, nothing written
    assert L.fn2_flow_warp_backward_workspace_bytes(0, C, H, W) == 0
    assert L.fn2_flow_warp_backward(p(img), p(flow), p(g), p(di), p(df), 0, C, H, W, 1, 1, p(full), 0, ops._stream()) == 0
    assert L.fn2_flow_warp_forward(p(img), p(flow), p(out), 0, C, H, W, ops.FILL_ZERO, ops._stream()) == 0
    torch.cuda.synchronize()
    assert (di == 7.0).all() and (df == 7.0).all() and (out == 7.0).all()
    # the full workspace is accepted
    assert L.fn2_flow_warp_backward(p(img), p(flow), p(g), p(di), p(df), N, C, H, W, 1, 1, p(full), nbytes, ops._stream()) == 0
    torch.cuda.synchronize()
    check_backward(host(img), host(flow), host(g), (True, True), host(di), host(df), "cabi")
