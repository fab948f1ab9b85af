"""The census loss, everything that needs no GPU: the binding tables, the host-only entry point and the header's refusals; the two
restatements of include/flownet2_hip_census_loss.h against each other and on hand cases; the float64 gradient against torch.autograd of a
float64 torch restatement (clamped taps, unfold); the pair symmetry; how far one NaN reaches; descent on a translated image with a
brightness offset; CensusLoss.summary, the Python refusals and the training script's flags."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import census_loss_ref as R
import unsup_loss_ref as UR
from flownet2_amd import _lib, evaluate, nets
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import CENSUS_LOSS_COL as COL, CENSUS_LOSS_COLUMNS as COLUMNS, CENSUS_LOSS_K as K
from flownet2_amd.graph_backend import GraphBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = [(1, 1, 1, 1), (1, 1, 3, 5), (3, 1, 7, 67), (2, 3, 16, 64), (1, 3, 37, 70)]      # those of tests/test_census_loss.py
WANT = ["fn2_census_loss_sizes", "fn2_census_loss_forward", "fn2_census_loss_backward"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


# ---- the header, the binding, sizes and refusals ----------------------------------------------------------------------------------
def test_header_declares_exactly_three_functions_in_tables_of_their_own():
    with open(os.path.join(_lib.INCLUDE_DIR, "flownet2_hip_census_loss.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert re.findall(r"\b(fn2_\w+)\s*\(", body) == WANT and list(_lib.CENSUS_LOSS_EXPORTS) == WANT
    assert list(_lib.CENSUS_LOSS_PROTOTYPES) == WANT and "typedef struct" not in body
    assert all(hasattr(_lib.lib(), name) for name in WANT)
    # the names are in their own tables and in none of the pinned ones, whose counts are what they were
    pinned = set(_lib.PROTOTYPES) | set(_lib.EXPORTS) | set(_lib.UNSUP_LOSS_PROTOTYPES) | set(_lib.FLOW_TRACK_PROTOTYPES)
    assert not set(WANT) & pinned and not set(_lib.CENSUS_LOSS_CONSTANTS) & (set(_lib.CONSTANTS) | set(_lib.UNSUP_LOSS_CONSTANTS))
    assert len(_lib.PROTOTYPES) == 193 and len(_lib.CONSTANTS) == 49 and len(_lib.EXPORTS) == 159 and len(_lib._STRUCTS) == 11
    assert list(_lib.UNSUP_LOSS_EXPORTS) == ["fn2_unsup_loss_sizes", "fn2_unsup_loss_forward", "fn2_unsup_loss_backward"]
    assert not any("census" in c.lower() for c in _lib._STRUCTS)
    assert COLUMNS == ("PIXELS", "COUNTED", "OCCLUDED", "OUTSIDE", "NONFINITE", "DATA_SUM", "PAIRS", "DIST_SUM") and K == 8
    assert _lib.CENSUS_LOSS_CONSTANTS == {"FN2_CENSUS_LOSS_" + n: i for i, n in enumerate(COLUMNS + ("K",))}
    proto = _lib.CENSUS_LOSS_PROTOTYPES
    assert proto["fn2_census_loss_forward"][0] is C.c_int and len(proto["fn2_census_loss_forward"][1]) == 24
    assert proto["fn2_census_loss_forward"][1][10:18] == [C.c_float] * 3 + [C.c_int] + [C.c_float] * 4
    assert len(proto["fn2_census_loss_backward"][1]) == 22 and proto["fn2_census_loss_backward"][1][8:16] == proto["fn2_census_loss_forward"][1][10:18]
    assert len(proto["fn2_census_loss_sizes"][1]) == 7


def test_sizes_are_those_of_the_tiles():
    for (H, W), tiles in (((1, 1), 1), ((3, 5), 1), ((8, 32), 1), ((9, 32), 2), ((8, 33), 2), ((37, 70), 15), ((320, 448), 560), ((384, 768), 1152)):
        assert R.tiles(H, W) == tiles
        for N in (1, 3):
            for radius in (1, 2, 3):
                saved = 2 * N * 3 * H * W
                assert R.sizes(N, H, W, radius) == (8 * K * 2 * N * min(tiles, 128) + 4 * saved, saved, K)
    nbytes = C.c_size_t(77)
    sizes = _lib.lib().fn2_census_loss_sizes
    assert sizes(0, 5, 7, 3, C.byref(nbytes), None, None) == R.INVALID and nbytes.value == 77
    assert sizes(1, 1 << 15, 1 << 15, 3, C.byref(nbytes), None, None) == R.INVALID and nbytes.value == 77
    for radius in (0, 4, -1):
        assert sizes(1, 5, 7, radius, C.byref(nbytes), None, None) == R.INVALID and nbytes.value == 77
        assert "radius" in _lib.lib().fn2_last_error_string().decode()
    assert sizes(1, 5, 7, 3, None, None, None) == R.OK


def _refusals(bufs, ws_bytes):
    """(label, expected status, what the error string must name, prefix, thunk) for every call the header says is refused on the host."""
    S, nan = (2, 3, 5, 7), float("nan")
    out = []

    def add(label, want, names, backward=None, shape=S, ws=bufs["ws"], nbytes=ws_bytes, **kw):
        blobs = {k: bufs[k] for k in ("img0", "img1", "fw", "bw", "occ_fw", "occ_bw", "results", "loss", "saved", "fw_diff", "bw_diff")}
        p = R.params()
        for k, v in kw.items():
            if k in blobs:
                blobs[k] = v
            else:
                p[k] = v
        six = [blobs[k] for k in ("img0", "img1", "fw", "bw", "occ_fw", "occ_bw")]
        fwd = lambda: R.forward(*six, shape, p, blobs["results"], blobs["loss"], blobs["saved"], ws, nbytes)
        bwd = lambda: R.backward(*six[:4], shape, p, blobs["results"], blobs["saved"], None, blobs["fw_diff"], blobs["bw_diff"])
        if backward is not True:
            out.append((label + " (forward)", want, names, "census_loss_forward:", fwd))
        if backward is not False and want != R.WORKSPACE:
            out.append((label + " (backward)", want, names, "census_loss_backward:", bwd))

    for k in ("img0", "img1", "fw", "results"):
        add(k + " NULL", R.INVALID, k, **{k: None})
    add("fw_diff NULL", R.INVALID, "fw_diff", backward=True, fw_diff=None)
    add("saved NULL", R.INVALID, "saved", backward=True, saved=None)
    add("bw_diff without a bw", R.INVALID, "bw_diff", backward=True, bw=None)
    for label, shape in (("N = 0", (0, 3, 5, 7)), ("N < 0", (-2, 3, 5, 7)), ("H = 0", (2, 3, 0, 7)), ("W < 0", (2, 3, 5, -7))):
        add(label, R.INVALID, "shape", shape=shape)
    add("C = 0", R.INVALID, "channels", shape=(2, 0, 5, 7))
    add("C = 5", R.INVALID, "channels", shape=(2, 5, 5, 7))
    add("2^31 elements", R.INVALID, "2^31", shape=(1 << 10, 2, 1 << 10, 1 << 10))
    add("2^31 elements by the channels", R.INVALID, "2^31", shape=(1 << 9, 4, 1 << 10, 1 << 10))
    add("H W alone is 2^30", R.INVALID, "2^31", shape=(1, 1, 1 << 15, 1 << 15))
    add("every extent the largest int", R.INVALID, "2^31", shape=(2 ** 31 - 1, 4, 2 ** 31 - 1, 2 ** 31 - 1))
    add("data_weight NaN", R.INVALID, "data_weight", data_weight=nan)
    add("data_weight < 0", R.INVALID, "data_weight", data_weight=-0.5)
    add("eps_d NaN", R.INVALID, "eps_d", charbonnier=(nan, 0.45))
    add("eps_d < 0", R.INVALID, "eps_d", charbonnier=(-1e-3, 0.45))
    add("gamma_d NaN", R.INVALID, "gamma_d", charbonnier=(1e-3, nan))
    add("gamma_d = 0", R.INVALID, "gamma_d", charbonnier=(1e-3, 0.0))
    add("gamma_d < 0", R.INVALID, "gamma_d", charbonnier=(1e-3, -0.45))
    for radius in (0, 4, -3):
        add("radius %d" % radius, R.INVALID, "radius", radius=radius)
    for name, pos in (("c_t", 0), ("c_h", 1)):
        for label, v in (("NaN", nan), ("= 0", 0.0), ("< 0", -0.1)):
            eps = [0.81, 0.1]
            eps[pos] = v
            add(f"{name} {label}", R.INVALID, name, census_eps=tuple(eps))
    for label, v in (("NaN", nan), ("= 0", 0.0), ("< 0", -255.0)):
        add("intensity_scale " + label, R.INVALID, "intensity_scale", intensity_scale=v)
    add("flow_mult NaN", R.INVALID, "flow_mult", flow_mult=nan)
    add("workspace NULL", R.WORKSPACE, "workspace", ws=None)
    add("workspace too small", R.WORKSPACE, "workspace", nbytes=ws_bytes - 1)
    return out


def test_every_host_refusal_writes_nothing_and_names_the_argument():
    """Refusals are decided before any launch, so they need no device: the pointers are host buffers that nobody dereferences."""
    ws_bytes, saved_floats, _ = R.sizes(2, 5, 7)
    buf = lambda n: (C.c_ubyte * n)(*([0x5A] * n))
    bufs = {k: buf(4 * 2 * c * 5 * 7) for k, c in (("img0", 3), ("img1", 3), ("fw", 2), ("bw", 2), ("occ_fw", 1), ("occ_bw", 1), ("fw_diff", 2), ("bw_diff", 2))}
    bufs.update(results=buf(8 * 2 * 3 * K), loss=buf(4), ws=buf(ws_bytes), saved=buf(4 * saved_floats))
    cases = _refusals(bufs, ws_bytes)
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels) and len(labels) >= 60
    for label, want, names, prefix, thunk in cases:
        assert thunk() == want, label
        text = _lib.lib().fn2_last_error_string().decode()
        assert text.startswith(prefix) and names in text, (label, text)
    for k, b in bufs.items():
        assert bytes(b) == b"\x5a" * len(b), k


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("kind", ["small", "large", "nonfinite"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_two_restatements_agree(shape, kind, radius):
    arrays = R.make_inputs(shape, kind, 3)
    for p in (R.params(radius=radius, **R.EXACT), R.params(radius=radius)):
        a, b = R.ref32(*arrays, p, 0.75), R.ref64(*arrays, p, 0.75)
        assert np.array_equal(a["rows"][:, :, R.COUNT_COLUMNS], b["rows"][:, :, R.COUNT_COLUMNS])
        rows = a["rows"][:, :, R.COUNT_COLUMNS[:5]]
        assert np.array_equal(rows[..., 0], rows[..., 1:].sum(-1))                  # PIXELS = COUNTED + OCCLUDED + OUTSIDE + NONFINITE
        if kind != "nonfinite":
            assert R.not_counted_share(a["rows"]) <= 1 / 3
        err, bnd = np.abs(a["rows"] - b["rows"]), b["rows_bound"]
        assert np.isfinite(bnd).all() and np.all(err <= bnd)
        assert abs(float(a["loss"]) - b["loss"]) <= b["loss_bound"]
        for d in range(2):
            assert np.isfinite(a["diff"][d]).all() and np.isfinite(b["diff_bound"][d]).all()
            assert np.all(np.abs(a["diff"][d] - b["diff"][d]) <= b["diff_bound"][d])
            # the bound is worth something: a small fraction of the largest gradient at almost every element
            assert np.median(b["diff_bound"][d]) <= 1e-2 * np.abs(b["diff"][d]).max() or not b["diff"][d].any()


def test_a_single_pixel_has_no_pairs():
    one = np.full((1, 1, 1, 1), 0.5, F)
    p = R.params(**R.EXACT)
    r = R.ref32(one, one * F(0.25), np.zeros((1, 2, 1, 1), F), p=p)
    row, eps = r["rows"][0, 0], F(p["charbonnier"][0])
    assert row[COL["COUNTED"]] == 1 and row[COL["PAIRS"]] == 0 and row[COL["DIST_SUM"]] == 0
    assert row[COL["DATA_SUM"]] == float(np.sqrt(eps * eps)) and r["loss"] == np.sqrt(eps * eps)      # psi(0)
    assert not r["rows"][1].any() and not _bits(np.abs(r["diff"][0])).any()
    assert _bits(r["planes"][0][0, :, 0, 0]).tolist() == _bits(np.array([0.5 * 255, 0.125 * 255, 0], F)).tolist()


def test_equal_images_with_zero_flow_have_no_distance_and_no_gradient():
    img = R.make_inputs((2, 3, 16, 64), "small", 3)[0]
    zero = np.zeros((2, 2, 16, 64), F)
    r = R.ref32(img, img, zero, zero, p=R.params(**R.EXACT))
    for d in range(2):
        assert all(not _bits(h).any() for h in r["h"][d].values())                  # every h is +0.0f
        assert not _bits(np.abs(r["diff"][d])).any() and r["rows"][d, -1, COL["DIST_SUM"]] == 0
        assert r["rows"][d, -1, COL["COUNTED"]] == 2 * 16 * 64
        assert r["rows"][d, -1, COL["PAIRS"]] == 2 * sum((16 - abs(dy)) * (64 - abs(dx)) for dx, dy in R.offsets(3))


def test_one_row_by_hand():
    """[1,1,1,4], radius 1, zero flow, intensity_scale 1 (G = I0, Wg = I1), c_t = 16, c_h = 0.64.  I0 = (0, 3, 3, 0), I1 = (0, 0, 3, 3): every
    difference is 0 or +-3, so t = 0 or +-3 / sqrt(9 + 16) = +-0.6 and, in every pair, exactly one of ta, tb is zero: e = +-0.6, h =
    0.36 / (0.36 + 0.64) = 0.36.  Pixels 0 and 3 have one neighbour, 1 and 2 have two: dist = (0.36, 0.72, 0.72, 0.36), six pairs."""
    img0 = np.array([0, 3, 3, 0], F).reshape(1, 1, 1, 4)
    img1 = np.array([0, 0, 3, 3], F).reshape(1, 1, 1, 4)
    p = R.params(radius=1, census_eps=(16.0, 0.64), intensity_scale=1.0, charbonnier=(0.0, 0.5))
    r = R.ref32(img0, img1, np.zeros((1, 2, 1, 4), F), p=p)
    t = F(3) / np.sqrt(F(3) * F(3) + F(16))
    s = t * t
    h = s / (s + F(0.64))
    assert abs(float(h) - 0.36) <= 4 * R.U
    row = r["rows"][0, 0]
    assert row[COL["COUNTED"]] == 4 and row[COL["PAIRS"]] == 6
    assert _bits(r["planes"][0][0, 0]).tolist() == _bits(img0[0, 0]).tolist() and _bits(r["planes"][0][0, 1]).tolist() == _bits(img1[0, 0]).tolist()
    dist = np.array([h, h + h, h + h, h], F)
    assert row[COL["DIST_SUM"]] == float(dist.astype(np.float64).sum())
    assert row[COL["DATA_SUM"]] == row[COL["DIST_SUM"]]                             # eps = 0, gamma = 0.5: psi(t) = |t|
    assert _bits(r["planes"][0][0, 2]).tolist() == _bits(np.ones((1, 4), F)).tolist() and r["loss"] == F(row[COL["DATA_SUM"]] / 4)      # psi' = 1
    assert [float(v[0, 0, x]) for x in range(4) for q, v in sorted(r["h"][0].items()) if q in ((-1, 0), (1, 0)) and 0 <= x + q[0] < 4] == [float(h)] * 6
    # occ and a NaN: pixel 1 occluded keeps its grey values, so its neighbours keep their pairs; a NaN in I0 at 1 takes them away
    occ = R.ref32(img0, img1, np.zeros((1, 2, 1, 4), F), occ_fw=np.array([0, 1, 0, 0], F).reshape(1, 1, 1, 4), p=p)["rows"][0, 0]
    assert occ[COL["OCCLUDED"]] == 1 and occ[COL["COUNTED"]] == 3 and occ[COL["PAIRS"]] == 4
    bad = img0.copy()
    bad[0, 0, 0, 1] = np.nan
    nanrow = R.ref32(bad, img1, np.zeros((1, 2, 1, 4), F), p=p)["rows"][0, 0]
    assert nanrow[COL["NONFINITE"]] == 1 and nanrow[COL["COUNTED"]] == 3 and nanrow[COL["PAIRS"]] == 2


def test_an_additive_brightness_offset_changes_no_bit_where_brightness_constancy_pays():
    """Values on multiples of 1/256 below 1, C = 3 (gsc = 85) and flows of whole pixels (bilinear weights 0 and 1): every grey value is
    exact in float32 with and without an offset of 0.25 on img1, so every difference inside a patch is the same number."""
    rng = np.random.default_rng(11)
    shape = (2, 3, 9, 21)
    img0, img1 = ((rng.integers(0, 129, shape) / 256.0).astype(F) for _ in range(2))
    fw, bw = np.zeros((2, 2, 9, 21), F), np.zeros((2, 2, 9, 21), F)
    fw[:, 0], bw[:, 0], bw[:, 1] = 1.0, -1.0, 2.0
    p = R.params(**R.EXACT)
    plain, lifted = R.ref32(img0, img1, fw, bw, p=p), R.ref32(img0, img1 + F(0.25), fw, bw, p=p)
    assert plain["rows"][:, -1, COL["DIST_SUM"]].min() > 0 and plain["rows"][0, -1, COL["OUTSIDE"]] == 2 * 9
    assert np.array_equal(_bits(plain["rows"]), _bits(lifted["rows"])) and _bits(plain["loss"]) == _bits(lifted["loss"])
    for d in range(2):
        assert np.array_equal(_bits(plain["diff"][d]), _bits(lifted["diff"][d])) and np.abs(plain["diff"][d]).max() > 0
        assert np.array_equal(_bits(plain["planes"][d][:, 2]), _bits(lifted["planes"][d][:, 2]))
    up = UR.params(smooth_weight=0.0, **UR.EXACT)
    a, b = UR.ref32(img0, img1, fw, bw, p=up)["rows"], UR.ref32(img0, img1 + F(0.25), fw, bw, p=up)["rows"]
    assert np.all(a[:, -1, UR.COL["DATA_SUM"]] != b[:, -1, UR.COL["DATA_SUM"]])


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_pair_symmetry(radius):
    arrays = R.make_inputs((1, 3, 37, 70), "nonfinite", 5)
    r = R.ref32(*arrays, p=R.params(radius=radius, **R.EXACT))
    seen = 0
    for d in range(2):
        for (dx, dy), h in r["h"][d].items():
            back = R.at(r["h"][d][(-dx, -dy)], dx, dy)                              # h(p + q, -q), at p
            assert np.array_equal(_bits(h), _bits(back))
            seen += int((h != 0).sum())
    assert seen > 1000


# ---- the gradient -----------------------------------------------------------------------------------------------------------------
def _torch_loss(arrays, p, leaves):
    """The loss of the header as a float64 torch graph of the two flows (`leaves`: float64 tensors), every decision and tap index taken
    from decide: bilinear interpolation with clamped taps, the patches with unfold, means over the counted pixels."""
    img0, img1, fw, bw, occ_fw, occ_bw = arrays
    T = lambda a: torch.from_numpy(np.where(np.isfinite(a) & (np.abs(a) <= 1e9), a, 0).astype(np.float64))
    eps_d, gam_d = float(F(p["charbonnier"][0])), float(F(p["charbonnier"][1]))
    c_t, c_h = float(F(p["census_eps"][0])), float(F(p["census_eps"][1]))
    mult, r = float(F(p["flow_mult"])), int(p["radius"])
    k = 2 * r + 1
    total = 0.0
    for (Ia, Io, a32, occ), leaf in zip(((img0, img1, fw, occ_fw), (img1, img0, bw, occ_bw)), leaves):
        N, Cc, H, W = Ia.shape
        gsc = float(F(p["intensity_scale"]) / F(Cc))
        dec = R.decide(Ia, Io, a32, occ, p)
        ixL, ixR, iyT, iyB = (torch.from_numpy(t.astype(np.int64)) for t in dec["taps"])
        a = leaf * mult
        x2 = a[:, 0] + torch.arange(W, dtype=torch.float64)[None, None, :]
        y2 = a[:, 1] + torch.arange(H, dtype=torch.float64)[None, :, None]
        al, be = x2 - ixL, y2 - iyT
        n_idx = torch.arange(N)[:, None, None]
        G, Wg = 0.0, 0.0
        for c in range(Cc):
            o = T(Io[:, c])
            tap = lambda iy, ix: o[n_idx, iy, ix]
            Wg = Wg + ((1 - al) * (1 - be) * tap(iyT, ixL) + al * (1 - be) * tap(iyT, ixR) + (1 - al) * be * tap(iyB, ixL) + al * be * tap(iyB, ixR))
            G = G + T(Ia[:, c])
        G, Wg = G * gsc, Wg * gsc
        patches = lambda t: torch.nn.functional.unfold(t[:, None], k, padding=r).reshape(N, k * k, H, W)      # row-major over (dy, dx)
        da, db = patches(G) - G[:, None], patches(Wg) - Wg[:, None]
        e = da / torch.sqrt(da * da + c_t) - db / torch.sqrt(db * db + c_t)
        h = e * e / (e * e + c_h)
        mask = np.zeros((N, k * k, H, W), bool)
        for (dx, dy), ex in dec["exists"].items():
            mask[:, (dy + r) * k + dx + r] = ex
        dist = torch.where(torch.from_numpy(mask), h, torch.zeros_like(h)).sum(1)
        counted = torch.from_numpy(dec["cls"] == 0)
        psi = (dist * dist + eps_d * eps_d) ** gam_d
        total = total + float(F(p["data_weight"])) * torch.where(counted, psi, torch.zeros_like(psi)).sum() / max(int(counted.sum()), 1)
    return total


def _off_the_grid(shape, kind, seed):
    """make_inputs with every target moved at least 1e-3 away from whole coordinates, where the bilinear interpolant has a kink."""
    arrays = R.make_inputs(shape, kind, seed)
    for a in arrays[2:4]:
        ok = np.isfinite(a)
        frac = np.where(ok, a, 0) - np.floor(np.where(ok, a, 0))                    # the pixel's own coordinate is whole
        a[ok & ((frac < 2e-3) | (frac > 1 - 2e-3))] += F(0.01)
    return arrays


@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("kind", ["small", "large", "nonfinite"])
@pytest.mark.parametrize("shape", [(1, 1, 3, 5), (3, 1, 7, 67), (2, 3, 16, 64)], ids=lambda s: "x".join(map(str, s)))
def test_float64_gradient_equals_autograd(shape, kind, radius):
    arrays = _off_the_grid(shape, kind, 4)
    p = R.params(radius=radius, flow_mult=1.0, data_weight=0.75)
    want = R.ref64(*arrays, p, 1.0)
    clean = lambda a: np.where(np.isfinite(a) & (np.abs(a) <= 1e9), a, 0).astype(np.float64)
    leaves = [torch.from_numpy(clean(arrays[2])).requires_grad_(True), torch.from_numpy(clean(arrays[3])).requires_grad_(True)]
    loss = _torch_loss(arrays, p, leaves)
    loss.backward()
    assert abs(float(loss.detach()) - want["loss"]) <= 1e-12 * abs(want["loss"])
    for d in range(2):
        got, ref = leaves[d].grad.numpy(), want["diff"][d]
        scale = np.abs(ref).max()
        assert scale > 0 and np.abs(got - ref).max() <= 1e-10 * scale, f"direction {d}: {np.abs(got - ref).max():.3e} of {scale:.3e}"


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_one_nan_reaches_twice_the_radius_and_no_further(radius):
    """With the normaliser held fixed (data_weight = COUNTED * 2^-12).  The gradient at r holds pd(r + q) of every pixel of r's patch, and
    pd(r + q) = psi'(dist(r + q)) moves when a pair of r + q's own patch goes: a pixel radius + 1 away changes, one 2 radius + 1 away
    does not."""
    arrays = R.make_inputs((1, 3, 24, 40), "small", 3)
    arrays[2][0, :, 8:17, 16:25] = F(0.25)
    arrays[4][0, 0] = 0
    y, x = 12, 20
    bad = [a.copy() for a in arrays]
    bad[2][0, 1, y, x] = np.nan
    diffs = []
    for case in (arrays, bad):
        case = case[:3] + [None, case[4], None]
        c = R.ref32(*case, p=R.params(radius=radius, **R.EXACT))["rows"][0, -1, COL["COUNTED"]]
        diffs.append(R.ref32(*case, p=R.params(radius=radius, data_weight=c * 2.0 ** -12, **R.EXACT))["diff"][0])
    changed = (_bits(diffs[0]) != _bits(diffs[1]))[0].any(0)
    yy, xx = np.mgrid[:24, :40]
    cheb = np.maximum(np.abs(yy - y), np.abs(xx - x))
    assert not changed[cheb > 2 * radius].any() and changed[cheb == radius + 1].any() and changed[cheb <= radius].any()


def test_descent_on_a_translated_image_with_a_brightness_offset():
    """R.DESCENT has the step size, the image and the figures of this run."""
    img0, img1 = R.descent_images()
    p = R.params()
    fw = np.zeros((1, 2, 16, 32), F)
    before = (R.ref64(img0, img1, fw, p=p)["loss"], R.descent_epe(fw, p)[0])
    for _ in range(R.DESCENT["steps"]):
        fw = (fw - R.DESCENT["step"] * R.ref64(img0, img1, fw, p=p)["diff"][0]).astype(F)
    after = (R.ref64(img0, img1, fw, p=p)["loss"], R.descent_epe(fw, p)[0])
    print(f"descent: loss {before[0]:.6f} -> {after[0]:.6f}, EPE {before[1]:.6f} -> {after[1]:.6f}")
    assert before[1] == 2.0 and after[0] < before[0] and after[1] < before[1]
    assert abs(after[0] - 3.001585) < 1e-3 and abs(after[1] - 1.540722) < 1e-3      # the figures recorded in R.DESCENT


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_device():
    z, fl = torch.zeros(1, 3, 4, 5), torch.zeros(1, 2, 4, 5)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.census_loss(z, z, fl)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.census_loss_report(z, z, fl)
    with pytest.raises(RuntimeError, match="gets no gradient"):
        Fn.census_loss(z.clone().requires_grad_(True), z, fl)
    with pytest.raises(RuntimeError, match="occ_fw gets no gradient"):
        Fn.census_loss(z, z, fl, occ_fw=torch.zeros(1, 1, 4, 5, requires_grad=True))
    with pytest.raises(ValueError, match="data_term must be"):
        Fn.unsupervised_loss(z, z, fl, data_term="gradient")
    with pytest.raises(ValueError, match='data_term is "brightness"'):
        Fn.unsupervised_loss(z, z, fl, census=dict(radius=2))
    with pytest.raises(ValueError, match="not \\['eps'\\]"):
        Fn.unsupervised_loss_report(z, z, fl, data_term="census", census=dict(eps=1))
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.unsupervised_loss(z, z, fl, data_term="census", census=dict(radius=2))
    assert "census_loss" in GraphBackend.FORWARDED and nets.backend_of(Fn).has_census_loss

    class OnlyBrightness:
        unsupervised_loss = staticmethod(Fn.unsupervised_loss)
    assert not GraphBackend(OnlyBrightness()).has_census_loss and GraphBackend(OnlyBrightness()).has_unsupervised_loss
    with pytest.raises(RuntimeError, match="no census_loss op"):
        nets.unsupervised_loss({2: z}, {2: z}, z, z, GraphBackend(OnlyBrightness()), data_term="census")
    import flownet2_amd
    assert flownet2_amd.census_loss is Fn.census_loss and flownet2_amd.census_loss_report is Fn.census_loss_report
    assert flownet2_amd.CensusLoss is evaluate.CensusLoss
    assert {"census_loss", "census_loss_report", "CensusLoss"} <= set(flownet2_amd.__all__)


def test_summary_by_hand():
    def row(**kw):
        out = np.zeros(K)
        for k, v in kw.items():
            out[COL[k]] = v
        return out
    fw = [row(PIXELS=100, COUNTED=50, OCCLUDED=30, OUTSIDE=15, NONFINITE=5, DATA_SUM=25.0, PAIRS=2000, DIST_SUM=100.0),
          row(PIXELS=100, COUNTED=100, DATA_SUM=50.0, PAIRS=4000, DIST_SUM=500.0)]
    c = evaluate.CensusLoss(fw, None, loss=1.5, data_weight=2.0, radius=2)
    s = c.summary()
    assert len(c) == 2 and s["samples"] == 2 and s["loss"] == 1.5 and s["data_weight"] == 2.0 and s["radius"] == 2
    assert s["fw"] == {"data_mean": 0.5, "dist_mean": 4.0, "pairs_mean": 40.0, "counted": 0.75, "occluded": 0.15, "outside": 0.075,
                       "nonfinite": 0.025, "pixels": 200}
    assert s["bw"]["pixels"] == 0 and np.isnan(s["bw"]["data_mean"]) and np.isnan(s["bw"]["pairs_mean"])
    with pytest.raises(ValueError, match="must be"):
        evaluate.CensusLoss(np.zeros((2, K + 1)))
    with pytest.raises(ValueError, match="backward rows"):
        evaluate.CensusLoss(np.zeros((2, K)), np.zeros((1, K)))
    u = evaluate.UnsupLoss(np.zeros((2, 8)), None, loss=2.0, data_weight=0.0, census=c)
    assert u.summary()["census"] == s and "census" not in evaluate.UnsupLoss(np.zeros((2, 8))).summary()


def test_the_training_script_takes_the_new_flags():
    spec = importlib.util.spec_from_file_location("train_pipeline", os.path.join(ROOT, "scripts", "train_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    a = ap.parse_args([])
    assert a.unsup_data == "brightness" and a.census_radius == 3 and a.unsupervised is False
    a = ap.parse_args(["--unsupervised", "--unsup-data", "census", "--census-radius", "2"])
    assert a.unsupervised and a.unsup_data == "census" and a.census_radius == 2
    for bad in (["--unsup-data", "gradient"], ["--census-radius", "4"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
