"""DataAugmentation (csrc/data_augmentation.hip) and FlowAugmentation (csrc/augmentation.hip) against their fp64 statements
(augmentation_bounds: plain NumPy float64 with a running first-order error next to every value), element by element, on every launch
branch of the two host functions.  Inputs are random, not smooth: rng.random images (for the colour cases with two channels of a pixel at
least 0.25 apart) and standard-normal flows x 8.  No comparison uses a quantile.  The only elements left out are the pixels whose fp64 s
or l lies within its running error of the per-pixel threshold 1e-2f (a discontinuity), at most 0.5 % of a case's pixels (asserted; the
cases here leave out none or a handful).  The bounds are described in augmentation_bounds; the 2x margin of the colour chains and the
E_POW ulps assumed for cosf / sinf / logf are stated there.

Branches (augmentation_bounds restates vec4, per_sample, bx, rows and the chunking; every case asserts what it is meant to select, and
  test_plan_matches_the_c_api holds the restatement against fn2_data_augmentation_workspace_bytes): no cropping with each mean mode;
  C = 1, 2, 4, 6 (the nc tail and the c0 loop); each mean mode under "all"; the statistics pass with 16-byte loads, scalar because
  H W % 4 != 0, scalar because the bottom is 4-byte aligned, bx > 1, capped at per_sample = 3 and 1 with grid-stride trips; more than 256
  rows in eigenspace_finish; item chunks of 16 (N = 16, 17, 35) and a <NOISE = false> chunk next to a <true> one; clamped positions;
  a near-black batch on the other side of every batch threshold; a second run in other allocations (the same bits, mean_rgb included:
  no atomics).  FlowAugmentation: identity, ordinary coefficients, the 64-sample chunk boundary (N = 65, 129), taps left of, right of,
  above and below the image, before the first and past the last sample, W odd with mirror on both images.
  Not reached: the grid-stride trip of data_aug_kernel and flow_aug_warp.  Their cap is 2^20 workgroups, so a trip needs more than 2.6e8
  output pixels, which no test of a few seconds has; the cap is not lowered for a test.

The C oracle is a second fp32 implementation and is held to the same statements on the CPU.  Its mean_rgb is ONE sequential fp32 sum
  over N H W terms, so its own d is N H W and its bound is wider than the kernel's (d from the launch plan); at the large statistics
  cases that bound is wide enough to be of little use (300 x 56 x 56: 5.6 % of A; under such an error half or all of the pixels count as
  being at a threshold, so the 0.5 % cap is asserted for the kernel's statement and not for the oracle's), which is why only an fp64
  statement can tell which of the two is right.  The oracle stays as the statement of the reference's arithmetic.
Teeth: eight mutations of the statements each push the oracle's output outside the bound on the case meant for it
  (test_teeth_*), so the bounds, not the inputs, are what lets a correct kernel pass.

Fixed with these tests: fn2_data_augmentation_forward launched eigenspace_init (a write of the workspace's record) before its
  "blob too large for the statistics pass" refusal; the check now stands in front of the launch like every other refusal
  (test_refusals_leave_top_and_workspace: every reachable refusal leaves top and the workspace as they were).

Worst error / bound on the MI355X (this file's printed ratios; recorded only, no bound is derived from them):
  data_aug_kernel, copy: 0 (bits); copy + mean per pixel 0.99, per channel 0.98 (one rounding against a bound of one rounding).
  data_aug_kernel, spatial only: C = 1 0.25, C = 2 0.33, C = 4 + mean 0.37, C = 6 + per-pixel mean 0.26; clamped positions 0.20.
  data_aug_kernel, colour chains: chromatic 0.036; shadow 0.17; noise 0.14; <false> chunk next to a <true> one 0.17; eigen with
    col_angle 0.005 (its twin without, stats_vec4: 0.006: the assumed ulps of cosf / sinf hold); "all" with mean none / per channel / per
    pixel 0.005 / 0.006 / 0.005; near-black batch 0.020; N = 16 / 17 / 35: 0.010 / 0.009 / 0.011.
  eigenspace_stats + eigenspace_finish by branch (the pixel chain behind them in brackets): 16-byte loads, bx = 1 (0.006); scalar,
    H W % 4 != 0 (0.007); scalar, 4-byte aligned bottom (0.007); bx = 3 (0.014); per_sample = 3 with two trips (0.012, one pixel of 10,800
    left out); per_sample = 1, scalar, eight trips (0.014); 300 rows in the finish (0.016); bx = 33, 264 rows (0.022).  The record over
    all of them: mean_rgb 0.084, max_abs_eig 0.37, mean_eig 0.038, max_l 0.083, max_rgb / min_rgb the same bits.
  The pixel chain from the RECORDED statistics (no statistics error in the bound): 0.008 - 0.045.
  The colour chains stay far below 1 because most of their bound is the position error ep of the sampling (worst case 3u of the three
  terms; the realised one is a fraction of an ulp of the sum), carried through the divisions by max_abs_eig, s and l.
  flow_aug_warp: identity 0.19, ordinary 0.46, N = 65 0.48, N = 129 0.51, taps outside 0.32, W odd with mirror 0.34; one tap candidate
    everywhere (no position within its error of a half-integer in these cases).
Tests marked gpu need the MI355X; the others check the plans, the caps, the statements against the C oracle and the teeth on the CPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import augmentation_bounds as B
import oracle
from flownet2_amd import _lib, ops

CAP = 0.005
# chromatic_eigvec of the published FlowNet2 training prototxts (rows: the eigenvectors)
EIGVEC = (0.51, 0.56, 0.65, 0.79, 0.01, -0.62, 0.35, -0.83, 0.44)

KIND = dict(
    spatial={},
    chromatic=dict(gamma=0.8, brightness=0.05, contrast=1.3, color1=1.2, color2=0.9, color3=1.1),
    eigen=dict(pow_nomean0=1.2, pow_nomean1=0.8, pow_nomean2=1.1, add_nomean0=0.02, add_nomean1=-0.03, add_nomean2=0.01, mult_nomean0=1.1,
               mult_nomean1=0.9, mult_nomean2=1.2, pow_withmean0=0.9, add_withmean0=0.03, mult_withmean0=1.1, pow_withmean1=1.2,
               add_withmean1=0.02, mult_withmean1=0.9, lmult_pow=0.8, lmult_add=0.05, lmult_mult=1.1),
    shadow=dict(shadow_angle=0.0, shadow_distance=1.0, shadow_strength=0.3),       # nx = 1, ny = 0, integer distance: the edge is exact
    noise=dict(noise=0.05),
)
KIND["eigen_angle"] = dict(KIND["eigen"], col_angle=0.3)
KIND["all"] = dict(KIND["chromatic"], **KIND["eigen_angle"], **KIND["shadow"], **KIND["noise"])

# name: bottom shape, crop (None: no cropping), kind, then options: mean (FN2_MEAN_*), aligned, scale, only (samples that get the kind;
# default: all but sample 1, which keeps default colour coefficients and is dragged through the colour kernel by the batch flags), spatial
DATA_CASES = {
    "copy": ((2, 3, 5, 7), None, "all", {}),
    "copy_mean_pixel": ((2, 3, 5, 7), None, "all", dict(mean=2)),
    "copy_mean_channel": ((2, 5, 4, 6), None, "spatial", dict(mean=1)),
    "spatial_c1": ((2, 1, 12, 15), (8, 10), "spatial", {}),
    "spatial_c2": ((2, 2, 12, 15), (8, 10), "spatial", {}),
    "spatial_c4": ((2, 4, 12, 15), (8, 10), "spatial", dict(mean=1)),
    "spatial_c6": ((2, 6, 12, 15), (8, 10), "spatial", dict(mean=2)),
    "all_mean_none": ((3, 3, 20, 24), (16, 20), "all", {}),
    "all_mean_channel": ((3, 3, 20, 24), (16, 20), "all", dict(mean=1)),
    "all_mean_pixel": ((3, 3, 20, 24), (16, 20), "all", dict(mean=2)),
    "chromatic": ((2, 3, 10, 12), (8, 8), "chromatic", {}),
    "shadow": ((2, 3, 10, 12), (8, 8), "shadow", {}),
    "noise": ((2, 3, 10, 12), (8, 8), "noise", {}),
    "eigen_angle": ((2, 3, 8, 8), (6, 6), "eigen_angle", {}),
    "stats_vec4": ((2, 3, 8, 8), (6, 6), "eigen", {}),
    "stats_odd": ((2, 3, 9, 7), (6, 6), "eigen", {}),
    "stats_misaligned": ((2, 3, 8, 8), (6, 6), "eigen", dict(aligned=False)),
    "stats_bx": ((2, 3, 40, 52), (8, 8), "eigen", {}),
    "stats_cap3": ((300, 3, 56, 56), (6, 6), "eigen", {}),
    "stats_cap1": ((1024, 3, 45, 45), (4, 4), "eigen", dict(seed=2)),        # (the seed: a powf argument below 1e-7 with 0 and 1)
    "finish_300": ((300, 3, 8, 8), (6, 6), "eigen", {}),
    "finish_bx33": ((8, 3, 184, 180), (8, 8), "eigen", {}),
    "chunk16": ((16, 3, 10, 12), (8, 8), "eigen", {}),
    "chunk17": ((17, 3, 10, 12), (8, 8), "eigen", {}),
    "chunk35": ((35, 3, 10, 12), (8, 8), "eigen", {}),
    "chunk_noise": ((18, 3, 10, 12), (8, 8), "noise", dict(only=(17,))),
    "clamped": ((2, 3, 10, 12), (10, 12), "spatial", dict(spatial=[dict(dx=0.45, dy=-0.45, zoom_x=0.4, zoom_y=0.4), dict(dx=-0.45, dy=0.45, zoom_x=0.4, zoom_y=0.4)])),
    "black": ((2, 3, 8, 8), (6, 6), "eigen", dict(scale=1e-3)),
}
# what each case is meant to select in the statistics pass: (vec4, bx, capped, finish_trips > 1, thread trips > 1)
STATS_EXPECT = {
    "stats_vec4": dict(vec4=True, bx=1, capped=False), "stats_odd": dict(vec4=False, bx=1), "stats_misaligned": dict(vec4=False, bx=1),
    "stats_bx": dict(vec4=True, bx=3, capped=False), "stats_cap3": dict(vec4=True, per_sample=3, bx=3, capped=True, trips=2),
    "stats_cap1": dict(vec4=False, per_sample=1, bx=1, capped=True, trips=8, rows=1024), "finish_300": dict(bx=1, rows=300, finish_trips=2),
    "finish_bx33": dict(vec4=True, bx=33, rows=264, finish_trips=2, capped=False),
}
STAT_CASES = [n for n, c in DATA_CASES.items() if c[1] is not None and c[2] in ("eigen", "eigen_angle", "all")]


def frozen(a):
    a.setflags(write=False)
    return a


def colour_image(rng, shape):
    """rng.random in [0, 1]; with three channels, pixels whose channels lie within 0.25 of each other are drawn again."""
    x = rng.random(shape).astype(np.float32)
    while shape[1] == 3:
        grey = (x.max(axis=1) - x.min(axis=1)) < 0.25
        if not grey.any():
            break
        x = np.where(grey[:, None], rng.random(shape).astype(np.float32), x)
    return x


def random_spatial(rng):
    sgn = lambda: 1.0 if rng.random() < 0.5 else -1.0
    return dict(mirror=float(rng.random() < 0.5), dx=sgn() * rng.uniform(0.01, 0.05), dy=sgn() * rng.uniform(0.01, 0.05),
                angle=sgn() * rng.uniform(0.02, 0.15), zoom_x=rng.uniform(1.02, 1.2), zoom_y=rng.uniform(1.02, 1.2))


@functools.lru_cache(maxsize=None)
def data_case(name):
    shape, crop, kind, opt = DATA_CASES[name]
    rng = np.random.default_rng(sorted(DATA_CASES).index(name) + 100 + 1000 * opt.get("seed", 0))
    N, Cc, H, W = shape
    img = frozen(colour_image(rng, shape) * np.float32(opt.get("scale", 1.0)))
    ch, cw = crop if crop else (0, 0)
    och, ocw = crop if crop else (H, W)
    only = opt.get("only", tuple(n for n in range(N) if n != 1))
    per = {n: dict(opt["spatial"][n] if "spatial" in opt else random_spatial(rng), **(KIND[kind] if n in only else {})) for n in range(N)}
    coeffs = frozen(B.coeff_array(N, per))
    mode = opt.get("mean", 0)
    mean = frozen(rng.random((Cc,) if mode == 1 else (Cc, och, ocw)).astype(np.float32)) if mode else None
    mats = frozen(np.stack([ops.augmentation_matrix(coeffs[n], cw, ch, W, H) for n in range(N)])) if crop else None
    return dict(name=name, img=img, coeffs=coeffs, mats=mats, ch=ch, cw=cw, mean=mean, mean_mode=mode, aligned=opt.get("aligned", True),
                eigvec=EIGVEC, seed=0x1234567887654321, stream=7, max_multiplier=1.5 if kind == "all" else 255.0)


@functools.lru_cache(maxsize=None)
def data_statement(name, who):
    """who = 'hip': d of mean_rgb from the launch plan; 'oracle': one sequential sum, d = N H W."""
    c = data_case(name)
    N, _, H, W = c["img"].shape
    d = B.mean_depth(B.stats_plan(N, H, W, c["aligned"])) if who == "hip" else N * H * W
    return B.data_aug_statement(c["img"], c["coeffs"], c["mats"], c["ch"], c["cw"], c["mean"], c["mean_mode"], c["max_multiplier"], c["eigvec"],
                                c["seed"], c["stream"], d_mean=d)


def oracle_data(c):
    return oracle.data_augmentation_forward(c["img"], c["coeffs"], c["ch"], c["cw"], mean=c["mean"], mean_mode=c["mean_mode"],
                                            max_multiplier=c["max_multiplier"], chromatic_eigvec=c["eigvec"], noise_seed=c["seed"], noise_stream=c["stream"])


def ratio_img(got, st):
    """Worst error / bound over the compared elements (NaN if anything is not finite) and the share of pixels left out."""
    err = np.abs(np.asarray(got, np.float64) - st["value"])
    keep = np.broadcast_to(~st["excluded"], err.shape)
    r = np.where(err == 0, 0.0, err / np.maximum(st["bound"], 1e-300))
    if not (np.isfinite(r[keep]).all() and np.isfinite(st["bound"][keep]).all()):
        return float("nan"), float(st["excluded"].mean())
    return float(r[keep].max()), float(st["excluded"].mean())


def check_img(what, got, st, cap=CAP):
    assert got.shape == st["value"].shape, what
    worst, share = ratio_img(got, st)
    print(f"{what}: worst err / bound {worst:.3f}, left out {share:.5f} of the pixels, largest bound {float(st['bound'].max()):.2e}")
    assert share <= cap, f"{what}: {share:.4f} of the pixels at a threshold"
    assert worst <= 1.0, f"{what}: error up to {worst:.3f} x its bound"


# ---------------------------------------------------------------------------------------------------------
# CPU: plans, caps, the statements against the C oracle, teeth
# ---------------------------------------------------------------------------------------------------------
def test_plan_matches_the_c_api():
    assert _lib.lib().fn2_data_augmentation_workspace_bytes(1) == _lib.lib().fn2_data_augmentation_workspace_bytes(1024) == B.workspace_bytes()
    assert 4 * B.RECORD_FLOATS <= B.PARTIAL_OFFSET
    for name in STAT_CASES:
        c = data_case(name)
        N, _, H, W = c["img"].shape
        plan = B.stats_plan(N, H, W, c["aligned"])
        assert plan["rows"] <= B.STAT_ROWS_MAX and B.PARTIAL_OFFSET + 48 * plan["rows"] <= B.workspace_bytes(), name
        for key, want in STATS_EXPECT.get(name, {}).items():
            assert plan[key] == want, (name, key, plan)
    assert B.stats_plan(2, 8, 8)["trips"] == 1 and B.stats_plan(2, 8, 8)["finish_trips"] == 1
    assert [len(B.chunks(n, B.ITEM_CHUNK)) for n in (16, 17, 35)] == [1, 2, 3] and B.chunks(35, B.ITEM_CHUNK)[-1] == (32, 3)
    assert [B.chunks(n, B.FLOW_CHUNK)[-1] for n in (65, 129)] == [(64, 1), (128, 1)]
    # the chunk of the noise case that holds the noisy sample takes <NOISE = true>, the other one <false>
    noisy = B.coeff_values(data_case("chunk_noise")["coeffs"])[:, B.F["noise"]] > 0
    assert [bool(noisy[n0:n0 + k].any()) for n0, k in B.chunks(18, B.ITEM_CHUNK)] == [False, True]


@pytest.mark.parametrize("name", list(DATA_CASES))
def test_cases_select_their_branch_and_stay_under_the_cap(name):
    c, st = data_case(name), data_statement(name, "hip")
    kind = DATA_CASES[name][2]
    share = float(st["excluded"].mean())
    print(f"{name}: flags {st['flags']}, left out {share:.5f}, pow log {st['pow_log']}")
    assert share <= CAP
    assert B.pow_log_in_range(st["pow_log"]), st["pow_log"]
    if c["ch"]:
        want = dict(spatial=(False, False, False), chromatic=(True, False, False), eigen=(False, True, False), eigen_angle=(False, True, False),
                    shadow=(False, False, True), noise=(False, False, True), all=(True, True, True))[kind]
        assert st["flags"] == want
        assert np.array_equal(B.coeff_values(c["coeffs"])[1, 6:], B.DEFAULT[6:]) or name == "clamped"      # sample 1: default colour coefficients
    if name == "clamped":
        n_pos = 2 * 10 * 12
        assert all(v >= n_pos // 6 for v in st["clamped"].values()) and st["clamped"]["x_low"] + st["clamped"]["x_high"] >= n_pos // 3, st["clamped"]
    if name == "black":
        assert st["es"]["big"] == [False] * 3 and not st["es"]["bigl"]
    elif st["es"] is not None:
        assert st["es"]["big"] == [True] * 3 and st["es"]["bigl"]


@pytest.mark.parametrize("name", list(DATA_CASES))
def test_oracle_data_augmentation_within_the_fp64_bound(name):
    # the cap on the pixels left out is asserted for the kernel's statement (test_cases_select_..., the GPU tests); with the oracle's
    # d = N H W the running error of s and l, and with it the share at a threshold, grows with the batch (see the module docstring)
    check_img(f"oracle {name}", oracle_data(data_case(name)), data_statement(name, "oracle"), cap=1.0)


def _mutated_data(name, mut):
    c = data_case(name)
    N, _, H, W = c["img"].shape
    return B.data_aug_statement(c["img"], c["coeffs"], c["mats"], c["ch"], c["cw"], c["mean"], c["mean_mode"], c["max_multiplier"], c["eigvec"],
                                c["seed"], c["stream"], d_mean=N * H * W, mut=mut)


@pytest.mark.parametrize("mut,name", [("swap_w", "spatial_c1"), ("no_001", "chromatic"), ("eigvec_not_transposed", "stats_vec4"),
                                      ("mean_nm1", "stats_vec4"), ("shadow_ge", "shadow"), ("mean_pp_as_pc", "all_mean_pixel")])
def test_teeth_data_augmentation(mut, name):
    got = oracle_data(data_case(name))
    assert ratio_img(got, data_statement(name, "oracle"))[0] <= 1.0
    worst, _ = ratio_img(got, _mutated_data(name, mut))
    print(f"{mut} on {name}: worst err / bound {worst:.3g}")
    assert worst > 1.0


# ---- FlowAugmentation ------------------------------------------------------------------------------------
# name: N, H, W, crop_h, crop_w, coefficients of image 1 per sample (None: random), offset of image 2's
FLOW_CASES = {
    "identity": (2, 9, 11, 9, 11, [{}, {}], {}),
    "ordinary": (3, 20, 24, 16, 20, None, dict(dx=0.01, angle=-0.02, zoom_x=1.03)),
    "chunk65": (65, 6, 8, 4, 6, None, dict(dy=0.02)),
    "chunk129": (129, 6, 8, 4, 6, None, dict(dx=-0.02)),
    "outside": (2, 10, 12, 10, 12, [dict(dx=-0.6, dy=-0.6, zoom_x=0.5, zoom_y=0.5), dict(dx=0.6, dy=0.6, zoom_x=0.5, zoom_y=0.5)], dict(angle=0.03)),
    "odd_mirror": (2, 9, 11, 7, 9, [dict(mirror=1.0, dx=0.04, angle=0.1, zoom_x=1.1), dict(mirror=1.0, dy=-0.03, angle=-0.08, zoom_y=1.15)], dict(dx=0.02)),
}


@functools.lru_cache(maxsize=None)
def flow_case(name):
    N, H, W, ch, cw, first, rel = FLOW_CASES[name]
    rng = np.random.default_rng(sorted(FLOW_CASES).index(name) + 300)
    flow = frozen((rng.standard_normal((N, 2, H, W)) * 8).astype(np.float32))
    first = first if first is not None else [random_spatial(rng) for _ in range(N)]
    c1 = frozen(B.coeff_array(N, dict(enumerate(first))))
    c2 = c1.copy()
    for f, v in rel.items():
        c2[:, B.F[f]] += np.float32(v if B.DEFAULT[B.F[f]] == 0 else np.log(v))
    c2 = frozen(c2)
    m1 = np.stack([ops.augmentation_matrix(c1[n], cw, ch, W, H) for n in range(N)])
    m2 = np.stack([ops.augmentation_matrix(c2[n], cw, ch, W, H, invert=True) for n in range(N)])
    cands, situations = B.flow_statement(flow, m1, m2, ch, cw)
    return dict(flow=flow, c1=c1, c2=c2, m1=m1, m2=m2, ch=ch, cw=cw, cands=cands, situations=situations)


def check_flow(what, got, cands):
    assert got.shape == cands[0][0].shape and np.isfinite(got).all(), what
    r = B.flow_ratio(got, cands)
    worst = float(r.max())
    print(f"{what}: worst err / bound {worst:.3f} ({len(cands)} tap candidates, largest bound {max(float(b.max()) for _, b in cands):.2e})")
    assert worst <= 1.0, f"{what}: error up to {worst:.3f} x its bound"


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_oracle_flow_augmentation_within_the_fp64_bound(name):
    c = flow_case(name)
    check_flow(f"oracle flow {name}", oracle.flow_augmentation_forward(c["flow"], c["c1"], c["c2"], c["ch"], c["cw"]), c["cands"])


def test_flow_cases_reach_their_situations():
    s = flow_case("outside")["situations"]
    print(s)
    assert all(v >= 5 for v in s.values()), s              # left, right, above, below, before the first sample, past the last one
    assert all(v == 0 for v in flow_case("identity")["situations"].values())
    assert flow_case("odd_mirror")["flow"].shape[3] % 2 == 1 and flow_case("odd_mirror")["c1"][:, 0].all() and flow_case("odd_mirror")["c2"][:, 0].all()
    assert np.abs(flow_case("identity")["cands"][0][0] - flow_case("identity")["flow"]).max() < 1e-12


@pytest.mark.parametrize("mut", ["floor", "clamped_index"])
def test_teeth_flow_augmentation(mut):
    c = flow_case("outside")
    got = oracle.flow_augmentation_forward(c["flow"], c["c1"], c["c2"], c["ch"], c["cw"])
    cands, _ = B.flow_statement(c["flow"], c["m1"], c["m2"], c["ch"], c["cw"], mut=mut)
    worst = float(B.flow_ratio(got, cands).max())
    print(f"{mut}: worst err / bound {worst:.3g}")
    assert float(B.flow_ratio(got, c["cands"]).max()) <= 1.0 and worst > 1.0


# ---------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------
PATTERN = 0xA5


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def dev_misaligned(a):
    """The blob on the GPU as a contiguous view that starts one float into its storage: 4-byte, not 16-byte aligned."""
    a = np.array(a, dtype=np.float32, order="C")
    t = torch.empty(a.size + 1, device="cuda", dtype=torch.float32)[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def hip_data(c, coeffs=None, eigvec=True, ws_bytes=None, crop=None, sentinel=None):
    """fn2_data_augmentation_forward with a workspace of the test's own -> (status, top, workspace bytes), all on the host."""
    img = c["img"]
    N, Cc, H, W = img.shape
    ch, cw = crop if crop else (c["ch"], c["cw"])
    och, ocw = (ch, cw) if ch else (H, W)
    p = ops.data_aug_params(cw, ch, c["max_multiplier"], c["eigvec"] if eigvec else None, c["mean_mode"], c["seed"], c["stream"])
    x = dev(img) if c["aligned"] else dev_misaligned(img)
    assert (x.data_ptr() % 16 == 0) == c["aligned"]
    co = np.ascontiguousarray(c["coeffs"] if coeffs is None else coeffs, np.float32)
    mean = dev(c["mean"]) if c["mean"] is not None else None
    nws = _lib.lib().fn2_data_augmentation_workspace_bytes(N) if ws_bytes is None else ws_bytes
    ws = torch.full((B.workspace_bytes(),), PATTERN, device="cuda", dtype=torch.uint8)
    top = torch.full((N, Cc, min(och, H), min(ocw, W)), float("nan") if sentinel is None else sentinel, device="cuda", dtype=torch.float32)
    rc = _lib.lib().fn2_data_augmentation_forward(C.byref(p), ops._ptr(x), C.c_void_p(co.ctypes.data), ops._ptr(mean), ops._ptr(top), N, Cc, H, W,
                                                  ops._ptr(ws), nws, ops._stream())
    torch.cuda.synchronize()
    return rc, top.cpu().numpy(), ws.cpu().numpy(), (x, ws, top)


def check_record(name, ws, st):
    """The EigenSpace record at the start of the workspace against the statement's statistics."""
    rec = ws[:4 * B.RECORD_FLOATS].view(np.float32)
    if st["es"] is None:
        assert (ws == PATTERN).all(), f"{name}: no chromatic-eigen coefficients, yet the workspace was written"
        return
    want, bound = B.es_record(st["es"])
    err = np.abs(rec[:16].astype(np.float64) - want)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    names = ["mean_eig"] * 3 + ["mean_rgb"] * 3 + ["max_abs_eig"] * 3 + ["max_rgb"] * 3 + ["min_rgb"] * 3 + ["max_l"]
    print(f"{name}: record worst err / bound " + ", ".join(f"{k} {max(r for r, q in zip(ratio, names) if q == k):.3f}" for k in dict.fromkeys(names)))
    assert np.array_equal(rec[9:15].view(np.uint32), np.concatenate([st["es"]["max_rgb"], st["es"]["min_rgb"]]).astype(np.float32).view(np.uint32))
    assert np.array_equal(rec[16:25].view(np.uint32), np.array(EIGVEC, np.float32).view(np.uint32))
    assert np.all(ratio <= 1.0), (name, dict(zip(names, ratio)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DATA_CASES))
def test_hip_data_augmentation_within_the_fp64_bound(name):
    c, st = data_case(name), data_statement(name, "hip")
    plan = B.stats_plan(c["img"].shape[0], c["img"].shape[2], c["img"].shape[3], c["aligned"])
    assert all(plan[key] == want for key, want in STATS_EXPECT.get(name, {}).items()), plan
    rc, top, ws, _ = hip_data(c)
    assert rc == 0, _lib.lib().fn2_last_error_string().decode()
    check_record(f"hip {name}", ws, st)
    check_img(f"hip {name}", top, st)
    if st["es"] is not None:
        # the statistics are held to their bounds above; from the RECORDED statistics (exact inputs) the pixel chain has to meet the bound
        # of its own roundings, which is not widened by the worst-case error of mean_rgb and max_abs_eig on every pixel
        rec = ws[:4 * B.RECORD_FLOATS].view(np.float32)
        check_img(f"hip {name} from the recorded statistics", top, B.data_aug_statement(
            c["img"], c["coeffs"], c["mats"], c["ch"], c["cw"], c["mean"], c["mean_mode"], c["max_multiplier"], c["eigvec"], c["seed"], c["stream"],
            d_mean=B.mean_depth(plan), record=rec))


@pytest.mark.gpu
def test_hip_second_run_in_other_allocations_gives_the_same_bits():
    c = data_case("stats_cap3")
    rc1, top1, ws1, keep = hip_data(c)                   # `keep` holds the first run's blobs, so the second run gets other addresses
    rc2, top2, ws2, keep2 = hip_data(c)
    assert rc1 == rc2 == 0 and all(a.data_ptr() != b.data_ptr() for a, b in zip(keep, keep2))
    assert np.array_equal(top1.view(np.uint32), top2.view(np.uint32))
    n = 4 * B.RECORD_FLOATS
    rows = B.stats_plan(300, 56, 56)["rows"]
    assert np.array_equal(ws1[:n], ws2[:n]) and np.array_equal(ws1[B.PARTIAL_OFFSET:B.PARTIAL_OFFSET + 48 * rows], ws2[B.PARTIAL_OFFSET:B.PARTIAL_OFFSET + 48 * rows])
    assert (ws1[B.PARTIAL_OFFSET + 48 * rows:] == PATTERN).all() and (ws1[n:B.PARTIAL_OFFSET] == PATTERN).all()      # nothing written beyond the plan's rows


@pytest.mark.gpu
def test_refusals_leave_top_and_workspace():
    inv, wsp = -1, -3                                      # FN2_ERR_INVALID_ARG, FN2_ERR_WORKSPACE (include/flownet2_hip.h)
    c3 = data_case("stats_vec4")
    c2 = dict(data_case("spatial_c2"))
    colour2 = B.coeff_array(2, {0: KIND["chromatic"]})
    eigen2 = B.coeff_array(2, {0: KIND["eigen"]})
    effect2 = B.coeff_array(2, {0: KIND["shadow"]})
    for what, want, kw, case in [("chromatic coefficients, C = 2", inv, dict(coeffs=colour2), c2), ("eigen coefficients, C = 2", inv, dict(coeffs=eigen2), c2),
                                 ("effect coefficients, C = 2", inv, dict(coeffs=effect2), c2), ("eigen without eigenvectors", inv, dict(eigvec=False), c3),
                                 ("workspace one byte short", wsp, dict(ws_bytes=B.workspace_bytes() - 1), c3),
                                 ("crop wider than the image", inv, dict(crop=(6, 9)), c3), ("crop higher than the image", inv, dict(crop=(9, 6)), c3)]:
        rc, top, ws, _ = hip_data(case, sentinel=7.25, **kw)
        assert rc == want, (what, rc)
        assert (top == np.float32(7.25)).all(), f"{what}: top was written"
        assert (ws == PATTERN).all(), f"{what}: the workspace was written"
    rc, top, ws, _ = hip_data(c3, sentinel=7.25)           # the same blobs are accepted with everything in place
    assert rc == 0 and not (top == np.float32(7.25)).any() and not (ws[:100] == PATTERN).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_hip_flow_augmentation_within_the_fp64_bound(name):
    c = flow_case(name)
    got = ops.flow_augmentation_forward(dev(c["flow"]), c["c1"], c["c2"], c["ch"], c["cw"]).cpu().numpy()
    check_flow(f"hip flow {name}", got, c["cands"])
