"""The Python layers over the census-loss kernels: functional.census_loss under torch.autograd against the raw calls, the data_term switch
of functional.unsupervised_loss and nets.unsupervised_loss (and the untouched default against the pinned bits of tests/golden/
stream_bits.json), census_loss_report, descent on the device, and scripts/train_pipeline.py --unsup-data census."""
import hashlib
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import census_loss_ref as R
import test_census_loss as T
import unsup_loss_ref as UR
from flownet2_amd import functional as Fn
from flownet2_amd import nets
from flownet2_amd.evaluate import CENSUS_LOSS_COL as COL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_same = T._same


def _tensors(case):
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in case.items()}


def test_functional_fills_the_gradients_with_the_kernels_arrays():
    case = T._case("1x3x37x70", "small")
    p = R.params(radius=2, data_weight=0.5)
    kw = dict(radius=2, data_weight=0.5)
    raw = T.run(case, p, total_diff=1.0)
    t = _tensors(case)
    fw, bw = t["fw"].requires_grad_(True), t["bw"].requires_grad_(True)
    loss = Fn.census_loss(t["img0"], t["img1"], fw, bw, t["occ_fw"], t["occ_bw"], **kw)
    assert loss.dim() == 0 and loss.is_cuda and _same(loss.detach().cpu().numpy(), raw["loss"])
    loss.backward()
    assert _same(fw.grad.cpu().numpy(), raw["diff"][0]) and _same(bw.grad.cpu().numpy(), raw["diff"][1])
    fw.grad = bw.grad = None
    (3.0 * Fn.census_loss(t["img0"], t["img1"], fw, bw, t["occ_fw"], t["occ_bw"], **kw)).backward()      # the upstream gradient, on the device
    scaled = T.run(case, p, total_diff=3.0)
    assert _same(fw.grad.cpu().numpy(), scaled["diff"][0]) and _same(bw.grad.cpu().numpy(), scaled["diff"][1])
    one = Fn.census_loss(t["img0"], t["img1"], fw.detach().requires_grad_(True), None, t["occ_fw"], **kw)
    assert _same(one.detach().cpu().numpy(), T.run(case, p, two=False, grad=False)["loss"])
    bw.grad = None
    Fn.census_loss(t["img0"], t["img1"], fw.detach(), bw, **kw).backward()          # the backward flow alone asks for a gradient
    assert bw.grad is not None and bool(bw.grad.abs().sum() > 0)
    with pytest.raises(RuntimeError, match="gets no gradient"):
        Fn.census_loss(t["img0"].clone().requires_grad_(True), t["img1"], fw)
    with pytest.raises(ValueError, match="must be"):
        Fn.census_loss(t["img0"], t["img1"], fw[:, :, :-1])
    with pytest.raises(Exception, match="radius"):
        Fn.census_loss(t["img0"], t["img1"], fw, radius=4)

    rep = Fn.census_loss_report(t["img0"], t["img1"], fw, bw, t["occ_fw"], t["occ_bw"], **kw)
    assert len(rep) == 1 and _same(rep.rows_fw, raw["rows"][0, :-1]) and _same(rep.rows_bw, raw["rows"][1, :-1]) and rep.loss == float(raw["loss"])
    s, tot = rep.summary(), raw["rows"][:, -1]
    for d, key in enumerate(("fw", "bw")):
        assert s[key]["data_mean"] == tot[d, COL["DATA_SUM"]] / tot[d, COL["COUNTED"]]
        assert s[key]["dist_mean"] == tot[d, COL["DIST_SUM"]] / tot[d, COL["COUNTED"]]
        assert s[key]["pairs_mean"] == tot[d, COL["PAIRS"]] / tot[d, COL["COUNTED"]] <= 24
        for share, col in (("counted", "COUNTED"), ("occluded", "OCCLUDED"), ("outside", "OUTSIDE"), ("nonfinite", "NONFINITE")):
            assert s[key][share] == tot[d, COL[col]] / tot[d, COL["PIXELS"]]
    assert 0 < s["fw"]["occluded"] < 0.5 and s["samples"] == 1 and s["loss"] == rep.loss and s["radius"] == 2


def test_the_census_data_term_is_census_loss_plus_the_smoothness_call():
    case = T._case("2x3x16x64", "small")
    t = _tensors(case)
    six = lambda fw, bw: (t["img0"], t["img1"], fw, bw, t["occ_fw"], t["occ_bw"])
    kw = dict(data_weight=0.75, smooth_weight=0.5, smooth_order=1, flow_mult=1.25)
    census = dict(radius=2, census_eps=(0.5, 0.2), intensity_scale=100.0)
    grads = []
    for composed in (False, True):
        fw, bw = t["fw"].clone().requires_grad_(True), t["bw"].clone().requires_grad_(True)
        if composed:
            loss = Fn.census_loss(*six(fw, bw), data_weight=0.75, flow_mult=1.25, **census) + \
                Fn.unsupervised_loss(*six(fw, bw), **dict(kw, data_weight=0.0))
        else:
            loss = Fn.unsupervised_loss(*six(fw, bw), data_term="census", census=census, **kw)
        loss.backward()
        grads.append((loss.detach().cpu().numpy(), fw.grad.cpu().numpy(), bw.grad.cpu().numpy()))
    assert all(_same(a, b) for a, b in zip(*grads)) and np.abs(grads[0][1]).max() > 0
    rep = Fn.unsupervised_loss_report(*six(t["fw"], t["bw"]), data_term="census", census=census, **kw)
    only = Fn.census_loss_report(*six(t["fw"], t["bw"]), data_weight=0.75, flow_mult=1.25, **census)
    assert rep.census is not None and _same(rep.census.rows_fw, only.rows_fw) and rep.data_weight == 0.0
    assert rep.loss == pytest.approx(float(grads[0][0]), rel=1e-6) and rep.summary()["census"]["radius"] == 2


def test_the_default_data_term_keeps_the_pinned_bits():
    """unsupervised_loss() without the new keywords on a case of tests/test_unsup_loss.py, against the hashes tests/test_stream_bits.py pins
    for the raw calls (defaults, both directions, total_diff 0.75)."""
    import test_unsup_loss as ul
    with open(os.path.join(ROOT, "tests", "golden", "stream_bits.json")) as f:
        want = json.load(f)["sha256"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    t = _tensors(ul._case("2x3x36x60", "small"))
    for explicit in ({}, dict(data_term="brightness")):
        fw, bw = t["fw"].clone().requires_grad_(True), t["bw"].clone().requires_grad_(True)
        loss = Fn.unsupervised_loss(t["img0"], t["img1"], fw, bw, t["occ_fw"], t["occ_bw"], **explicit)
        (0.75 * loss).backward()
        key = "unsup_loss/2x3x36x60/small/general/order2/two/"
        assert sha(loss.detach().cpu().numpy().reshape(1)[0]) == want[key + "loss"]
        assert sha(fw.grad.cpu().numpy()) == want[key + "diff0"] and sha(bw.grad.cpu().numpy()) == want[key + "diff1"]


def test_nets_unsupervised_loss_passes_the_data_term_to_every_scale():
    N, H, W = 2, 32, 64
    img0, img1 = (torch.from_numpy(t).cuda() for t in UR.make_images((N, 3, H, W), 5))
    rng = np.random.default_rng(9)
    sizes = {3: (8, 16), 2: (16, 32)}                                               # scale -> (h, w); LOSS_WEIGHTS lists scale 3 before scale 2
    flows_fw = {s: torch.from_numpy(rng.normal(0, 0.02, (N, 2, h, w)).astype(F)).cuda().requires_grad_(True) for s, (h, w) in sizes.items()}
    flows_bw = {s: torch.from_numpy(rng.normal(0, 0.02, (N, 2, h, w)).astype(F)).cuda().requires_grad_(True) for s, (h, w) in sizes.items()}
    assert nets.backend_of(Fn).has_census_loss
    census = dict(radius=2)
    total = nets.unsupervised_loss(flows_fw, flows_bw, img0, img1, Fn, smooth_order=1, data_term="census", census=census)
    want = None
    for s in (3, 2):
        (h, w), f, b, lw = sizes[s], flows_fw[s], flows_bw[s], nets.LOSS_WEIGHTS[s]
        mult = nets.FLOW_SCALE * w / W
        i0, i1 = Fn.downsample(img0, h, w), Fn.downsample(img1, h, w)
        c = Fn.flow_consistency(f.detach() * mult, b.detach() * mult)
        term = (Fn.census_loss(i0, i1, f, b, c.occ_fw, c.occ_bw, flow_mult=mult, **census) +
                Fn.unsupervised_loss(i0, i1, f, b, c.occ_fw, c.occ_bw, data_weight=0.0, smooth_order=1, flow_mult=mult)) * lw
        want = term if want is None else want + term
    assert total.dim() == 0 and _same(total.detach().cpu().numpy(), want.detach().cpu().numpy())
    brightness = nets.unsupervised_loss(flows_fw, flows_bw, img0, img1, Fn, smooth_order=1)
    assert float(brightness.detach()) != float(total.detach())
    total.backward()
    assert all(f.grad is not None and bool(f.grad.abs().sum() > 0) for f in list(flows_fw.values()) + list(flows_bw.values()))


def test_descent_on_a_translated_image_with_a_brightness_offset():
    """The descent of tests/test_census_loss_host.py on the device (census_loss_ref.DESCENT: the image, the step size and the float64
    restatement's figures, loss 6.510285 -> 3.001585 and EPE 2.0 -> 1.540722): the kernel must lower both too.  Observed on an MI355X:
    loss 6.510285 -> 3.243133, EPE 2.0 -> 1.557716."""
    img0, img1 = R.descent_images()
    i0, i1 = torch.from_numpy(img0).cuda(), torch.from_numpy(img1).cuda()
    fw = torch.zeros((1, 2, 16, 32), device="cuda", requires_grad=True)
    p = R.params()

    def measure():
        rep = Fn.census_loss_report(i0, i1, fw.detach())
        epe, counted = R.descent_epe(fw.detach().cpu().numpy(), p)
        assert counted == rep.rows_fw[0, COL["COUNTED"]]
        return rep.loss, epe

    before = measure()
    for _ in range(R.DESCENT["steps"]):
        fw.grad = None
        Fn.census_loss(i0, i1, fw).backward()
        with torch.no_grad():
            fw -= R.DESCENT["step"] * fw.grad
    after = measure()
    print(f"descent: loss {before[0]:.6f} -> {after[0]:.6f}, EPE {before[1]:.6f} -> {after[1]:.6f}")
    assert before[1] == 2.0 and after[0] < before[0] and after[1] < before[1]


def test_the_training_script_trains_on_the_census_term():
    """Two steps on the records and at the sizes of tests/test_unsup_loss_runner.py, as a fresh child process."""
    small = ["--batch", "2", "--iters", "2", "--height", "160", "--width", "224", "--crop-height", "128", "--crop-width", "192", "--no-prefetch"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_pipeline.py"), *small, "--unsupervised", "--unsup-data", "census",
                        "--census-radius", "2"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^unsupervised loss ([0-9.eE+-]+|nan|inf) \(census data term of radius 2, smooth weight 1, order 2, occlusion masks on\), "
                  r"EPE against the ground truth ([0-9.eE+-]+|nan|inf)$", r.stdout, flags=re.M)
    assert m, r.stdout
    loss, epe = float(m.group(1)), float(m.group(2))
    assert math.isfinite(loss) and loss > 0 and math.isfinite(epe) and epe > 0
