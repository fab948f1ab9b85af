"""The runners' picture flags end to end, each script in a fresh child process on randomly initialised FlowNetC weights (a temporary
.caffemodel.h5) and 64 x 64 crops of the FlyingChairs pair in tests/golden/chairs, as in test_flow_consistency_runner.py (whose reason
for --general-conv own holds here too): scripts/run_flownet.py --color writes the colour coding of the very flow it writes and keeps
out.flo's bytes; scripts/run_flownet_many.py --color writes the same PNG bytes at --batch 1 and --batch 2, and out.bw.png with
--bidirectional; scripts/eval_flownet.py --error-maps / --color-maps writes one picture per list line and keeps the JSON's bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from flownet2_amd import caffemodel, flo, nets, visualize
from flownet2_amd import functional as Fn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIRS = os.path.join(ROOT, "tests", "golden", "chairs")
CROPS = ((100, 200), (260, 40))                                                     # (y, x) of the two 64 x 64 crops
COLOR_MAX = 0.5


def _script(name):
    return [sys.executable, os.path.join(ROOT, "scripts", name)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every child process of this module, started together and waited for once."""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("fv_runner")
    layers = {}
    for k, v in nets.init_params("C", seed=3).items():
        layers.setdefault(k[:-2], []).append(v.numpy())
    weights = str(tmp / "c.caffemodel.h5")
    caffemodel.write_caffemodel_h5(weights, layers)
    imgs = [np.asarray(Image.open(os.path.join(CHAIRS, f"0000000-img{k}.png"))) for k in (0, 1)]
    gt = np.load(os.path.join(CHAIRS, "0000000-gt.npz"))["flow"]
    gt = gt if gt.shape[0] == 2 else gt.transpose(2, 0, 1)
    pairs, gts = [], []
    for j, (y, x) in enumerate(CROPS):
        names = [str(tmp / f"p{j}_img{k}.png") for k in (0, 1)]
        for k in (0, 1):
            Image.fromarray(imgs[k][y:y + 64, x:x + 64]).save(names[k])
        gts.append(np.ascontiguousarray(gt[:, y:y + 64, x:x + 64], np.float32))
        np.savez(str(tmp / f"p{j}_gt.npz"), flow=gts[-1])
        pairs.append(names)
    dirs = {}
    for tag in ("plain", "single", "fixed", "many1", "many2", "err", "col"):
        dirs[tag] = tmp / tag
        dirs[tag].mkdir()
    lists = {}
    for tag in ("plain", "many1", "many2"):
        lists[tag] = str(tmp / f"{tag}.txt")
        with open(lists[tag], "w") as f:
            for j, (a, b) in enumerate(pairs):
                f.write(f"{a} {b} {dirs[tag] / ('out%d.flo' % j)}\n")
    lists["eval"] = str(tmp / "eval.txt")
    with open(lists["eval"], "w") as f:
        for j, (a, b) in enumerate(pairs):
            f.write(f"{a} {b} {tmp / ('p%d_gt.npz' % j)}\n")
    net = ["--net", "C", "--weights", weights, "--general-conv", "own"]
    many, one = _script("run_flownet_many.py") + net, _script("run_flownet.py") + net + [pairs[0][0], pairs[0][1]]
    cmds = {
        "plain": many + ["--batch", "2", lists["plain"]],
        "many2": many + ["--batch", "2", "--color", "--bidirectional", lists["many2"]],
        "many1": many + ["--batch", "1", "--color", lists["many1"]],
        "single": one + [str(dirs["single"] / "out.flo"), "--color", str(dirs["single"] / "out.png")],
        "fixed": one + [str(dirs["fixed"] / "out.flo"), "--color", str(dirs["fixed"] / "out.png"), "--color-max", str(COLOR_MAX)],
        "eval": _script("eval_flownet.py") + net + ["--json", str(tmp / "eval.json"), "--error-maps", str(dirs["err"]), "--color-maps",
                                             str(dirs["col"]), lists["eval"]],
        "eval_plain": _script("eval_flownet.py") + net + ["--json", str(tmp / "eval_plain.json"), lists["eval"]],
    }
    procs = {tag: subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for tag, cmd in cmds.items()}
    for tag, p in procs.items():
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f"{tag}: exit status {p.returncode}\n{out.decode()[-3000:]}"
    return {"tmp": tmp, "dirs": dirs, "gts": gts}


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _flow(path):
    return torch.from_numpy(flo.read_flo(str(path)).transpose(2, 0, 1)[np.newaxis].copy()).cuda()


def test_the_single_runner_writes_the_colour_coding_of_its_flow(runs):
    d = runs["dirs"]
    plain = _read(d["plain"] / "out0.flo")
    assert len(plain) == 12 + 64 * 64 * 8
    assert _read(d["single"] / "out.flo") == plain and _read(d["fixed"] / "out.flo") == plain      # the flag changes no byte of the flow
    assert sorted(os.listdir(d["single"])) == ["out.flo", "out.png"] and sorted(os.listdir(d["plain"])) == ["out0.flo", "out1.flo"]
    flow = _flow(d["single"] / "out.flo")
    png = visualize.read_png8(str(d["single"] / "out.png"))
    assert png.shape == (64, 64, 3) and np.array_equal(png, Fn.flow_to_color(flow)[0].cpu().numpy())
    assert len(np.unique(png.reshape(-1, 3), axis=0)) > 16                          # a picture, not a flat field
    fixed = visualize.read_png8(str(d["fixed"] / "out.png"))
    assert np.array_equal(fixed, Fn.flow_to_color(flow, max_flow=COLOR_MAX)[0].cpu().numpy()) and not np.array_equal(fixed, png)


def test_a_pairs_picture_does_not_depend_on_the_batch(runs):
    d = runs["dirs"]
    for j in (0, 1):
        assert _read(d["many2"] / f"out{j}.flo") == _read(d["plain"] / f"out{j}.flo") == _read(d["many1"] / f"out{j}.flo")
        png = _read(d["many2"] / f"out{j}.png")
        assert png == _read(d["many1"] / f"out{j}.png") and png[:8] == b"\x89PNG\r\n\x1a\n"
        assert np.array_equal(visualize.read_png8(str(d["many2"] / f"out{j}.png")), Fn.flow_to_color(_flow(d["many2"] / f"out{j}.flo"))[0].cpu().numpy())
        bw = visualize.read_png8(str(d["many2"] / f"out{j}.bw.png"))
        assert np.array_equal(bw, Fn.flow_to_color(_flow(d["many2"] / f"out{j}.bw.flo"))[0].cpu().numpy())
    assert _read(d["many2"] / "out0.png") == _read(d["single"] / "out.png")         # and not on the script
    assert sorted(os.listdir(d["many1"])) == ["out0.flo", "out0.png", "out1.flo", "out1.png"]


def test_the_evaluator_writes_one_picture_per_list_line(runs):
    d = runs["dirs"]
    assert _read(runs["tmp"] / "eval.json") == _read(runs["tmp"] / "eval_plain.json")      # the pictures change no byte of the numbers
    assert sorted(os.listdir(d["err"])) == ["000000.png", "000001.png"] == sorted(os.listdir(d["col"]))
    for j in (0, 1):
        pred = _flow(d["plain"] / f"out{j}.flo")                                    # the runner's prediction is the evaluator's
        gt = torch.from_numpy(runs["gts"][j][np.newaxis]).cuda()
        err = visualize.read_png8(str(d["err"] / f"{j:06d}.png"))
        assert np.array_equal(err, Fn.flow_error_map(pred, gt)[0].cpu().numpy()) and len(np.unique(err.reshape(-1, 3), axis=0)) > 1
        assert np.array_equal(visualize.read_png8(str(d["col"] / f"{j:06d}.png")), Fn.flow_to_color(pred)[0].cpu().numpy())
