"""The runners' bidirectional flags end to end, each script in a fresh child process on randomly initialised FlowNetC weights (a temporary
.caffemodel.h5) and 64 x 64 crops of the FlyingChairs pair in tests/golden/chairs: scripts/run_flownet_many.py --bidirectional keeps
out.flo's bytes, writes the swapped line's flow as out.bw.flo, the occlusion planes as PGM and a JSON whose bytes do not depend on --batch;
scripts/run_flownet.py --backward / --occlusion writes the same files for one pair; scripts/eval_flownet.py --occ-from-consistency gets its
matched / unmatched split from the check.

A 64 x 64 image leaves FlowNetC a 1 x 1 map at conv6, and the Deconvolution{4, 2, 1} above it is a shape outside the net's kernel
families: by default it goes to the library, whose choice of algorithm is not a function of the call alone.  Every run here therefore
passes --general-conv own, which keeps that layer on the project's general-geometry kernels: the bytes are then a function of the pair."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from flownet2_amd import caffemodel, evaluate, flo, nets
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import CONSISTENCY_COL, COL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIRS = os.path.join(ROOT, "tests", "golden", "chairs")
CROPS = ((100, 200), (260, 40))                                                     # (y, x) of the two 64 x 64 crops


def _script(name):
    return [sys.executable, os.path.join(ROOT, "scripts", name)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every child process of this module, started together and waited for once."""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("fc_runner")
    layers = {}
    for k, v in nets.init_params("C", seed=3).items():
        layers.setdefault(k[:-2], []).append(v.numpy())
    weights = str(tmp / "c.caffemodel.h5")
    caffemodel.write_caffemodel_h5(weights, layers)
    imgs = [np.asarray(Image.open(os.path.join(CHAIRS, f"0000000-img{k}.png"))) for k in (0, 1)]
    gt = np.load(os.path.join(CHAIRS, "0000000-gt.npz"))["flow"]
    gt = gt if gt.shape[0] == 2 else gt.transpose(2, 0, 1)
    pairs = []
    for j, (y, x) in enumerate(CROPS):
        names = [str(tmp / f"p{j}_img{k}.png") for k in (0, 1)]
        for k in (0, 1):
            Image.fromarray(imgs[k][y:y + 64, x:x + 64]).save(names[k])
        np.savez(str(tmp / f"p{j}_gt.npz"), flow=np.ascontiguousarray(gt[:, y:y + 64, x:x + 64]))
        pairs.append(names)
    dirs = {}
    for tag in ("plain", "bi2", "bi1", "swapped", "single"):
        dirs[tag] = tmp / tag
        dirs[tag].mkdir()
    lists = {}
    for tag in ("plain", "bi2", "bi1", "swapped"):
        lists[tag] = str(tmp / f"{tag}.txt")
        with open(lists[tag], "w") as f:
            for j, (a, b) in enumerate(pairs):
                a, b = (b, a) if tag == "swapped" else (a, b)
                f.write(f"{a} {b} {dirs[tag] / ('out%d.flo' % j)}\n")
    lists["eval"] = str(tmp / "eval.txt")
    with open(lists["eval"], "w") as f:
        for j, (a, b) in enumerate(pairs):
            f.write(f"{a} {b} {tmp / ('p%d_gt.npz' % j)}\n")
    net = ["--net", "C", "--weights", weights, "--general-conv", "own"]
    many = _script("run_flownet_many.py") + net
    cmds = {
        "plain": many + ["--batch", "2", lists["plain"]],
        "bi2": many + ["--batch", "2", "--bidirectional", "--consistency-json", str(dirs["bi2"] / "c.json"), lists["bi2"]],
        "bi1": many + ["--batch", "1", "--bidirectional", "--consistency-json", str(dirs["bi1"] / "c.json"), lists["bi1"]],
        "swapped": many + ["--batch", "2", lists["swapped"]],
        "single": _script("run_flownet.py") + net + [pairs[0][0], pairs[0][1], str(dirs["single"] / "out.flo"),
                                               "--backward", str(dirs["single"] / "out.bw.flo"), "--occlusion", str(dirs["single"] / "out.occ.pgm")],
        "eval": _script("eval_flownet.py") + net + ["--occ-from-consistency", "--json", str(tmp / "eval.json"),
                                             lists["eval"]],
        "eval_plain": _script("eval_flownet.py") + net + ["--json", str(tmp / "eval_plain.json"), lists["eval"]],
    }
    procs = {tag: subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for tag, cmd in cmds.items()}
    for tag, p in procs.items():
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f"{tag}: exit status {p.returncode}\n{out.decode()[-3000:]}"
    return {"tmp": tmp, "dirs": dirs}


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_forward_flow_keeps_its_bytes(runs):
    d = runs["dirs"]
    for j in (0, 1):
        plain = _read(d["plain"] / f"out{j}.flo")
        assert len(plain) == 12 + 64 * 64 * 8
        assert _read(d["bi2"] / f"out{j}.flo") == plain and _read(d["bi1"] / f"out{j}.flo") == plain
    assert _read(d["single"] / "out.flo") == _read(d["plain"] / "out0.flo")
    assert sorted(os.listdir(d["plain"])) == ["out0.flo", "out1.flo"]                # no flag, no further file
    assert sorted(os.listdir(d["bi2"])) == sorted(["c.json"] + [f"out{j}{s}" for j in (0, 1) for s in (".flo", ".bw.flo", ".occ.pgm", ".bw.occ.pgm")])


def test_backward_flow_is_the_plain_run_on_the_swapped_line(runs):
    d = runs["dirs"]
    for j in (0, 1):
        swapped = _read(d["swapped"] / f"out{j}.flo")
        assert _read(d["bi2"] / f"out{j}.bw.flo") == swapped and _read(d["bi1"] / f"out{j}.bw.flo") == swapped
        assert swapped != _read(d["plain"] / f"out{j}.flo")
    assert _read(d["single"] / "out.bw.flo") == _read(d["swapped"] / "out0.flo")


def test_pgm_is_the_occ_plane_of_the_written_flows(runs):
    d = runs["dirs"]
    for j in (0, 1):
        fw = torch.from_numpy(flo.read_flo(str(d["bi2"] / f"out{j}.flo")).transpose(2, 0, 1)[np.newaxis].copy()).cuda()
        bw = torch.from_numpy(flo.read_flo(str(d["bi2"] / f"out{j}.bw.flo")).transpose(2, 0, 1)[np.newaxis].copy()).cuda()
        c = Fn.flow_consistency(fw, bw)
        for name, occ in ((f"out{j}.occ.pgm", c.occ_fw), (f"out{j}.bw.occ.pgm", c.occ_bw)):
            want = b"P5\n64 64\n255\n" + (occ[0, 0].cpu().numpy() * 255).astype(np.uint8).tobytes()
            assert _read(d["bi2"] / name) == want and _read(d["bi1"] / name) == want
            if j == 0 and name.endswith("0.occ.pgm"):
                assert _read(d["single"] / "out.occ.pgm") == want
        doc = json.loads(_read(d["bi2"] / "c.json"))
        assert doc["rows_fw"][j] == c.rows_fw[0].tolist() and doc["rows_bw"][j] == c.rows_bw[0].tolist()


def test_consistency_json_does_not_depend_on_the_batch(runs):
    d = runs["dirs"]
    text = _read(d["bi2"] / "c.json")
    assert text == _read(d["bi1"] / "c.json")

    def refuse(token):
        raise AssertionError(f"{token} is not JSON")
    doc = json.loads(text, parse_constant=refuse)
    assert len(doc["lines"]) == 2 and doc["summary"]["samples"] == 2 and doc["summary"]["alpha"] == [0.01, 0.5]
    assert doc["summary"]["fw"]["pixels"] == 2 * 64 * 64 and doc["lines"][0]["fw"]["pixels"] == 64 * 64
    assert doc["columns"] == list(evaluate.CONSISTENCY_COLUMNS)


def test_evaluator_takes_its_occlusion_plane_from_the_check(runs):
    doc = json.loads(_read(runs["tmp"] / "eval.json"))
    plain = json.loads(_read(runs["tmp"] / "eval_plain.json"))
    assert doc["occ_source"] == "consistency" and doc["alpha"] == [0.01, 0.5] and "occ_source" not in plain
    cons = json.loads(_read(runs["dirs"]["bi2"] / "c.json"))
    rows, prows = np.array(doc["rows"]), np.array(plain["rows"])
    assert np.array_equal(rows[:, COL["OCC_COUNT"]], np.array(cons["rows_fw"])[:, CONSISTENCY_COL["OCCLUDED"]]) and rows[:, COL["OCC_COUNT"]].sum() > 0
    assert not prows[:, COL["OCC_COUNT"]].any() and plain["summary"]["epe_unmatched"] is None and doc["summary"]["epe_unmatched"] is not None
    keep = [i for i in range(rows.shape[1]) if i not in (COL["OCC_COUNT"], COL["OCC_EPE_SUM"])]
    assert np.array_equal(rows[:, keep], prows[:, keep])                             # the prediction and every other column: unchanged
