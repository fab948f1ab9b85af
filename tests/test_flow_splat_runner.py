"""scripts/interpolate_flownet.py end to end, each run in a fresh child process on randomly initialised FlowNetC weights (a temporary
.caffemodel.h5) and four 64 x 64 crops of one FlyingChairs image in tests/golden/chairs, each shifted by (1, 2) pixels against the one
before: the files it writes, and the same bytes for --batch 1 and --batch 3; and scripts/train_pipeline.py --unsupervised --unsup-occ
range, two steps with a finite loss.

Every interpolation run passes --general-conv own, for the reason given in test_flow_consistency_runner.py."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from flownet2_amd import caffemodel, nets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIRS = os.path.join(ROOT, "tests", "golden", "chairs")
ORIGIN, SHIFT, FRAMES = (100, 200), (1, 2), 4
SMALL = ["--batch", "2", "--iters", "2", "--height", "160", "--width", "224", "--crop-height", "128", "--crop-width", "192", "--no-prefetch"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every child process of this module, started together and waited for once."""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("fs_runner")
    layers = {}
    for k, v in nets.init_params("C", seed=3).items():
        layers.setdefault(k[:-2], []).append(v.numpy())
    weights = str(tmp / "c.caffemodel.h5")
    caffemodel.write_caffemodel_h5(weights, layers)
    img = np.asarray(Image.open(os.path.join(CHAIRS, "0000000-img0.png")))
    names = []
    for k in range(FRAMES):
        y, x = ORIGIN[0] + k * SHIFT[0], ORIGIN[1] + k * SHIFT[1]
        names.append(str(tmp / f"frame{k}.png"))
        Image.fromarray(img[y:y + 64, x:x + 64]).save(names[-1])
    frames = str(tmp / "frames.txt")
    with open(frames, "w") as f:
        f.write("\n".join(names) + "\n")
    interp = [sys.executable, os.path.join(ROOT, "scripts", "interpolate_flownet.py"), "--net", "C", "--weights", weights, "--general-conv", "own"]
    cmds = {
        "b1": interp + ["--batch", "1", "--factor", "4", frames, str(tmp / "b1")],
        "b3": interp + ["--batch", "3", "--factor", "4", frames, str(tmp / "b3")],
        "mid": interp + ["--batch", "2", frames, str(tmp / "mid")],
        "train": [sys.executable, os.path.join(ROOT, "scripts", "train_pipeline.py"), *SMALL, "--unsupervised", "--unsup-occ", "range"],
    }
    procs = {tag: subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for tag, cmd in cmds.items()}
    out = {}
    for tag, p in procs.items():
        text, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f"{tag}: exit status {p.returncode}\n{text.decode()[-3000:]}"
        out[tag] = text.decode()
    return {"tmp": tmp, "out": out}


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_the_files_and_their_bytes_do_not_depend_on_the_batch(runs):
    from PIL import Image
    tmp = runs["tmp"]
    want = sorted("frame%05d_t%.3f.png" % (k, t) for k in range(FRAMES - 1) for t in (0.25, 0.5, 0.75))
    assert sorted(os.listdir(tmp / "b1")) == want and sorted(os.listdir(tmp / "b3")) == want
    for name in want:
        assert _read(tmp / "b1" / name) == _read(tmp / "b3" / name), name
    assert sorted(os.listdir(tmp / "mid")) == ["frame%05d_t0.500.png" % k for k in range(FRAMES - 1)]
    for k in range(FRAMES - 1):
        assert _read(tmp / "mid" / ("frame%05d_t0.500.png" % k)) == _read(tmp / "b1" / ("frame%05d_t0.500.png" % k))
        a = np.asarray(Image.open(tmp / "mid" / ("frame%05d_t0.500.png" % k)))
        assert a.shape == (64, 64, 3) and a.dtype == np.uint8 and a.std() > 1          # a picture, not a constant
    assert "wrote 9 frames" in runs["out"]["b1"] and "wrote 3 frames" in runs["out"]["mid"]


def test_unsupervised_training_with_range_map_occlusion(runs):
    m = re.search(r"^unsupervised loss ([0-9.eE+-]+|nan|inf) \(smooth weight ([0-9.g]+), order (\d), occlusion masks (\w+)\), "
                  r"EPE against the ground truth ([0-9.eE+-]+|nan|inf)$", runs["out"]["train"], flags=re.M)
    assert m, runs["out"]["train"]
    loss, epe = float(m.group(1)), float(m.group(5))
    assert math.isfinite(loss) and loss > 0 and math.isfinite(epe) and epe > 0 and m.group(4) == "range"
