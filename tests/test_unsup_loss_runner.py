"""scripts/train_pipeline.py --unsupervised: two FlowNetC passes (img0, img1) and (img1, img0), nets.unsupervised_loss on the two pyramids,
backward and the optimizer step, at 128 x 192 -- the crop smoke() trains FlowNetC at, the smallest the suite runs the training graph on --
and the stage table of the run without the flag."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--batch", "2", "--iters", "2", "--height", "160", "--width", "224", "--crop-height", "128", "--crop-width", "192", "--no-prefetch"]
STAGES = ["decode", "scale", "draw0 (host)", "augment0", "draw1 (host)", "augment1", "flow_aug", "train step"]


def _run(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_pipeline.py"), *SMALL, *flags], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _table(out):
    return [m.group(1) for m in re.finditer(r"^\| (.+?) \| [0-9.]+ \|$", out, flags=re.M)]


def test_unsupervised_training_prints_a_finite_loss_and_an_epe():
    out = _run("--unsupervised")
    m = re.search(r"^unsupervised loss ([0-9.eE+-]+|nan|inf) \(smooth weight ([0-9.g]+), order (\d), occlusion masks (on|off)\), "
                  r"EPE against the ground truth ([0-9.eE+-]+|nan|inf)$", out, flags=re.M)
    assert m, out
    loss, epe = float(m.group(1)), float(m.group(5))
    assert math.isfinite(loss) and loss > 0 and math.isfinite(epe) and epe > 0
    assert (m.group(2), m.group(3), m.group(4)) == ("1", "2", "on")
    assert _table(out) == STAGES and "NaN ground truth kept" not in out


def test_without_the_flag_the_output_is_the_supervised_one():
    out = _run()
    assert _table(out) == STAGES
    assert re.search(r"^loss [0-9.]+, NaN ground truth kept: True$", out, flags=re.M) and "unsupervised" not in out
