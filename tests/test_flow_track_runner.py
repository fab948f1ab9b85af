"""scripts/track_flownet.py end to end, each run in a fresh child process on randomly initialised FlowNetC weights (a temporary
.caffemodel.h5) and four 64 x 64 crops of one FlyingChairs image in tests/golden/chairs, each shifted by (1, 2) pixels against the one
before: tracks.npz and the --long-range flow have the same bytes for --window 1 and --window 3; the long-range flow is
FlowTracks.long_range_flow() of the per-pair flows that scripts/run_flownet_many.py --bidirectional writes; and those keep the bytes
of a plain run.

The weights are untrained, so the forward and the backward flow of a pair do not cancel and the consistency test with the published
alpha stops every point in its first frame (measured: 50 % INCONSISTENT, 48 % MARKED, 2 % OUTSIDE, no step taken).  The tracker runs
therefore pass --alpha 1e9 1e9, which leaves the motion-boundary marks and the image border to stop points: about a third of the pixels
of frame 0 then reach the last frame.

Every run passes --general-conv own, for the reason given in test_flow_consistency_runner.py: on 64-pixel-high images one Deconvolution
of FlowNetC would otherwise go to the library, whose bits are not a function of the call alone."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from flownet2_amd import caffemodel, evaluate, flo, nets, visualize
from flownet2_amd import functional as Fn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIRS = os.path.join(ROOT, "tests", "golden", "chairs")
ALPHA = (1e9, 1e9)                                                                 # see above
ORIGIN, SHIFT, FRAMES = (100, 200), (1, 2), 4                                       # (y, x) of the first crop; the offset from frame to frame


def _script(name):
    return [sys.executable, os.path.join(ROOT, "scripts", name)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every child process of this module, started together and waited for once."""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("ft_runner")
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
    dirs = {}
    for tag in ("w1", "w3", "lr1", "lr3", "bi", "plain"):
        dirs[tag] = tmp / tag
        dirs[tag].mkdir()
    lists = {}
    for tag in ("bi", "plain"):
        lists[tag] = str(tmp / f"{tag}.txt")
        with open(lists[tag], "w") as f:
            for k in range(FRAMES - 1):
                f.write(f"{names[k]} {names[k + 1]} {dirs[tag] / ('out%d.flo' % k)}\n")
    net = ["--net", "C", "--weights", weights, "--general-conv", "own"]
    track, many = _script("track_flownet.py") + net + ["--alpha", repr(ALPHA[0]), repr(ALPHA[1])], _script("run_flownet_many.py") + net
    cmds = {
        "w1": track + ["--window", "1", frames, str(dirs["w1"])],
        "w3": track + ["--window", "3", frames, str(dirs["w3"])],
        "lr1": track + ["--window", "1", "--long-range", str(dirs["lr1"] / "lr.flo"), "--color", str(dirs["lr1"] / "lr.png"), frames, str(dirs["lr1"])],
        "lr3": track + ["--window", "3", "--long-range", str(dirs["lr3"] / "lr.flo"), "--color", str(dirs["lr3"] / "lr.png"), frames, str(dirs["lr3"])],
        "bi": many + ["--batch", "2", "--bidirectional", lists["bi"]],
        "plain": many + ["--batch", "2", lists["plain"]],
    }
    procs = {tag: subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for tag, cmd in cmds.items()}
    for tag, p in procs.items():
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f"{tag}: exit status {p.returncode}\n{out.decode()[-3000:]}"
    return {"tmp": tmp, "dirs": dirs}


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_tracks_npz_does_not_depend_on_the_window(runs):
    d = runs["dirs"]
    assert sorted(os.listdir(d["w1"])) == ["tracks.npz"] and evaluate.track_names(str(d["w1"])) == str(d["w1"] / "tracks.npz")
    assert _read(d["w1"] / "tracks.npz") == _read(d["w3"] / "tracks.npz")
    with np.load(str(d["w1"] / "tracks.npz")) as z:
        pos, ids, state = z["pos"], z["track_id"], z["state"]
    P = 16 * 16                                                                     # --cell 4 on 64 x 64
    assert pos.shape == (FRAMES, 2, P) and pos.dtype == np.float32 and ids.shape == (FRAMES, P) and ids.dtype == np.int32 and state.shape == (P,)
    assert ids[0].tolist() == list(range(P)) and pos[0, 0].reshape(16, 16)[3].tolist() == [1.5 + 4 * k for k in range(16)]
    assert np.array_equal(np.isnan(pos[:, 0]), ids < 0) and np.array_equal(np.isnan(pos[:, 1]), ids < 0)
    inside = ~np.isnan(pos)
    assert np.all(pos[inside] >= 0) and np.all(pos[:, 0][inside[:, 0]] < 64) and np.all(pos[:, 1][inside[:, 1]] < 64)
    # an id lives in one slot, through consecutive frames; a slot that gets a new id has lost the old one for good
    for p in range(P):
        seen = [i for i in ids[:, p].tolist() if i >= 0]
        assert seen == sorted(seen) and all(b - a == 0 or b >= P for a, b in zip(seen, seen[1:]))
    used = ids[ids >= 0]
    assert used.max() + 1 == len(np.unique(used))                                   # ids are handed out without gaps
    assert np.array_equal(state == 0, ids[-1] >= 0)
    moved = (ids[1:] == ids[:-1]) & (ids[1:] >= 0)                                  # a point carried from one frame to the next ...
    print("tracks:", int(moved.sum()), "carried steps,", int(used.max()) + 1, "trajectories in", P, "slots")
    assert moved.any() and used.max() >= P and (pos[1:][:, 0][moved] != pos[:-1][:, 0][moved]).any()      # ... has moved, and slots were reseeded


def test_long_range_flow_is_the_tracker_on_the_runners_flows(runs):
    d = runs["dirs"]
    for name in ("lr.flo", "lr.png", "tracks.npz"):
        assert _read(d["lr1"] / name) == _read(d["lr3"] / name), name
    assert sorted(os.listdir(d["lr1"])) == ["lr.flo", "lr.png", "tracks.npz"]
    pairs = range(FRAMES - 1)
    load = lambda name: torch.from_numpy(np.stack([flo.read_flo(str(d["bi"] / name.format(k))).transpose(2, 0, 1) for k in pairs])).cuda()
    fw, bw = load("out{}.flo"), load("out{}.bw.flo")                               # [T,2,H,W]
    flags = Fn.flow_consistency(fw, bw, flags=True).flags_fw
    t = Fn.flow_track(fw.unsqueeze(0), bw.unsqueeze(0), stop=flags.unsqueeze(0), alpha=ALPHA)
    want = t.long_range_flow()
    got = flo.read_flo(str(d["lr1"] / "lr.flo")).transpose(2, 0, 1)
    assert got.shape == (2, 64, 64) and np.array_equal(got.view(np.uint32), want[0].cpu().numpy().view(np.uint32))
    alive = t.state[0].cpu().numpy() == 0
    steps = t.steps[0].cpu().numpy()
    print("long range:", t.summary(), "steps histogram", np.bincount(steps, minlength=FRAMES).tolist(), "|fw| max", float(fw.abs().max()))
    assert np.array_equal(got[0].reshape(-1) != np.float32(1e10), alive)
    assert 0 < alive.sum() < alive.size and steps.max() == FRAMES - 1 and (steps == 0).any()      # the inputs make the comparison worth something
    rgb = visualize.read_png8(str(d["lr1"] / "lr.png"))
    assert rgb.shape == (64, 64, 3) and np.array_equal(rgb, Fn.flow_to_color(want)[0].cpu().numpy())
    with np.load(str(d["lr1"] / "tracks.npz")) as z:
        assert z["pos"].shape == (FRAMES, 2, 64 * 64) and np.array_equal(z["state"], t.state[0].cpu().numpy())
        reached = ~np.isnan(z["pos"])
        assert np.array_equal(z["pos"][reached].view(np.uint32), t.tracks[0].cpu().numpy()[reached].view(np.uint32))
        assert np.array_equal(z["track_id"][-1] >= 0, alive)


def test_the_per_pair_flows_keep_their_bytes(runs):
    d = runs["dirs"]
    for k in range(FRAMES - 1):
        plain = _read(d["plain"] / f"out{k}.flo")
        assert len(plain) == 12 + 64 * 64 * 8 and _read(d["bi"] / f"out{k}.flo") == plain
    assert sorted(os.listdir(d["plain"])) == [f"out{k}.flo" for k in range(FRAMES - 1)]
