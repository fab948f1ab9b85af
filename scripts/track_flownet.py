#!/usr/bin/env python
"""Dense point trajectories through a video on the MI355X path (after Sundaram, Brox and Keutzer, ECCV 2010).

    python scripts/track_flownet.py frames.txt OUT_DIR --weights W [--net C|S|2] [--window K] [--cell C] [--no-reseed]
    python scripts/track_flownet.py frames.txt OUT_DIR --weights W --long-range OUT.flo [--color OUT.png]

frames.txt lists one image per line, in order, all of one size.  For every consecutive pair the net runs in both directions in one step
(as run_flownet_many.py --bidirectional does), functional.flow_consistency supplies the motion-boundary flags, functional.flow_track
advances the points (they stop where they are occluded, leave the image or reach a motion boundary) and functional.flow_track_reseed
starts new points in the cells of `--cell` pixels that no point covers any more (`--no-reseed`: never).  `--window K` sends K pairs
through the net at once; the tracker is stepped per frame, so that the reseeding sees every frame.

OUT_DIR/tracks.npz holds pos float32 [F,2,P] (x, y of slot p in frame f; NaN where the slot is empty), track_id int32 [F,P] (-1 where
empty; a slot that is reseeded gets a new id) and state uint8 [P] (0 = alive in the last frame, else the reason the slot's last point
stopped).

`--long-range OUT.flo` tracks every pixel of frame 0 (--cell 1 --no-reseed) with ONE tracker call over the K frames of a window, and writes
the flow from frame 0 to the last frame (FlowTracks.long_range_flow: 1e10, the unknown-flow value, where the point was lost), with
`--color OUT.png` its colour coding.

The net runs in functional's batch-invariant mode and one tracker call over K frames equals K calls over one, so the bytes of every
output are the same for any --window.  Net loading, the arithmetic flags and --general-conv are run_flownet.py's / run_flownet_many.py's.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet2_amd import evaluate, flo, visualize  # noqa: E402
from flownet2_amd import functional as Fn  # noqa: E402
import run_flownet as RF  # noqa: E402
import run_flownet_many as RM  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("frames", help="text file: one image per line, in order")
    ap.add_argument("out_dir")
    ap.add_argument("--net", choices=["C", "S", "2"], default="C")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--window", type=int, default=1, metavar="K", help="pairs that go through the net at once")
    ap.add_argument("--cell", type=int, default=None, metavar="C", help="one point per C x C pixels (default 4)")
    ap.add_argument("--no-reseed", action="store_true", help="start no new points where coverage is lost")
    ap.add_argument("--long-range", default=None, metavar="OUT.flo", help="track every pixel of frame 0 (--cell 1 --no-reseed) and write "
                    "the flow from frame 0 to the last frame")
    ap.add_argument("--color", default=None, metavar="OUT.png", help="with --long-range: the long-range flow's colour coding")
    ap.add_argument("--alpha", type=float, nargs=2, default=[0.01, 0.5], metavar=("A1", "A2"), help="inconsistent: |a+b|^2 > A1 (|a|^2+|b|^2) + A2")
    ap.add_argument("--beta", type=float, nargs=2, default=[0.01, 0.002], metavar=("B1", "B2"), help="motion boundary: |grad|^2 > B1 |a|^2 + B2")
    Fn.add_arithmetic_flags(ap, RM.ARITH)
    Fn.add_general_convolution_flag(ap)
    a = ap.parse_args(argv)
    if a.window < 1:
        ap.error("--window must be at least 1")
    if a.color and not a.long_range:
        ap.error("--color draws the long-range flow: it needs --long-range")
    if a.long_range:
        if a.cell not in (None, 1):
            ap.error("--long-range tracks every pixel: --cell is 1")
        a.cell, a.no_reseed = 1, True
    a.cell = 4 if a.cell is None else a.cell
    if a.cell < 1:
        ap.error("--cell must be at least 1")
    return a


def next_ids(ids, next_id, state, born):
    """The trajectory ids [P] after a tracker step and a reseed: -1 where the slot's point has stopped, a new id (counting on from
    next_id, in slot order) where a point was born.  -> (ids, the next unused id)."""
    ids = np.where(np.asarray(state) != 0, -1, ids).astype(np.int32)
    new = np.flatnonzero(np.asarray(born) != 0)
    ids[new] = next_id + np.arange(new.size, dtype=np.int32)
    return ids, next_id + int(new.size)


def windows(paths, k, read):
    """Yield (index of the first pair, frames [n + 1,3,H,W]) for windows of at most k consecutive pairs; every file is read once."""
    last = read(paths[0])
    for start in range(0, len(paths) - 1, k):
        frames = [last] + [read(p) for p in paths[start + 1:start + 1 + k]]
        for f in frames[1:]:
            if f.shape != last.shape:
                raise SystemExit(f"frames differ in size: {f.shape[2:]} against {last.shape[2:]}")
        last = frames[-1]
        yield start, np.concatenate(frames)


def main():
    a = parse_args()
    paths = [l.strip() for l in open(a.frames) if l.strip()]
    if len(paths) < 2:
        raise SystemExit("need at least two frames")
    for p in paths:
        if not os.path.exists(p):
            raise SystemExit("image does not exist: " + p)
    os.makedirs(a.out_dir, exist_ok=True)
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    Fn.set_batch_invariant(True)                    # a pair's flow does not depend on the window it was computed in
    Fn.apply_arithmetic_flags(a, RM.ARITH)
    Fn.apply_general_convolution_flag(a)
    P, mean = RF.load_params(a.net, a.weights, dev)
    alpha, beta = tuple(a.alpha), tuple(a.beta)

    points = state = ids = None
    pos, track_ids, calls, next_id = [], [], [], 0
    for _, frames in windows(paths, a.window, RF.read_image):
        f = torch.from_numpy(frames).to(dev)
        n = f.shape[0] - 1
        flow = RF.infer(a.net, P, torch.cat([f[:-1], f[1:]]), torch.cat([f[1:], f[:-1]]), mean)      # rows 0 .. n-1 forward, n .. 2n-1 backward
        fw, bw = flow[:n].contiguous(), flow[n:].contiguous()
        H, W = fw.shape[2:]
        with torch.no_grad():
            flags = Fn.flow_consistency(fw, bw, alpha=alpha, beta=beta, flags=True).flags_fw
            if points is None:
                points = Fn.flow_track_grid(1, H, W, a.cell, device=dev)
                state = torch.zeros((1, points.shape[2]), dtype=torch.uint8, device=dev)
                ids, next_id = next_ids(np.zeros(points.shape[2], np.int32), 0, state[0].cpu().numpy(), np.ones(points.shape[2], np.uint8))
                pos.append(points[0].cpu().numpy())
                track_ids.append(ids)
            if a.long_range:                            # one call over the window's frames
                calls.append(Fn.flow_track(fw.unsqueeze(0), bw.unsqueeze(0), points=points, state=state, stop=flags.unsqueeze(0), alpha=alpha))
                points, state = calls[-1].points, calls[-1].state
                continue
            for k in range(n):                          # one call per frame: the reseeding looks at every frame
                t = Fn.flow_track(fw[k:k + 1], bw[k:k + 1], points=points, state=state, stop=flags[k:k + 1], alpha=alpha, tracks=False)
                points, state = t.points, t.state
                stopped = state[0].cpu().numpy()
                born = np.zeros_like(stopped)
                if not a.no_reseed:
                    born = Fn.flow_track_reseed(points, state, (H, W), a.cell)[0].cpu().numpy()
                ids, next_id = next_ids(ids, next_id, stopped, born)
                here = points[0].cpu().numpy()
                pos.append(np.where(ids >= 0, here, np.float32(np.nan)))
                track_ids.append(ids)

    out = evaluate.track_names(a.out_dir)
    if a.long_range:
        whole = calls[0].merge(calls[1:]) if len(calls) > 1 else calls[0]
        tracks = whole.tracks[0].cpu().numpy()                                                  # [F,2,P], NaN after the stop
        alive = ~np.isnan(tracks[:, 0])
        alive[0] = True
        evaluate.write_tracks_npz(out, tracks, np.where(alive, np.arange(tracks.shape[2], dtype=np.int32), -1), whole.state[0].cpu().numpy())
        lr = whole.long_range_flow()
        flo.write_flo(a.long_range, lr[0].cpu().numpy())
        print("wrote", a.long_range, tuple(lr.shape[2:]), evaluate.json_ready(whole.summary()))
        if a.color:
            with torch.no_grad():
                visualize.write_png(a.color, Fn.flow_to_color(lr.contiguous())[0])
            print("wrote", a.color)
    else:
        evaluate.write_tracks_npz(out, np.stack(pos), np.stack(track_ids), state[0].cpu().numpy())
    print(f"wrote {out}: {len(paths)} frames, {points.shape[2]} slots, {next_id} trajectories")


if __name__ == "__main__":
    main()
