#!/usr/bin/env python
"""In-between frames of a video on the MI355X path: FlowNet in both directions, then softmax splatting (functional.flow_interpolate).

    python scripts/interpolate_flownet.py frames.txt OUT_DIR --weights W [--net C|S|2] [--times 0.5 ...] | [--factor K] [--alpha A] [--batch B]

frames.txt lists one image per line, in order, all of one size.  For every consecutive pair (k, k + 1) the net runs in both directions in
one step (as track_flownet.py does), and for every time t the frame between them is written to OUT_DIR/frame<k>_t<t>.png
(visualize.write_png; t with three decimals).  --times gives the times in (0, 1); --factor K stands for 1/K, 2/K, ..., (K-1)/K (K = 2, the
default, is the one frame in the middle).  --alpha is flow_interpolate's knob: how strongly a pixel whose brightness the flow does not
explain gives way where several land on one cell; its default is arbitrary.  Nothing is learned and nothing refines the frame: what no
pixel of either frame reaches is the cross-fade of the two frames.

--batch B sends B pairs through the net and through the splatting at once.  The net runs in functional's batch-invariant mode and the
splat's sum at a cell depends on the sample alone, so the bytes of every file are the same for any --batch.  Net loading, the arithmetic
flags and --general-conv are run_flownet.py's / run_flownet_many.py's.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet2_amd import visualize  # noqa: E402
from flownet2_amd import functional as Fn  # noqa: E402
import run_flownet as RF  # noqa: E402
import run_flownet_many as RM  # noqa: E402
from track_flownet import windows  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("frames", help="text file: one image per line, in order")
    ap.add_argument("out_dir")
    ap.add_argument("--net", choices=["C", "S", "2"], default="C")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--times", type=float, nargs="+", default=None, metavar="T", help="times in (0, 1) between a pair of frames")
    ap.add_argument("--factor", type=int, default=None, metavar="K", help="K - 1 frames per pair, at 1/K ... (K-1)/K (default 2)")
    ap.add_argument("--alpha", type=float, default=20.0, metavar="A", help="flow_interpolate's importance knob")
    ap.add_argument("--batch", type=int, default=1, metavar="B", help="pairs that go through the net and the splatting at once")
    Fn.add_arithmetic_flags(ap, RM.ARITH)
    Fn.add_general_convolution_flag(ap)
    return ap


def times_of(a):
    """The times asked for, ascending; exits on a contradiction."""
    if a.times is not None and a.factor is not None:
        raise SystemExit("--times and --factor exclude one another")
    if a.times is not None:
        if not all(0.0 < t < 1.0 for t in a.times):
            raise SystemExit("--times must lie in (0, 1)")
        return sorted(a.times)
    k = 2 if a.factor is None else a.factor
    if k < 2:
        raise SystemExit("--factor must be at least 2")
    return [i / k for i in range(1, k)]


def frame_name(out_dir, k, t):
    return os.path.join(out_dir, "frame%05d_t%.3f.png" % (k, t))


def to_png(frame):
    """[3,H,W] BGR float in [0, 255] (run_flownet.read_image's layout) -> uint8 [H,W,3] RGB, rounded to nearest."""
    return frame.clamp(0.0, 255.0).add(0.5).floor().to(torch.uint8)[[2, 1, 0]].permute(1, 2, 0).contiguous()


def main():
    a = build_parser().parse_args()
    times = times_of(a)
    if a.batch < 1:
        raise SystemExit("--batch must be at least 1")
    paths = [l.strip() for l in open(a.frames) if l.strip()]
    if len(paths) < 2:
        raise SystemExit("need at least two frames")
    for p in paths:
        if not os.path.exists(p):
            raise SystemExit("image does not exist: " + p)
    os.makedirs(a.out_dir, exist_ok=True)
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    Fn.set_batch_invariant(True)                    # a pair's flow does not depend on the batch it was computed in
    Fn.apply_arithmetic_flags(a, RM.ARITH)
    Fn.apply_general_convolution_flag(a)
    P, mean = RF.load_params(a.net, a.weights, dev)
    written = 0
    for start, frames in windows(paths, a.batch, RF.read_image):
        if frames.shape[1] != 3:
            raise SystemExit("the frames must be colour images")
        f = torch.from_numpy(frames).to(dev)
        n = f.shape[0] - 1
        i0, i1 = f[:-1].contiguous(), f[1:].contiguous()
        flow = RF.infer(a.net, P, torch.cat([i0, i1]), torch.cat([i1, i0]), mean)      # rows 0 .. n-1 forward, n .. 2n-1 backward
        fw, bw = flow[:n].contiguous(), flow[n:].contiguous()
        for t in times:
            mid = Fn.flow_interpolate(i0, i1, fw, bw, t, alpha=a.alpha)
            for k in range(n):
                visualize.write_png(frame_name(a.out_dir, start + k, t), to_png(mid[k]))
                written += 1
    print(f"wrote {written} frames to {a.out_dir}: {len(paths) - 1} pairs, times {times}")


if __name__ == "__main__":
    main()
