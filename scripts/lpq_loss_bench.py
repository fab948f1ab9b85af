#!/usr/bin/env python
"""Timing of the one-launch LpqLoss (csrc/lpq_loss.hip: lpq_fwd_multi / lpq_bwd_multi) at FlowNetC's five training scales, batch 8
@448x320 (predictions [8, 2, 5 x 7] ... [8, 2, 80 x 112] and targets of the same shapes), on the same blobs in one process:
  lpq p=2 q=0.2      the small-displacement form (powf twice per element in the forward, three times in the backward)
  lpq p=2 q=0.5      the L1Loss{l2_per_location} function on the new kernel (powf in the forward; the p side of the backward is 2 t)
  l1 multi           the same function on the existing kernel (csrc/l1loss.hip: l1loss_fwd_multi / l1loss_bwd_multi), d d and sqrtf
  torch composite    abs, pow, sum per scale as eager torch ops (forward) and their autograd backward: what the layer costs without a kernel
Run on the GPU box:
    python scripts/lpq_loss_bench.py [--iters 200] [--repeats 7] [--batch 8]
Device events around `iters` back-to-back calls, a warm-up of every variant first, the variants alternating inside every repeat.  Per
variant and direction: the median over the repeats of the mean time per call, the spread (min .. max over the repeats), and the bytes
the pass has to move (forward: both bottoms read; backward: both bottoms read, both diffs written) over that time as a share of the
6.3 TB/s a streaming kernel reaches on this chip.  The five scales hold 0.76 MB of predictions in all: a pass of this size is bound by
its launch and the one-workgroup finalise, not by HBM, and the share says so."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flownet2_amd import nets, ops  # noqa: E402

HBM_ROOF = 6.3e12          # bytes / s, measured streaming rate (float4 copy) of an MI355X; the data sheet says 8.0e12


def timeit(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters           # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=448)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    scales = list(nets.LOSS_WEIGHTS.items())
    shapes = [(a.batch, 2, a.height >> s, a.width >> s) for s, _ in scales]
    preds = [(torch.randn(sh, generator=g) * 0.5).cuda() for sh in shapes]
    tgts = [(torch.randn(sh, generator=g) * 0.5).cuda() for sh in shapes]
    for t in tgts:
        t[0, :, 0, 0] = float("nan")
    weights = [w for _, w in scales]
    total_diff = torch.ones((), device="cuda")
    nbytes = sum(p.numel() * 4 for p in preds)

    variants = {}
    for name, (p, q) in (("lpq p=2 q=0.2", (2.0, 0.2)), ("lpq p=2 q=0.5", (2.0, 0.5))):
        params = ops.lpq_params(p, q, 0.0, 1e-2, False, True)
        ws = ops.lpq_loss_forward_multi(params, preds, tgts, weights)[2]
        variants[name] = (lambda params=params: ops.lpq_loss_forward_multi(params, preds, tgts, weights),
                          lambda params=params, ws=ws: ops.lpq_loss_backward_multi(params, preds, tgts, weights, total_diff, ws, need1=True))
    l1 = ops.l1_params(True, False, True, 1e-2, 0.0)
    l1ws = ops.l1loss_forward_multi(l1, preds, tgts, weights)[2]
    variants["l1 multi"] = (lambda: ops.l1loss_forward_multi(l1, preds, tgts, weights),
                            lambda: ops.l1loss_backward_multi(l1, preds, tgts, weights, total_diff, l1ws, need1=True))

    def composite(p, q):
        total = 0.0
        for x, t, w in zip(leaves, tleaves, weights):
            d = torch.nan_to_num(x - t, nan=0.0)
            total = total + w * ((d.abs() ** p).sum(1) + 1e-2).pow(q).sum() / x.shape[0]
        return total
    leaves = [p.clone().requires_grad_(True) for p in preds]
    tleaves = [t.clone().requires_grad_(True) for t in tgts]

    def composite_backward():
        torch.autograd.grad(composite(2.0, 0.2), leaves + tleaves)
    variants["torch composite (forward; forward + backward)"] = (lambda: composite(2.0, 0.2), composite_backward)

    for fwd, bwd in variants.values():                  # warm-up
        for _ in range(10):
            fwd(), bwd()
    torch.cuda.synchronize()
    times = {(n, d): [] for n in variants for d in ("forward", "backward")}
    for _ in range(a.repeats):
        for n, (fwd, bwd) in variants.items():
            times[(n, "forward")].append(timeit(fwd, a.iters))
            times[(n, "backward")].append(timeit(bwd, a.iters))
    print("one-launch loss of %d scales, batch %d @%dx%d: %.2f MB of predictions, as much of targets" % (len(scales), a.batch, a.width, a.height, nbytes / 1e6))
    print("| variant | direction | us per call, median (min .. max of %d repeats x %d calls) | bytes moved | share of 6.3 TB/s |\n|---|---|---|---|---|"
          % (a.repeats, a.iters))
    for (n, d), ts in times.items():
        moved = 2 * nbytes if d == "forward" else 4 * nbytes
        med = statistics.median(ts)
        print("| %s | %s | %.2f (%.2f .. %.2f) | %.2f MB | %.2f %% |" % (n, d, med, min(ts), max(ts), moved / 1e6, 100 * moved / (med * 1e-6) / HBM_ROOF))
    print("(a call includes its host side -- the ctypes call, the output allocations, one launch -- which is what bounds back-to-back calls of "
          "this size; a larger --batch shows the kernels themselves)")


if __name__ == "__main__":
    main()
