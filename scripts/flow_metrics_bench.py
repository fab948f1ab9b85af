#!/usr/bin/env python
"""Timing of the fused flow-metrics call (csrc/flow_metrics.hip: flow_metrics_partial + flow_metrics_final) against the same metrics
written as eager torch operations, on the same blobs in one process, at [8,2,320,448] (FlowNetC's training crop, batch 8) and
[4,2,384,768] (a KITTI-sized crop, batch 4), with `valid` and `occ` masks:
  fused              ops.flow_metrics: the ctypes call, three allocations (workspace, results, no map), two launches
  fused + epe_map    the same with the [N,1,H,W] EPE map written
  eager torch        validity, differences, sqrt, atan2, the classifications as boolean maps and one per-sample fp64 reduction per column
Run on the GPU box:
    python scripts/flow_metrics_bench.py [--iters 200] [--repeats 7] [--out profiles/flow_metrics.md]
Device events around `iters` back-to-back calls, a warm-up of every variant first, the variants alternating inside every repeat.  Per
variant: the median over the repeats of the mean time per call with min .. max of the repeats, the bytes the fused pass has to move
(pred, gt: 16 B per pixel; valid, occ: 8; the map: 4 -- read or written once) and those bytes over the time as a share of the 6.3 TB/s
a streaming kernel reaches on this chip.  For the eager form the same bytes are the LEAST it could move; it moves many times more."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flownet2_amd import ops  # noqa: E402

HBM_ROOF = 6.3e12          # bytes / s, measured streaming rate (float4 copy) of an MI355X; the data sheet says 8.0e12
SHAPES = [(8, 2, 320, 448), (4, 2, 384, 768)]


def timeit(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters           # us per call


def eager(pred, gt, valid, occ, outlier=(3.0, 0.05), bands=(10.0, 40.0)):
    """The arithmetic of include/flownet2_hip_flow_metrics.h as torch operations -> [N, K] float64 rows in the kernel's column order."""
    pu, pv, gu, gv = pred[:, 0], pred[:, 1], gt[:, 0], gt[:, 1]
    ok = ~torch.isnan(gu) & ~torch.isnan(gv) & (gu.abs() <= 1e9) & (gv.abs() <= 1e9) & (valid[:, 0] != 0)
    finite = torch.isfinite(pu) & torch.isfinite(pv)
    nonfinite, c = ok & ~finite, ok & finite
    zero = torch.zeros((), device=pred.device)
    pu, pv, gu, gv = (torch.where(c, t, zero) for t in (pu, pv, gu, gv))
    du, dv = pu - gu, pv - gv
    s = du * du + dv * dv
    epe = s.sqrt()
    mag = (gu * gu + gv * gv).sqrt()
    cx, cy, cz = pv - gv, gu - pu, pu * gv - pv * gu
    ae = torch.atan2((cx * cx + cy * cy + cz * cz).sqrt(), 1 + pu * gu + pv * gv)
    outl = c & (epe > outlier[0]) & (epe > outlier[1] * mag)
    band = [c & (mag < bands[0]), c & (mag >= bands[0]) & (mag < bands[1]), c & (mag >= bands[1])]
    occl = c & (occ[:, 0] != 0)
    tot = lambda t: t.flatten(1).sum(1, dtype=torch.float64)
    cols = [tot(c), tot(nonfinite), tot(epe), tot(s), epe.flatten(1).max(1).values.double(), tot(outl), tot(ae)]
    cols += [tot(b) for b in band] + [tot(torch.where(b, epe, zero)) for b in band] + [tot(occl), tot(torch.where(occl, epe, zero))]
    return torch.stack(cols, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_metrics.md"))
    a = ap.parse_args()
    lines = ["# Flow metrics: the fused call against eager torch operations", "",
             "Written by `scripts/flow_metrics_bench.py` on an MI355X; all figures of this file come from one run of it.  Device events around "
             f"{a.iters} back-to-back calls, every variant warmed up first, the variants alternating inside each of {a.repeats} repeats; "
             "`median (min .. max)` over the repeats of the mean time per call.  A call includes its host side (the ctypes call or the torch "
             "dispatches, the output allocations).  Bytes: what the fused pass must move -- 24 B per pixel read (pred, gt, valid, occ), 4 more "
             "written with the EPE map -- and for the eager form the same figure, the least it could move.", ""]
    g = torch.Generator().manual_seed(0)
    for shape in SHAPES:
        N, _, H, W = shape
        gt = (torch.randn(shape, generator=g) * 15).cuda()
        pred = gt + (torch.randn(shape, generator=g) * 2).cuda()
        gt[:, :, :8, :8] = float("nan")
        valid = (torch.rand((N, 1, H, W), generator=g) < 0.9).float().cuda()
        occ = (torch.rand((N, 1, H, W), generator=g) < 0.2).float().cuda()
        variants = {"fused": lambda: ops.flow_metrics(pred, gt, valid, occ),
                    "fused + epe_map": lambda: ops.flow_metrics(pred, gt, valid, occ, epe_map=True),
                    "eager torch": lambda: eager(pred, gt, valid, occ)}
        # the two forms compute the same thing: counts equal, sums to fp32 rounding
        rows, ref = ops.flow_metrics(pred, gt, valid, occ)[0][:N], eager(pred, gt, valid, occ)
        counts = [0, 1, 5, 7, 8, 9, 13]
        assert torch.equal(rows[:, counts], ref[:, counts]) and torch.allclose(rows, ref, rtol=1e-5, atol=0)
        for fn in variants.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n in variants}
        for _ in range(a.repeats):
            for n, fn in variants.items():
                times[n].append(timeit(fn, a.iters))
        px = N * H * W
        lines += [f"## [{N},2,{H},{W}]: {px} pixels", "", "| variant | us per call, median (min .. max) | bytes moved | share of 6.3 TB/s |", "|---|---|---|---|"]
        med = {}
        for n, ts in times.items():
            moved = px * (28 if n == "fused + epe_map" else 24)
            med[n] = statistics.median(ts)
            lines.append("| %s | %.2f (%.2f .. %.2f) | %.2f MB | %.1f %% |" % (n, med[n], min(ts), max(ts), moved / 1e6, 100 * moved / (med[n] * 1e-6) / HBM_ROOF))
        ratio = med["eager torch"] / med["fused"]
        lines += ["", "eager / fused = %.1f (medians): the fused call is %s." % (ratio, "faster" if ratio > 1 else "NOT faster: the expectation does not hold here"), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
