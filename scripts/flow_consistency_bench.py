#!/usr/bin/env python
"""Timing of the fused forward-backward consistency call (csrc/flow_consistency.hip: flow_consistency_partial + flow_consistency_final)
against the same check composed by hand from functional.flow_warp (twice, FILL_NAN) and eager torch operations, on the same blobs in one
process, at [8,2,320,448] (FlowNetC's training crop, batch 8) and [4,2,384,768] (a KITTI-sized crop, batch 4).  Inputs: smooth random
flows of a few pixels, the backward flow near the negative of the forward one, and a pasted rectangle (the occluder) that moves
differently in the forward flow.
  fused              ops.flow_consistency: the ctypes call, the allocations (workspace, results, the two occ planes), two launches
  fused + all maps   the same with the flag, err and warped maps of both directions written
  composed           per direction flow_warp, the finite / inside tests, the central differences on clamped slices, the two thresholds as
                     boolean maps, occ, err and one per-sample fp64 reduction per column
Run on the GPU box:
    python scripts/flow_consistency_bench.py [--iters 200] [--repeats 7] [--out profiles/flow_consistency.md]
Device events around `iters` back-to-back calls, a warm-up of every variant first, the variants alternating inside every repeat.  Per
variant: the median over the repeats of the mean time per call with min .. max of the repeats, the bytes the fused pass has to move (fw,
bw read once: 16 B per pixel; the occ planes 8; flags 2, err 8, warped 16 -- the taps and the neighbours come from the caches) and those
bytes over the time as a share of the 6.3 TB/s a streaming kernel reaches on this chip.  For the composed form the same bytes are the
LEAST it could move; it moves many times more."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flownet2_amd import ops  # noqa: E402
from flownet2_amd import functional as Fn  # noqa: E402

HBM_ROOF = 6.3e12          # bytes / s, measured streaming rate (float4 copy) of an MI355X; the data sheet says 8.0e12
SHAPES = [(8, 2, 320, 448), (4, 2, 384, 768)]
ALPHA, BETA = (0.01, 0.5), (0.01, 0.002)


def timeit(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters           # us per call


def make_flows(shape, g):
    N, _, H, W = shape
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    fw = torch.empty(shape)
    for n in range(N):
        for c in range(2):
            amp, fx, fy, p0, p1, off = (torch.rand((), generator=g).item() for _ in range(6))
            fw[n, c] = (1 + 5 * amp) * torch.sin((0.005 + 0.03 * fx) * x + 6.28 * p0) * torch.cos((0.005 + 0.03 * fy) * y + 6.28 * p1) + 4 * off - 2
    bw = -fw + 0.05 * torch.randn(shape, generator=g)
    fw[:, 0, H // 4:H // 4 + H // 3, W // 4:W // 4 + W // 3] += 9.0        # the occluder
    fw[:, 1, H // 4:H // 4 + H // 3, W // 4:W // 4 + W // 3] -= 6.0
    return fw.cuda(), bw.cuda()


def composed_direction(a, o):
    """One direction of include/flownet2_hip_flow_consistency.h as flow_warp + torch operations -> (occ [N,1,H,W], [N, 8] float64 rows)."""
    N, _, H, W = a.shape
    au, av = a[:, 0], a[:, 1]
    fin = (au.abs() <= 1e9) & (av.abs() <= 1e9)
    dx = lambda t: 0.5 * (torch.cat([t[:, :, 1:], t[:, :, -1:]], 2) - torch.cat([t[:, :, :1], t[:, :, :-1]], 2))
    dy = lambda t: 0.5 * (torch.cat([t[:, 1:], t[:, -1:]], 1) - torch.cat([t[:, :1], t[:, :-1]], 1))
    ux, uy, vx, vy = dx(au), dy(au), dx(av), dy(av)
    g = ux * ux + uy * uy + vx * vx + vy * vy
    mag = au * au + av * av
    boundary = fin & (g > BETA[0] * mag + BETA[1])                       # a NaN neighbour makes g NaN: no flag
    x2 = torch.arange(W, device=a.device, dtype=torch.float32).view(1, 1, W) + au
    y2 = torch.arange(H, device=a.device, dtype=torch.float32).view(1, H, 1) + av
    inside = fin & (x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H)
    b = Fn.flow_warp(o, a, ops.FILL_NAN)
    bu, bv = b[:, 0], b[:, 1]
    full = inside & (bu.abs() <= 1e9) & (bv.abs() <= 1e9)
    su, sv = au + bu, av + bv
    s = su * su + sv * sv
    m = mag + (bu * bu + bv * bv)
    inconsistent = full & (s > ALPHA[0] * m + ALPHA[1])
    nonfinite, outside = ~fin | (inside & ~full), fin & ~inside
    occluded = nonfinite | outside | inconsistent
    err = torch.where(full, s.sqrt(), torch.zeros((), device=a.device))
    tot = lambda t: t.flatten(1).sum(1, dtype=torch.float64)
    rows = torch.stack([torch.full((N,), float(H * W), dtype=torch.float64, device=a.device), tot(nonfinite), tot(outside), tot(inconsistent),
                        tot(occluded), tot(boundary), tot(err), err.flatten(1).max(1).values.double()], 1)
    return occluded.float().unsqueeze(1), rows


def composed(fw, bw):
    return composed_direction(fw, bw), composed_direction(bw, fw)


def count_kernels(fn):
    """Device kernels one call of fn launches, from torch's profiler; None where the profiler reports no device events."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
        return n or None
    except Exception as e:      # noqa: BLE001 -- a count is a footnote; the timings do not depend on it
        print("kernel count not available:", e, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_consistency.md"))
    a = ap.parse_args()
    lines = ["# Forward-backward consistency: the fused call against flow_warp plus eager torch operations", "",
             "Written by `scripts/flow_consistency_bench.py` on an MI355X; all figures of this file come from one run of it.  Device events "
             f"around {a.iters} back-to-back calls, every variant warmed up first, the variants alternating inside each of {a.repeats} repeats; "
             "`median (min .. max)` over the repeats of the mean time per call.  A call includes its host side (the ctypes call or the torch "
             "dispatches, the output allocations).  Bytes: what the fused pass must move for both directions -- 16 B per pixel read (fw, bw, "
             "each once; taps and neighbours come from the caches), 8 written for the two occ planes, 26 more with the flag, err and warped "
             "maps -- and for the composed form the same figure as the plain fused call, the least it could move.  Launches: two for the "
             "fused call; the composed form's are counted from its own trace below.", ""]
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for shape in SHAPES:
            N, _, H, W = shape
            fw, bw = make_flows(shape, g)
            variants = {"fused": lambda: ops.flow_consistency(fw, bw, ALPHA, BETA),
                        "fused + all maps": lambda: ops.flow_consistency(fw, bw, ALPHA, BETA, flags=True, err=True, warped=True),
                        "composed": lambda: composed(fw, bw)}
            # the two forms compute the same thing: flow_warp contracts its four products, so a pixel on a threshold may fall either way
            results, occ = ops.flow_consistency(fw, bw, ALPHA, BETA)[:2]
            ref = composed(fw, bw)
            px = N * H * W
            for d in range(2):
                differ = int((occ[d] != ref[d][0]).sum())
                assert differ <= 1e-4 * px, f"direction {d}: {differ} of {px} occ pixels differ"
                assert torch.allclose(results[d, :N], ref[d][1], rtol=1e-3, atol=0), (results[d, :N], ref[d][1])
            launches = count_kernels(lambda: composed(fw, bw))
            for fn in variants.values():
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            times = {n: [] for n in variants}
            for _ in range(a.repeats):
                for n, fn in variants.items():
                    times[n].append(timeit(fn, a.iters))
            occluded = float(results[0, N, 4] / results[0, N, 0])
            lines += [f"## [{N},2,{H},{W}]: {px} pixels, {100 * occluded:.1f} % occluded in the forward direction", "",
                      "| variant | us per call, median (min .. max) | bytes moved | share of 6.3 TB/s |", "|---|---|---|---|"]
            med = {}
            for n, ts in times.items():
                moved = px * (50 if n == "fused + all maps" else 24)
                med[n] = statistics.median(ts)
                lines.append("| %s | %.2f (%.2f .. %.2f) | %.2f MB | %.1f %% |" % (n, med[n], min(ts), max(ts), moved / 1e6, 100 * moved / (med[n] * 1e-6) / HBM_ROOF))
            ratio = med["composed"] / med["fused"]
            lines += ["", "composed / fused = %.1f (medians): the fused call is %s.  Device activities (kernels and copies, from torch's profiler) in one composed call: %s (fused: 2)." % (
                ratio, "faster" if ratio > 1 else "NOT faster: the expectation does not hold here", "not counted" if launches is None else launches), ""]
            assert math.isfinite(ratio)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
