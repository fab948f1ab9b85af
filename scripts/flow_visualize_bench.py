#!/usr/bin/env python
"""Timing of the fused visualisation calls (csrc/flow_visualize.hip: flow_color_max + flow_color, flow_error_map) against the same
pictures composed from eager torch operations, on the same blobs in one process, at [8,2,320,448] (FlowNetC's training crop, batch 8) and
[4,2,384,768] (a KITTI-sized crop, batch 4).  Inputs: smooth random flows of a few pixels; the prediction is the ground truth plus an
error whose size spans every bin of the error image.
  color, sample      ops.flow_color under NORM_SAMPLE: the ctypes call, the allocations (workspace, rgb), two launches
  color, fixed       the same under NORM_FIXED: one launch, no workspace
  error map          ops.flow_error_map without valid / occ: one launch
  composed ...       the arithmetic of include/flownet2_hip_flow_visualize.h as torch operations on the device (the maximum stays on the
                     device there too: no host readback in either form)
Run on the GPU box:
    python scripts/flow_visualize_bench.py [--iters 200] [--repeats 7] [--out profiles/flow_visualize.md]
Device events around `iters` back-to-back calls, a warm-up of every variant first, the variants alternating inside every repeat.  Per
variant: the median over the repeats of the mean time per call with min .. max of the repeats, the bytes the fused pass has to move
(colour coding: 8 B per pixel read and 3 written, 8 more read by the maximum pass; error image: 16 read, 3 written) and those bytes over
the time as a share of the 6.3 TB/s a streaming kernel reaches on this chip.  For a composed form the same bytes are the LEAST it could
move; it moves many times more."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flownet2_amd import ops  # noqa: E402

HBM_ROOF = 6.3e12          # bytes / s, measured streaming rate (float4 copy) of an MI355X; the data sheet says 8.0e12
SHAPES = [(8, 2, 320, 448), (4, 2, 384, 768)]
FIXED_MAX = 4.0
ABS_THRESH, REL_THRESH = 3.0, 0.05
BYTES = {"color, sample": 19, "color, fixed": 11, "error map": 19}          # per pixel, fused; "composed X" is charged the same


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
    gt = torch.empty(shape)
    for n in range(N):
        for c in range(2):
            amp, fx, fy, p0, p1, off = (torch.rand((), generator=g).item() for _ in range(6))
            gt[n, c] = (1 + 5 * amp) * torch.sin((0.005 + 0.03 * fx) * x + 6.28 * p0) * torch.cos((0.005 + 0.03 * fy) * y + 6.28 * p1) + 4 * off - 2
    err = torch.randn(shape, generator=g) * torch.exp(8 * torch.rand((N, 1, H, W), generator=g) - 4)
    return (gt + err).cuda(), gt.cuda()


def wheel(device):
    w = [(255, 255 * i // 15, 0) for i in range(15)] + [(255 - 255 * i // 6, 255, 0) for i in range(6)] + [(0, 255, 255 * i // 4) for i in range(4)]
    w += [(0, 255 - 255 * i // 11, 255) for i in range(11)] + [(255 * i // 13, 0, 255) for i in range(13)] + [(255, 0, 255 - 255 * i // 6) for i in range(6)]
    return torch.tensor(w, dtype=torch.float32, device=device)


def composed_color(flow, table, max_flow=None):
    N = flow.shape[0]
    u, v = flow[:, 0], flow[:, 1]
    known = (u.abs() <= 1e9) & (v.abs() <= 1e9)
    zero = torch.zeros((), device=flow.device)
    u, v = torch.where(known, u, zero), torch.where(known, v, zero)
    rad = (u * u + v * v).sqrt()
    if max_flow is None:
        m = rad.flatten(1).max(1).values
        maxrad = torch.where(m > 0, m, torch.ones((), device=flow.device)).view(N, 1, 1)
    else:
        maxrad = max_flow
    rn = (rad / maxrad).unsqueeze(-1)
    fk = (torch.atan2(-v, -u) / math.pi + 1.0) * 0.5 * 54.0
    k0 = fk.to(torch.int64).clamp(0, 54)
    f = (fk - k0).unsqueeze(-1)
    w0, w1 = table[k0], table[(k0 + 1) % 55]
    c = w0 + f * (w1 - w0)
    out = torch.where(rn <= 1, 255.0 - rn * (255.0 - c), 0.75 * c)
    return torch.where(known.unsqueeze(-1), out.to(torch.int32), torch.zeros((), dtype=torch.int32, device=flow.device)).to(torch.uint8)


def composed_error(pred, gt, edges, colors):
    pu, pv, gu, gv = pred[:, 0], pred[:, 1], gt[:, 0], gt[:, 1]
    use = (gu.abs() <= 1e9) & (gv.abs() <= 1e9)
    fin = use & (pu.abs() <= 1e9) & (pv.abs() <= 1e9)
    du, dv = pu - gu, pv - gv
    epe = (du * du + dv * dv).sqrt()
    mag = (gu * gu + gv * gv).sqrt()
    n = epe / ABS_THRESH
    n = torch.where(mag > 0, torch.minimum(n, epe / mag / REL_THRESH), n)
    bins = torch.where(fin, torch.bucketize(n, edges, right=True), torch.full((), 9, dtype=torch.int64, device=pred.device))
    return torch.where(use.unsqueeze(-1), colors[bins], torch.zeros((), dtype=torch.uint8, device=pred.device))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_visualize.md"))
    a = ap.parse_args()
    lines = ["# Flow visualisation: the fused calls against eager torch operations", "",
             "Written by `scripts/flow_visualize_bench.py` on an MI355X; all figures of this file come from one run of it.  Device events "
             f"around {a.iters} back-to-back calls, every variant warmed up first, the variants alternating inside each of {a.repeats} repeats; "
             "`median (min .. max)` over the repeats of the mean time per call.  A call includes its host side (the ctypes call or the torch "
             "dispatches, the output allocations).  Bytes: what the fused pass must move -- the colour coding reads 8 B per pixel and writes "
             "3, and reads 8 more in the maximum pass of the per-sample normalisation; the error image (no valid / occ plane) reads 16 and "
             "writes 3 -- and for a composed form the same figure as its fused call, the least it could move.  Launches: two for the colour "
             "coding under NORM_SAMPLE, one under NORM_FIXED, one for the error image; the composed forms' are counted from their own traces "
             "below.", ""]
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for shape in SHAPES:
            N, _, H, W = shape
            pred, gt = make_flows(shape, g)
            table = wheel(pred.device)
            edges = torch.tensor([0.0625, 0.125, 0.25, 0.5, 1, 2, 4, 8, 16], dtype=torch.float32, device=pred.device)
            colors = torch.tensor([(49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248), (254, 224, 144), (253, 174, 97),
                                   (244, 109, 67), (215, 48, 39), (165, 0, 38)], dtype=torch.uint8, device=pred.device)
            variants = {"color, sample": lambda: ops.flow_color(pred, "sample"),
                        "color, fixed": lambda: ops.flow_color(pred, "fixed", FIXED_MAX),
                        "error map": lambda: ops.flow_error_map(pred, gt, None, None, ABS_THRESH, REL_THRESH),
                        "composed color, sample": lambda: composed_color(pred, table),
                        "composed color, fixed": lambda: composed_color(pred, table, FIXED_MAX),
                        "composed error map": lambda: composed_error(pred, gt, edges, colors)}
            # the two forms draw the same picture: torch's atan2 and its contracted products may move a value across an integer or an edge
            px = N * H * W
            for fused, comp in (("color, sample", "composed color, sample"), ("color, fixed", "composed color, fixed"), ("error map", "composed error map")):
                x, y = variants[fused](), variants[comp]()
                x = x[0] if isinstance(x, tuple) else x
                d = (x.to(torch.int32) - y.to(torch.int32)).abs()
                differ = int((d > 0).sum())
                assert differ <= 2e-3 * 3 * px, f"{fused}: {differ} of {3 * px} bytes differ"
                if fused != "error map":
                    assert int(d.max()) <= 1, f"{fused}: a byte differs by {int(d.max())}"
            launches = {n: count_kernels(fn) for n, fn in variants.items() if n.startswith("composed")}
            for fn in variants.values():
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            times = {n: [] for n in variants}
            for _ in range(a.repeats):
                for n, fn in variants.items():
                    times[n].append(timeit(fn, a.iters))
            beyond = float(((pred[:, 0] ** 2 + pred[:, 1] ** 2).sqrt() > FIXED_MAX).float().mean())
            lines += [f"## [{N},2,{H},{W}]: {px} pixels, {100 * beyond:.1f} % beyond the fixed radius {FIXED_MAX:g}", "",
                      "| variant | us per call, median (min .. max) | bytes moved | share of 6.3 TB/s |", "|---|---|---|---|"]
            med = {}
            for n, ts in times.items():
                moved = px * BYTES[n.replace("composed ", "")]
                med[n] = statistics.median(ts)
                lines.append("| %s | %.2f (%.2f .. %.2f) | %.2f MB | %.1f %% |" % (n, med[n], min(ts), max(ts), moved / 1e6, 100 * moved / (med[n] * 1e-6) / HBM_ROOF))
            lines.append("")
            for fused in BYTES:
                ratio = med["composed " + fused] / med[fused]
                count = launches["composed " + fused]
                lines.append("%s: composed / fused = %.1f (medians): the fused call is %s.  Device activities (kernels and copies, from torch's profiler) in "
                             "one composed call: %s (fused: %d)." % (fused, ratio, "faster" if ratio > 1 else "NOT faster: the expectation does not hold here",
                                                                     "not counted" if count is None else count, 2 if fused == "color, sample" else 1))
                assert math.isfinite(ratio)
            lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
