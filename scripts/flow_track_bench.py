#!/usr/bin/env python
"""Timing of the point tracker (csrc/flow_track.hip: flow_track_gather + flow_track_final) on the dense pixel grid, at [8,T,2,320,448]
(FlowNetC's training crop, batch 8) and [4,T,2,384,768] (a KITTI-sized crop, batch 4) for T = 1 and T = 8, against the same tracking
composed by hand, on the same blobs in one process.  Inputs: per frame a smooth random flow of a few pixels, the backward flow near the
negative of the forward one, a pasted rectangle (the occluder) that moves differently in the forward flow; the stop planes are the
flags_fw of ops.flow_consistency on every frame, computed before the timing for every variant alike (their cost is its own line).
  fused              ops.flow_track with the trajectories written: the ctypes call, the allocations, two launches for all T frames
  fused, no tracks   the same without the [N,T+1,2,P] trajectories
  T calls of T = 1   (T = 8 only) eight calls over one frame each, carrying points and state: what a streaming user runs
  composed           per frame: functional.flow_warp of the forward flow by the displacement so far, flow_warp of the backward flow by the
                     new displacement, the finite / inside / consistency tests and a nearest-pixel gather of the stop plane as eager
                     torch operations, the displacement and the state updated under a mask
  flags              T calls of ops.flow_consistency(flags=True): what produces the stop planes (not part of any line above)
Run on the GPU box:
    python scripts/flow_track_bench.py [--iters 100] [--repeats 5] [--out profiles/flow_track.md]
Device events around `iters` back-to-back calls, a warm-up of every variant first, the variants alternating inside every repeat.  Per
variant: the median over the repeats of the mean time per call with min .. max of the repeats, the bytes the fused pass has to move and
those bytes over the time as a share of the 6.3 TB/s a streaming kernel reaches on this chip.  Bytes per point: per frame 8 (fw) + 8 (bw)
+ 1 (stop) read -- on the grid neighbouring points share their taps, which come from the caches -- and 8 written with the trajectories;
per call 8 (points) read, 8 (points_out) + 1 (state) + 4 (steps) written, and 8 for the trajectories' first frame.  For the other forms
the same figure is the LEAST they could move."""
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
from flow_consistency_bench import HBM_ROOF, count_kernels, timeit  # noqa: E402

PLANES = [(8, 320, 448), (4, 384, 768)]
FRAMES = (1, 8)
ALPHA = (0.01, 0.5)
BOUNDARY = 8


def make_sequence(N, T, H, W, g):
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    fw = torch.empty((N, T, 2, H, W))
    for n in range(N):
        for t in range(T):
            for c in range(2):
                amp, fx, fy, p0, p1, off = (torch.rand((), generator=g).item() for _ in range(6))
                fw[n, t, c] = (0.5 + 2 * amp) * torch.sin((0.005 + 0.02 * fx) * x + 6.28 * p0) * torch.cos((0.005 + 0.02 * fy) * y + 6.28 * p1) + 2 * off - 1
    bw = -fw + 0.05 * torch.randn(fw.shape, generator=g)
    fw[:, :, 0, H // 4:H // 4 + H // 3, W // 4:W // 4 + W // 3] += 9.0        # the occluder
    fw[:, :, 1, H // 4:H // 4 + H // 3, W // 4:W // 4 + W // 3] -= 6.0
    return fw.cuda(), bw.cuda()


def composed(fw, bw, stop):
    """The tracker of include/flownet2_hip_flow_track.h on the dense grid as flow_warp + torch operations -> (displacement [N,2,H,W],
    state uint8 [N,H,W])."""
    N, T, _, H, W = fw.shape
    dev = fw.device
    gx = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    gy = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    disp = torch.zeros((N, 2, H, W), device=dev)
    state = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    batch = torch.arange(N, device=dev).view(N, 1, 1)
    for t in range(T):
        live = state == 0
        a = Fn.flow_warp(fw[:, t].contiguous(), disp, ops.FILL_NAN)                         # fw[t] at grid + disp
        au, av = a[:, 0], a[:, 1]
        bad_a = live & ~((au.abs() <= 1e9) & (av.abs() <= 1e9))
        jx = (gx + disp[:, 0] + 0.5).long().clamp(0, W - 1)
        jy = (gy + disp[:, 1] + 0.5).long().clamp(0, H - 1)
        marked = live & ~bad_a & ((stop[:, t, 0][batch, jy, jx] & BOUNDARY) != 0)
        moved = disp + torch.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0)
        x2, y2 = gx + moved[:, 0], gy + moved[:, 1]
        go = live & ~bad_a & ~marked
        outside = go & ~((x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H))
        go = go & ~outside
        b = Fn.flow_warp(bw[:, t].contiguous(), moved, ops.FILL_NAN)                       # bw[t] at the target
        bu, bv = b[:, 0], b[:, 1]
        bad_b = go & ~((bu.abs() <= 1e9) & (bv.abs() <= 1e9))
        go = go & ~bad_b
        su, sv = au + bu, av + bv
        s = su * su + sv * sv
        m = (au * au + av * av) + (bu * bu + bv * bv)
        inconsistent = go & (s > ALPHA[0] * m + ALPHA[1])
        go = go & ~inconsistent
        state = torch.where(bad_a | bad_b, 1, torch.where(marked, 8, torch.where(outside, 2, torch.where(inconsistent, 4, state)))).to(torch.uint8)
        disp = torch.where(go.unsqueeze(1), moved, disp)
    return disp, state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_track.md"))
    a = ap.parse_args()
    lines = ["# Point trajectories: one gather launch for T frames against T calls and against flow_warp plus eager torch operations", "",
             "Written by `scripts/flow_track_bench.py` on an MI355X; all figures of this file come from one run of it.  The dense pixel grid "
             "(P = H W points per sample) tracked through T frames.  Device events "
             f"around {a.iters} back-to-back calls, every variant warmed up first, the variants alternating inside each of {a.repeats} repeats; "
             "`median (min .. max)` over the repeats of the mean time per call.  A call includes its host side (the ctypes call or the torch "
             "dispatches, the output allocations).  Bytes: what the fused pass must move -- per point and frame 17 B read (fw, bw, the stop "
             "byte; neighbouring points share their taps, which come from the caches) and 8 written with the trajectories, per point and "
             "call 8 read and 13 written (21 with the trajectories' first frame) -- and for the other forms the same figure, the least they "
             "could move.  The stop planes (flags_fw of flow_consistency on every frame) are made before the timing for every variant "
             "alike; the `flags` line is what making them costs.", ""]
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for N, H, W in PLANES:
            for T in FRAMES:
                fw, bw = make_sequence(N, T, H, W, g)
                make_flags = lambda: torch.stack([ops.flow_consistency(fw[:, t].contiguous(), bw[:, t].contiguous(), flags=True)[2][0] for t in range(T)], 1)
                stop = make_flags().contiguous()
                grid = Fn.flow_track_grid(N, H, W, 1)
                P = H * W

                def chained():
                    points, state = grid, None
                    for t in range(T):
                        _, _, points, state, _ = ops.flow_track(fw[:, t:t + 1], bw[:, t:t + 1], points, state=state, stop=stop[:, t:t + 1], alpha=ALPHA, tracks=False)
                    return points, state

                variants = {"fused": lambda: ops.flow_track(fw, bw, grid, stop=stop, alpha=ALPHA),
                            "fused, no tracks": lambda: ops.flow_track(fw, bw, grid, stop=stop, alpha=ALPHA, tracks=False)}
                if T > 1:
                    variants[f"{T} calls of T = 1"] = chained
                variants["composed"] = lambda: composed(fw, bw, stop)
                variants["flags"] = make_flags
                # the forms compute the same thing: T calls to the bit; flow_warp contracts its products, so a point on a threshold may fall
                # either way in the composed form, and whoever samples near it afterwards follows
                results, _, p_out, s_out, _ = ops.flow_track(fw, bw, grid, stop=stop, alpha=ALPHA)
                cp, cs = chained()
                assert torch.equal(cs, s_out) and torch.equal(cp.view(torch.int32), p_out.view(torch.int32)), "T calls differ from one"
                disp, state = composed(fw, bw, stop)
                differ = int((state.view(N, P) != s_out).sum())
                assert differ <= 2e-3 * N * P, f"{differ} of {N * P} states differ between the composed and the fused form"
                same = (state.view(N, P) == 0) & (s_out == 0)
                gap = ((disp.view(N, 2, P) + grid - p_out).abs().amax(1))[same].max().item()
                assert gap <= 1e-2, gap
                launches = count_kernels(lambda: composed(fw, bw, stop))
                for fn in variants.values():
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                times = {n: [] for n in variants}
                for _ in range(a.repeats):
                    for n, fn in variants.items():
                        times[n].append(timeit(fn, a.iters))
                alive = float(results[N, 1] / results[N, 0])
                lines += [f"## [{N},{T},2,{H},{W}]: {N * P} points, {T} frame{'s' if T > 1 else ''}, {100 * alive:.1f} % alive at the end", "",
                          "| variant | us per call, median (min .. max) | bytes moved | share of 6.3 TB/s |", "|---|---|---|---|"]
                med = {}
                for n, ts in times.items():
                    med[n] = statistics.median(ts)
                    if n == "flags":
                        lines.append("| %s | %.2f (%.2f .. %.2f) | | |" % (n, med[n], min(ts), max(ts)))
                        continue
                    with_tracks = n == "fused"
                    moved = N * P * (T * (17 + (8 if with_tracks else 0)) + 21 + (8 if with_tracks else 0))
                    lines.append("| %s | %.2f (%.2f .. %.2f) | %.2f MB | %.1f %% |" % (n, med[n], min(ts), max(ts), moved / 1e6, 100 * moved / (med[n] * 1e-6) / HBM_ROOF))
                ratio = med["composed"] / med["fused"]
                text = "composed / fused = %.1f (medians): the fused call is %s.  " % (ratio, "faster" if ratio > 1 else "NOT faster: the expectation does not hold here")
                if T > 1:
                    r2 = med[f"{T} calls of T = 1"] / med["fused, no tracks"]
                    text += "%d calls of T = 1 / one call without tracks = %.2f: one call over the window is %s.  " % (T, r2, "faster" if r2 > 1 else "NOT faster")
                    assert math.isfinite(r2)
                text += "Device activities (kernels and copies, from torch's profiler) in one composed call: %s (fused: 2).  " % ("not counted" if launches is None else launches)
                text += "%d of %d states differ between the composed and the fused form (flow_warp contracts its products)." % (differ, N * P)
                lines += ["", text, ""]
                assert math.isfinite(ratio)
                del fw, bw, stop
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
