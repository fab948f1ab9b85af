#!/usr/bin/env python
"""Timing of forward warping (csrc/flow_splat.hip: a memset, flow_splat_link + flow_splat_gather + flow_splat_final forward,
flow_splat_bwd backward) at [8,3,320,448] (FlowNetC's training crop, batch 8) and [4,3,384,768] (a KITTI-sized crop, batch 4), modes
"sum" and "softmax", on a smooth flow (flow_consistency_bench.make_flows: a few pixels of motion and an occluder) and on an i.i.d. flow
(uniform in [-8, 8]: neighbouring sources land far apart, every list is chased through cold lines), in one process:
  fused forward                 ops.flow_splat_forward (out and weight): the ctypes call, the allocations, a memset and three launches
  fused forward + backward      functional.flow_splat(...) and .backward() through out: one more launch and autograd's bookkeeping
  composed forward (+ backward) the same result from eager torch operations: floor, the four weights, index_put_(accumulate=True) per tap
                                (float atomics: neither the order nor the bits are fixed), the division; under autograd for the backward
  flow_warp image gradient      ("sum" only) ops.flow_warp_backward(propagate_image only) at the same shape: the kernel pair
                                warp_bwd_link + warp_bwd_gather that "sum" generalises
  flow_interpolate and its parts   the two flow_warp calls with the eager z planes, the two raw softmax splats, the eager blend
Run on the GPU box:
    python scripts/flow_splat_bench.py [--iters 100] [--repeats 7] [--out TABLE.md]     (the timing section of profiles/flow_splat.md)
Device events around `iters` back-to-back calls, a warm-up of every variant first, the variants alternating inside every repeat.  Per
variant: the median over the repeats of the mean time per call with min .. max of the repeats, the bytes the fused passes have to move
and those bytes over the time as a share of the 6.3 TB/s a streaming kernel reaches on this chip.  Bytes per pixel at C = 3 (DESIGN.md
section 3.20 has the count): forward 70 for "sum", 78 for "softmax"; backward 56 more for "sum", 76 more for "softmax"."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet2_amd import ops  # noqa: E402
from flownet2_amd import functional as Fn  # noqa: E402
from flow_consistency_bench import HBM_ROOF, count_kernels, make_flows, timeit  # noqa: E402
from unsup_loss_bench import make_images  # noqa: E402

SHAPES = [(8, 3, 320, 448), (4, 3, 384, 768)]
BYTES = {"sum": (70, 56), "softmax": (78, 76)}


def composed(values, flow, metric, mode):
    """flow_splat(values, flow, metric, mode=mode) from eager torch operations (t = 1; inputs without non-finite values)."""
    N, C, H, W = values.shape
    x2 = torch.arange(W, device=flow.device, dtype=torch.float32).view(1, 1, W) + flow[:, 0]
    y2 = torch.arange(H, device=flow.device, dtype=torch.float32).view(1, H, 1) + flow[:, 1]
    inside = (x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H)
    xl, yt = x2.detach().floor().clamp(0, W - 1), y2.detach().floor().clamp(0, H - 1)
    al, be = x2 - xl, y2 - yt
    xl, yt = xl.long(), yt.long()
    xr, yb = (xl + 1).clamp(max=W - 1), (yt + 1).clamp(max=H - 1)
    e = torch.exp(metric[:, 0]) if mode == "softmax" else torch.ones_like(x2)
    e = e * inside
    base = (torch.arange(N, device=flow.device) * (H * W)).view(N, 1, 1)
    num = torch.zeros((C, N * H * W), device=flow.device)
    den = torch.zeros(N * H * W, device=flow.device)
    vals = values.permute(1, 0, 2, 3).reshape(C, -1)
    chan = torch.arange(C, device=flow.device).view(C, 1)
    for yy, xx, w in ((yt, xl, (1 - al) * (1 - be)), (yt, xr, al * (1 - be)), (yb, xl, (1 - al) * be), (yb, xr, al * be)):
        idx = (base + yy * W + xx).reshape(-1)
        ws = (w * e).reshape(-1)
        num = num.index_put((chan.expand(C, idx.numel()), idx.expand(C, idx.numel())), vals * ws, accumulate=True)
        den = den.index_put((idx,), ws, accumulate=True)
    num, den = num.view(C, N, H, W).permute(1, 0, 2, 3), den.view(N, 1, H, W)
    return num if mode == "sum" else torch.where(den > 0, num / den.clamp(min=1e-30), torch.zeros_like(num))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table (the timing section of profiles/flow_splat.md) to this file")
    a = ap.parse_args()
    lines = ["## Timing: the fused call against eager torch operations and against FlowWarp's image gradient", "",
             "Written by `scripts/flow_splat_bench.py` on an MI355X; all figures of this section come from one run of it.  t = 1.  Device events "
             f"around {a.iters} back-to-back calls, every variant warmed up first, the variants alternating inside each of {a.repeats} repeats; "
             "`median (min .. max)` over the repeats of the mean time per call.  A call includes its host side (the ctypes call or the torch "
             "dispatches, the allocations, autograd's bookkeeping).  Bytes: what the fused passes must move (the script's docstring has the "
             "count) and the same figure for the other variants.", ""]
    g = torch.Generator().manual_seed(0)
    for shape in SHAPES:
        N, C, H, W = shape
        img0, img1 = make_images(shape, g)
        img0, img1 = img0 * 255, img1 * 255
        smooth, back = make_flows((N, 2, H, W), g)
        iid = ((torch.rand((N, 2, H, W), generator=g) * 16) - 8).cuda()
        metric = (-4 * torch.rand((N, 1, H, W), generator=g)).cuda()
        gout = torch.randn(shape, generator=g).cuda()
        for flow_name, flow in (("smooth flow", smooth), ("i.i.d. flow in [-8, 8]", iid)):
            lv, lf, lz = (t.clone().requires_grad_(True) for t in (img0, flow, metric))
            variants = {}
            for mode in ("sum", "softmax"):
                imp = "none" if mode == "sum" else "softmax"
                z = None if mode == "sum" else metric

                def fused_f(imp=imp, z=z, mode=mode):
                    return ops.flow_splat_forward(img0, flow, z, importance=imp, normalize=mode != "sum")

                def fused_fb(mode=mode):
                    lv.grad = lf.grad = lz.grad = None
                    Fn.flow_splat(lv, lf, lz, mode=mode).backward(gout)

                def composed_f(mode=mode):
                    with torch.no_grad():
                        return composed(img0, flow, metric, mode)

                def composed_fb(mode=mode):
                    lv.grad = lf.grad = lz.grad = None
                    composed(lv, lf, lz, mode).backward(gout)

                # the two forms compute the same thing (another order of summation)
                got, want = fused_f()[1], composed_f()
                gap = float((got - want).abs().max() / want.abs().max())
                assert gap <= 1e-4, (mode, gap)
                variants.update({f"{mode}: fused forward": fused_f, f"{mode}: composed forward": composed_f,
                                 f"{mode}: fused forward + backward": fused_fb, f"{mode}: composed forward + backward": composed_fb})
            variants["sum: flow_warp image gradient"] = lambda: ops.flow_warp_backward(img0, flow, gout, True, False)
            launches = {k: count_kernels(v) for k, v in variants.items()}
            for v in variants.values():
                timeit(v, 10)
            runs = {k: [] for k in variants}
            for _ in range(a.repeats):
                for k, v in variants.items():
                    runs[k].append(timeit(v, a.iters))
            with torch.no_grad():
                rep = Fn.flow_splat_report(img0, flow).summary()
            pixels = N * H * W
            lines += [f"### [{N},{C},{H},{W}], {flow_name}  (splatted {rep['splatted']:.3f}, holes {rep['holes']:.3f}, largest weight "
                      f"{rep['weight_max']:.2f})", "",
                      "| variant | us per call, median (min .. max) | launches | bytes moved | share of 6.3 TB/s |", "|---|---|---|---|---|"]
            med = {}
            for k, t in runs.items():
                fwd, bwd = BYTES[k.split(":")[0]]
                nbytes = pixels * (fwd + bwd if k.endswith("backward") else fwd)
                med[k] = statistics.median(t)
                lines.append(f"| {k} | {med[k]:.1f} ({min(t):.1f} .. {max(t):.1f}) | {launches[k] if launches[k] is not None else 'n/a'} | "
                             f"{nbytes / 1e6:.1f} MB | {100 * nbytes / (med[k] * 1e-6) / HBM_ROOF:.1f} % |")
            lines += ["", "Composed over fused: " + ", ".join(
                f"{mode} forward {med[mode + ': composed forward'] / med[mode + ': fused forward']:.2f}x, forward + backward "
                f"{med[mode + ': composed forward + backward'] / med[mode + ': fused forward + backward']:.2f}x" for mode in ("sum", "softmax"))
                + f".  Fused sum forward over the flow_warp image gradient: {med['sum: fused forward'] / med['sum: flow_warp image gradient']:.2f}x.", ""]
        # flow_interpolate against its parts, on the smooth pair
        t = 0.5

        def z_planes():
            with torch.no_grad():
                return (-20.0 * (img0 - Fn.flow_warp(img1, smooth)).abs().mean(dim=1, keepdim=True) / 255.0,
                        -20.0 * (img1 - Fn.flow_warp(img0, back)).abs().mean(dim=1, keepdim=True) / 255.0)
        z0, z1 = z_planes()

        def splats():
            return (ops.flow_splat_forward(img0, smooth, z0, t=t, importance="softmax"), ops.flow_splat_forward(img1, back, z1, t=1 - t, importance="softmax"))
        (_, n0, d0, _, _), (_, n1, d1, _, _) = splats()

        def blend():
            den = (1 - t) * d0 + t * d1
            return torch.where(den > 0, ((1 - t) * n0 + t * n1) / den, (1 - t) * img0 + t * img1)
        parts = {"flow_interpolate": lambda: Fn.flow_interpolate(img0, img1, smooth, back, t), "its two flow_warp calls and z planes": z_planes,
                 "its two softmax splats": splats, "its eager blend": blend}
        for v in parts.values():
            timeit(v, 10)
        runs = {k: [] for k in parts}
        for _ in range(a.repeats):
            for k, v in parts.items():
                runs[k].append(timeit(v, a.iters))
        lines += [f"### [{N},{C},{H},{W}], flow_interpolate at t = 0.5 on the smooth pair", "", "| part | us per call, median (min .. max) | launches |",
                  "|---|---|---|"]
        for k, tt in runs.items():
            n = count_kernels(parts[k])
            lines.append(f"| {k} | {statistics.median(tt):.1f} ({min(tt):.1f} .. {max(tt):.1f}) | {n if n is not None else 'n/a'} |")
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
