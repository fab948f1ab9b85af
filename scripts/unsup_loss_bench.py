#!/usr/bin/env python
"""Timing of the unsupervised loss (csrc/unsup_loss.hip: unsup_loss_partial + unsup_loss_final forward, unsup_loss_grad backward) at
[8,3,320,448] (FlowNetC's training crop, batch 8) and [4,3,384,768] (a KITTI-sized crop, batch 4): both directions, second-order
smoothness, edge weight 10, gamma 0.45, with the occlusion planes of flow_consistency (made before the timing for every variant alike),
against the same loss composed from functional.flow_warp and eager torch operations, on the same blobs in one process.
  fused forward              ops.unsup_loss_forward: the ctypes call, the allocations, two launches
  fused forward + backward   functional.unsupervised_loss(...).backward(): three launches and autograd's bookkeeping
  composed forward           per direction flow_warp, the Charbonnier penalty, the masked mean, the second differences of the flow along
                             both axes, the edge weights from the image differences, the mean of the weighted terms
  composed forward + backward   the same under autograd, through _FlowWarp's own backward kernels
Run on the GPU box:
    python scripts/unsup_loss_bench.py [--iters 100] [--repeats 7] [--out TABLE.md]     (the timing section of profiles/unsup_loss.md)
Device events around `iters` back-to-back calls, a warm-up of every variant first, the variants alternating inside every repeat.  Per
variant: the median over the repeats of the mean time per call with min .. max of the repeats, the bytes the fused pass has to move and
those bytes over the time as a share of the 6.3 TB/s a streaming kernel reaches on this chip.  Bytes per pixel, both directions, C = 3:
forward 8 (fw) + 8 (bw) + 4 + 4 (occ) + 12 + 12 (each image once: it is one direction's own image and the other's warped one, and the
neighbours and taps come from the caches) = 48 read; backward the same 48 read and 16 written.  For the composed form the same figure
is the LEAST it could move."""
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

SHAPES = [(8, 3, 320, 448), (4, 3, 384, 768)]
EPS, GAMMA, EDGE = 1e-3, 0.45, 10.0
READ_BYTES, WRITE_BYTES = 48, 16


def make_images(shape, g):
    N, C, H, W = shape
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    img = torch.full(shape, 0.5)
    for n in range(N):
        for c in range(C):
            for _ in range(4):
                amp, fx, fy, ph = (torch.rand((), generator=g).item() for _ in range(4))
                img[n, c] += 0.12 * amp * torch.sin((0.02 + 0.2 * fx) * x + (0.02 + 0.2 * fy) * y + 6.28 * ph)
    return img.cuda(), torch.roll(img, (1, 2), (2, 3)).cuda()


def composed_direction(Ia, Io, a, occ):
    """One direction of include/flownet2_hip_unsup_loss.h (order 2) as flow_warp + torch operations -> its part of the loss."""
    N, C, H, W = Ia.shape
    psi = lambda t: (t * t + EPS * EPS) ** GAMMA
    ad = a.detach()
    x2 = torch.arange(W, device=a.device, dtype=torch.float32).view(1, 1, W) + ad[:, 0]
    y2 = torch.arange(H, device=a.device, dtype=torch.float32).view(1, H, 1) + ad[:, 1]
    mask = ((x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H) & (occ[:, 0] == 0)).float()
    data = (psi(Ia - Fn.flow_warp(Io, a)).sum(1) * mask).sum() / mask.sum().clamp(min=1)
    sx = (a[:, :, :, :-2] - 2 * a[:, :, :, 1:-1]) + a[:, :, :, 2:]
    sy = (a[:, :, :-2] - 2 * a[:, :, 1:-1]) + a[:, :, 2:]
    wx = torch.exp(-EDGE * (Ia[:, :, :, 2:] - Ia[:, :, :, :-2]).abs().mean(1))
    wy = torch.exp(-EDGE * (Ia[:, :, 2:] - Ia[:, :, :-2]).abs().mean(1))
    smooth = ((wx * psi(sx).sum(1)).sum() + (wy * psi(sy).sum(1)).sum()) / (wx.numel() + wy.numel())
    return data + smooth


def composed(img0, img1, fw, bw, occ_fw, occ_bw):
    return composed_direction(img0, img1, fw, occ_fw) + composed_direction(img1, img0, bw, occ_bw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table (the timing section of profiles/unsup_loss.md) to this file")
    a = ap.parse_args()
    lines = ["## Timing: the fused call against flow_warp plus eager torch operations", "",
             "Written by `scripts/unsup_loss_bench.py` on an MI355X; all figures of this section come from one run of it.  Both directions, "
             f"second-order smoothness, gamma {GAMMA}, edge weight {EDGE:g}, with occlusion planes.  Device events around {a.iters} back-to-back "
             f"calls, every variant warmed up first, the variants alternating inside each of {a.repeats} repeats; `median (min .. max)` over the "
             "repeats of the mean time per call.  A call includes its host side (the ctypes call or the torch dispatches, the allocations, "
             f"autograd's bookkeeping).  Bytes: what the fused pass must move -- {READ_BYTES} B per pixel read forward, {READ_BYTES} read and "
             f"{WRITE_BYTES} written backward -- and for the composed form the same figure, the least it could move.", ""]
    g = torch.Generator().manual_seed(0)
    for shape in SHAPES:
        N, C, H, W = shape
        img0, img1 = make_images(shape, g)
        fw, bw = make_flows((N, 2, H, W), g)
        fw, bw = fw * 0.4, bw * 0.4
        with torch.no_grad():
            _, occ, _, _, _ = ops.flow_consistency(fw, bw)
        occ_fw, occ_bw = occ
        params = ops.unsup_loss_params(charbonnier=(EPS, GAMMA), smooth_charbonnier=(EPS, GAMMA), edge_weight=EDGE, smooth_order=2)
        lf, lb = fw.clone().requires_grad_(True), bw.clone().requires_grad_(True)

        def fused_fb():
            lf.grad = lb.grad = None
            Fn.unsupervised_loss(img0, img1, lf, lb, occ_fw, occ_bw, charbonnier=(EPS, GAMMA), smooth_charbonnier=(EPS, GAMMA), edge_weight=EDGE).backward()

        def composed_fb():
            lf.grad = lb.grad = None
            composed(img0, img1, lf, lb, occ_fw, occ_bw).backward()

        def composed_f():
            with torch.no_grad():
                return composed(img0, img1, fw, bw, occ_fw, occ_bw)

        variants = {"fused forward": lambda: ops.unsup_loss_forward(img0, img1, fw, bw, occ_fw, occ_bw, params),
                    "composed forward": composed_f,
                    "fused forward + backward": fused_fb,
                    "composed forward + backward": composed_fb}
        # the forms compute the same loss and gradients (another association, and the composed form treats non-finite values otherwise:
        # these inputs have none)
        fused_loss = float(variants["fused forward"]()[1])
        comp_loss = float(composed_f())
        assert abs(fused_loss - comp_loss) <= 1e-4 * abs(comp_loss), (fused_loss, comp_loss)
        fused_fb()
        gf = lf.grad.clone()
        composed_fb()
        gap = float((gf - lf.grad).abs().max() / lf.grad.abs().max())
        assert gap <= 1e-3, gap
        launches = {k: count_kernels(v) for k, v in variants.items()}
        for v in variants.values():
            timeit(v, 10)
        runs = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, v in variants.items():
                runs[k].append(timeit(v, a.iters))
        pixels = N * H * W
        lines += [f"### [{N},{C},{H},{W}]  (loss {fused_loss:.6f}; largest gradient difference between the forms {gap:.1e} of the largest gradient)", "",
                  "| variant | us per call, median (min .. max) | launches | bytes moved | share of 6.3 TB/s |", "|---|---|---|---|---|"]
        for k, t in runs.items():
            nbytes = pixels * (READ_BYTES if k.endswith("forward") else 2 * READ_BYTES + WRITE_BYTES)
            med = statistics.median(t)
            lines.append(f"| {k} | {med:.1f} ({min(t):.1f} .. {max(t):.1f}) | {launches[k] if launches[k] is not None else 'n/a'} | "
                         f"{nbytes / 1e6:.1f} MB | {100 * nbytes / (med * 1e-6) / HBM_ROOF:.1f} % |")
        ratio_f = statistics.median(runs["composed forward"]) / statistics.median(runs["fused forward"])
        ratio_fb = statistics.median(runs["composed forward + backward"]) / statistics.median(runs["fused forward + backward"])
        lines += ["", f"Composed over fused: forward {ratio_f:.2f}x, forward + backward {ratio_fb:.2f}x.", ""]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
