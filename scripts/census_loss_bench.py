#!/usr/bin/env python
"""Timing of the census data term (csrc/census_loss.hip: census_loss_warp + census_loss_stencil + census_loss_final forward,
census_loss_grad backward) at [8,3,320,448] (FlowNetC's training crop, batch 8) and [4,3,384,768] (a KITTI-sized crop, batch 4): both
directions, radius 3 (a 7 x 7 patch, 48 pairs per pixel), gamma 0.45, with the occlusion planes of flow_consistency (made before the timing
for every variant alike), against the same loss composed from functional.flow_warp, unfold and eager torch operations, and against the
brightness-constancy call of csrc/unsup_loss.hip for scale, on the same blobs in one process.
  fused forward                 ops.census_loss_forward with the saved planes: the ctypes call, the allocations, three launches
  fused forward + backward      functional.census_loss(...).backward(): four launches and autograd's bookkeeping
  composed forward              per direction flow_warp, the two grey planes, unfold of both over the 7 x 7 patch (49 planes each), the
                                soft ternary differences, the masked sum over the patch, the Charbonnier penalty, the masked mean
  composed forward + backward   the same under autograd, through _FlowWarp's own backward kernels
  brightness forward (+ backward)   functional.unsupervised_loss with its defaults: data AND smoothness term
Run on the GPU box:
    python scripts/census_loss_bench.py [--iters 100] [--repeats 7] [--out TABLE.md]     (the timing section of profiles/census_loss.md)
Device events around `iters` back-to-back calls, a warm-up of every variant first, the variants alternating inside every repeat.  Per
variant: the median over the repeats of the mean time per call with min .. max of the repeats, the bytes the fused passes have to move
and those bytes over the time as a share of the 6.3 TB/s a streaming kernel reaches on this chip.  Bytes per pixel, both directions,
C = 3: the warp pass reads 8 + 8 (flows) + 4 + 4 (occ) + 12 + 12 (each image once: it is one direction's own image and the other's warped
one; the taps come from the caches) = 48 and writes 2 x 3 planes = 24; the stencil pass reads them (24; the halo comes from the caches)
and writes pd (8): 104 forward.  The backward reads the planes (24), the flows (16) and the images' taps (24) and writes 16: 80.  For the
composed form and the brightness call the census figure is shown too, so that the column compares like with like."""
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
EPS, GAMMA, RADIUS, C_T, C_H, SCALE = 1e-3, 0.45, 3, 0.81, 0.1, 255.0
FWD_BYTES, BWD_BYTES = 104, 80


def composed_direction(Ia, Io, a, occ):
    """One direction of include/flownet2_hip_census_loss.h as flow_warp + unfold + torch operations -> its part of the loss (inputs
    without non-finite values)."""
    N, C, H, W = Ia.shape
    k = 2 * RADIUS + 1
    gsc = SCALE / C
    ad = a.detach()
    x2 = torch.arange(W, device=a.device, dtype=torch.float32).view(1, 1, W) + ad[:, 0]
    y2 = torch.arange(H, device=a.device, dtype=torch.float32).view(1, H, 1) + ad[:, 1]
    inside = (x2 >= 0) & (y2 >= 0) & (x2 < W) & (y2 < H)
    counted = (inside & (occ[:, 0] == 0)).float()
    defined = inside.float()
    G = Ia.sum(1) * gsc
    Wg = Fn.flow_warp(Io, a).sum(1) * gsc
    patches = lambda t: torch.nn.functional.unfold(t[:, None], k, padding=RADIUS).view(N, k * k, H, W)
    da, db = patches(G) - G[:, None], patches(Wg) - Wg[:, None]
    e = da / torch.sqrt(da * da + C_T) - db / torch.sqrt(db * db + C_T)
    s = e * e
    exists = patches(defined) * defined[:, None]                                    # the centre's own h is zero: it needs no mask
    dist = (s / (s + C_H) * exists).sum(1)
    psi = (dist * dist + EPS * EPS) ** GAMMA
    return (psi * counted).sum() / counted.sum().clamp(min=1)


def composed(img0, img1, fw, bw, occ_fw, occ_bw):
    return composed_direction(img0, img1, fw, occ_fw) + composed_direction(img1, img0, bw, occ_bw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table (the timing section of profiles/census_loss.md) to this file")
    a = ap.parse_args()
    lines = ["## Timing: the fused call against flow_warp, unfold and eager torch operations", "",
             "Written by `scripts/census_loss_bench.py` on an MI355X; all figures of this section come from one run of it.  Both directions, "
             f"radius {RADIUS}, gamma {GAMMA}, with occlusion planes.  Device events around {a.iters} back-to-back calls, every variant warmed up "
             f"first, the variants alternating inside each of {a.repeats} repeats; `median (min .. max)` over the repeats of the mean time per "
             "call.  A call includes its host side (the ctypes call or the torch dispatches, the allocations, autograd's bookkeeping).  Bytes: "
             f"what the fused passes must move -- {FWD_BYTES} B per pixel forward, {BWD_BYTES} more backward (the script's docstring has the "
             "count) -- and the same figure for the other variants.  The brightness rows are `functional.unsupervised_loss` with its defaults "
             "(data and smoothness term), for scale.", ""]
    g = torch.Generator().manual_seed(0)
    for shape in SHAPES:
        N, C, H, W = shape
        img0, img1 = make_images(shape, g)
        fw, bw = make_flows((N, 2, H, W), g)
        fw, bw = fw * 0.4, bw * 0.4
        with torch.no_grad():
            _, occ, _, _, _ = ops.flow_consistency(fw, bw)
        occ_fw, occ_bw = occ
        params = ops.census_loss_params(charbonnier=(EPS, GAMMA), radius=RADIUS, census_eps=(C_T, C_H), intensity_scale=SCALE)
        lf, lb = fw.clone().requires_grad_(True), bw.clone().requires_grad_(True)

        def fused_fb():
            lf.grad = lb.grad = None
            Fn.census_loss(img0, img1, lf, lb, occ_fw, occ_bw, charbonnier=(EPS, GAMMA), radius=RADIUS).backward()

        def composed_fb():
            lf.grad = lb.grad = None
            composed(img0, img1, lf, lb, occ_fw, occ_bw).backward()

        def composed_f():
            with torch.no_grad():
                return composed(img0, img1, fw, bw, occ_fw, occ_bw)

        def brightness_f():
            with torch.no_grad():
                return Fn.unsupervised_loss(img0, img1, fw, bw, occ_fw, occ_bw)

        def brightness_fb():
            lf.grad = lb.grad = None
            Fn.unsupervised_loss(img0, img1, lf, lb, occ_fw, occ_bw).backward()

        variants = {"fused forward": lambda: ops.census_loss_forward(img0, img1, fw, bw, occ_fw, occ_bw, params),
                    "composed forward": composed_f,
                    "brightness forward": brightness_f,
                    "fused forward + backward": fused_fb,
                    "composed forward + backward": composed_fb,
                    "brightness forward + backward": brightness_fb}
        # the forms compute the same loss and gradients (another association; these inputs have no non-finite values)
        fused_loss = float(variants["fused forward"]()[1])
        comp_loss = float(composed_f())
        assert abs(fused_loss - comp_loss) <= 1e-3 * abs(comp_loss), (fused_loss, comp_loss)
        fused_fb()
        gf = lf.grad.clone()
        composed_fb()
        gap = float((gf - lf.grad).abs().max() / lf.grad.abs().max())
        assert gap <= 1e-2, gap
        launches = {k: count_kernels(v) for k, v in variants.items()}
        for v in variants.values():
            timeit(v, 10)
        runs = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, v in variants.items():
                runs[k].append(timeit(v, a.iters))
        pixels = N * H * W
        lines += [f"### [{N},{C},{H},{W}]  (loss {fused_loss:.6f}, composed {comp_loss:.6f}; largest gradient difference between the forms {gap:.1e} of "
                  "the largest gradient)", "",
                  "| variant | us per call, median (min .. max) | launches | bytes moved | share of 6.3 TB/s |", "|---|---|---|---|---|"]
        for k, t in runs.items():
            nbytes = pixels * (FWD_BYTES if k.endswith("forward") else FWD_BYTES + BWD_BYTES)
            med = statistics.median(t)
            lines.append(f"| {k} | {med:.1f} ({min(t):.1f} .. {max(t):.1f}) | {launches[k] if launches[k] is not None else 'n/a'} | "
                         f"{nbytes / 1e6:.1f} MB | {100 * nbytes / (med * 1e-6) / HBM_ROOF:.1f} % |")
        med = {k: statistics.median(t) for k, t in runs.items()}
        lines += ["", f"Composed over fused: forward {med['composed forward'] / med['fused forward']:.2f}x, forward + backward "
                      f"{med['composed forward + backward'] / med['fused forward + backward']:.2f}x.  Fused census over the brightness call: forward "
                      f"{med['fused forward'] / med['brightness forward']:.2f}x, forward + backward "
                      f"{med['fused forward + backward'] / med['brightness forward + backward']:.2f}x.", ""]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
