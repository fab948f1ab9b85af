#!/usr/bin/env python3
"""Exact fp32 Winograd kernel (csrc/conv_wino.hip) against the split-bf16 Winograd kernel (csrc/conv_wino_bf16x3.hip) in ONE process: after a
warm-up of both routes (which also lets each pick its tile variant), the two are timed alternately with device events, ROUNDS windows of
LAUNCHES launches each; reported: the median and the spread of the per-launch time, their ratio, every tile variant of the split kernel on
its own, and the largest difference between the two results.

Layers: conv3_1 and conv4_1 of FlowNetC at batch 8 @448x320, and the Winograd layers of FlowNet2 at batch 4 @768x384 with the most
multiplies (profiles/r06_flownet2_kernels.md counts time per kernel variant, not per layer: FlowNetC's conv3_1, conv4_1 of the three
encoders, conv3_1 of the two FlowNetS), plus two layers of classes of their own: a 64-channel layer on a large map (FlowNet-SD's interconv2)
and a layer with fewer input channels than one k-step (the fusion net's conv0).

    python scripts/probes/wino_bf16x3_bench.py [--out profiles/wino_bf16x3_bench.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402

from flownet2_amd import _lib, ops  # noqa: E402

# [N, Cin, H, W] -> Cout, 3x3 / 1 / 1
LAYERS = {
    "C conv3_1 @8x448x320": (8, 473, 40, 56, 256), "C conv4_1 @8x448x320": (8, 512, 20, 28, 512),
    "C conv3_1 @4x768x384": (4, 473, 48, 96, 256), "C/S conv4_1 @4x768x384": (4, 512, 24, 48, 512), "S conv3_1 @4x768x384": (4, 256, 48, 96, 256),
    "SD interconv2 @4x768x384": (4, 194, 96, 192, 64), "fusion conv0 @4x768x384": (4, 11, 384, 768, 64),
}
ROUNDS, LAUNCHES = 12, 20
EXACT, SPLIT = ops.CONV_ROUTE_WINOGRAD, ops.CONV_ROUTE_WINOGRAD | ops.CONV_ARITH_BF16X3
# registers of the build (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950: arch VGPRs + accumulator VGPRs, no spills) and dynamic
# LDS per workgroup of the tile variants
SPLIT_VARIANTS = [("16x16 px x 64 channels", "256 + 256", 145408), ("8x32 px x 64 channels", "256 + 256", 124928)]


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "wino_bf16x3_bench.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wino_bf16x3_bench: needs the GPU (no fallback: a CPU time says nothing)")
    L = _lib.lib()
    lines = ["# Winograd F(2x2, 3x3) convolution: exact fp32 against split-bf16 (bf16x3)", "",
             "`scripts/probes/wino_bf16x3_bench.py` on %s: both routes in one process, warmed up, timed alternately with device events, %d windows of "
             "%d launches each; us per launch, median (min .. max)." % (torch.cuda.get_device_name(0), ROUNDS, LAUNCHES), ""]
    table = ["| layer | exact fp32 (conv_wino) | bf16x3 (cost-model / autotuned pick) | bf16x3 / exact | max abs difference | result scale |", "|---|---|---|---|---|---|"]
    per_variant = ["| layer | variant | VGPRs | LDS bytes / workgroup | us per launch |", "|---|---|---|---|---|"]
    verdict = []
    for name, (N, Cin, H, W, Cout) in LAYERS.items():
        d = ops.conv_desc(N, Cin, H, W, Cout, 3, 1, 1)
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn(N, Cin, H, W, device="cuda", generator=g)
        w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) * (2.0 / (Cin * 9)) ** 0.5
        b = torch.randn(Cout, device="cuda", generator=g) * 0.1
        out = {r: torch.empty((N, Cout, H, W), device="cuda") for r in (EXACT, SPLIT)}
        packed = {r: ops.conv_pack_weights(w, d, r) for r in (EXACT, SPLIT)}
        run = {r: (lambda r=r: ops.conv_forward(x, packed[r], b, d, r, False, True, 0.1, out=out[r])) for r in (EXACT, SPLIT)}
        for _ in range(3):                                    # warm-up: first launches, variant selection, clocks
            for r in run:
                window(run[r])
        t = {r: [] for r in run}
        for _ in range(ROUNDS):
            for r in run:
                t[r].append(window(run[r]))
        med = {r: statistics.median(t[r]) for r in run}
        diff = float((out[EXACT] - out[SPLIT]).abs().max())
        scale = float(out[EXACT].abs().max())
        fmt = lambda v: "%.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))
        table.append("| %s `[%d,%d,%d,%d] -> %d` | %s | %s | %.3f | %.2e | %.2f |" % (name, N, Cin, H, W, Cout, fmt(t[EXACT]), fmt(t[SPLIT]),
                                                                                 med[SPLIT] / med[EXACT], diff, scale))
        verdict.append("%s: bf16x3 is %s than the exact kernel (%.1f against %.1f us, ratio %.3f)."
                       % (name, "FASTER" if med[SPLIT] < med[EXACT] else "NOT faster", med[SPLIT], med[EXACT], med[SPLIT] / med[EXACT]))
        try:
            for v in range(int(L.fn2_conv_wino_bf16x3_num_variants())):
                L.fn2_debug_set_conv_wino_bf16x3_variant(v)
                window(run[SPLIT])
                tv = [window(run[SPLIT]) for _ in range(4)]
                label, vgpr, lds = SPLIT_VARIANTS[v] if v < len(SPLIT_VARIANTS) else ("variant %d" % v, "?", 0)
                per_variant.append("| %s | %d: %s | %s | %d | %s |" % (name, v, label, vgpr, lds, fmt(tv)))
        finally:
            L.fn2_debug_set_conv_wino_bf16x3_variant(-1)
    lines += table + [""] + verdict + ["", "Tile variants of the split kernel, forced one by one (4 windows each):", ""] + per_variant + [""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
