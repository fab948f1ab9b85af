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
import statistics

from bf16x3_probe import LAUNCHES, ROUNDS, alternate, arguments, fmt, variant_rows, write_report  # (puts the repository on sys.path)

import torch  # noqa: E402

from flownet2_amd import ops  # noqa: E402

# [N, Cin, H, W] -> Cout, 3x3 / 1 / 1
LAYERS = {
    "C conv3_1 @8x448x320": (8, 473, 40, 56, 256), "C conv4_1 @8x448x320": (8, 512, 20, 28, 512),
    "C conv3_1 @4x768x384": (4, 473, 48, 96, 256), "C/S conv4_1 @4x768x384": (4, 512, 24, 48, 512), "S conv3_1 @4x768x384": (4, 256, 48, 96, 256),
    "SD interconv2 @4x768x384": (4, 194, 96, 192, 64), "fusion conv0 @4x768x384": (4, 11, 384, 768, 64),
}
EXACT, SPLIT = ops.CONV_ROUTE_WINOGRAD, ops.CONV_ROUTE_WINOGRAD | ops.CONV_ARITH_BF16X3
# registers of the build (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950: arch VGPRs + accumulator VGPRs, no spills) and dynamic
# LDS per workgroup of the tile variants
SPLIT_VARIANTS = [("16x16 px x 64 channels", "256 + 256", 145408), ("8x32 px x 64 channels", "256 + 256", 124928)]


def main():
    a = arguments("wino_bf16x3_bench")
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
        t = alternate(run)
        med = {r: statistics.median(t[r]) for r in run}
        diff = float((out[EXACT] - out[SPLIT]).abs().max())
        scale = float(out[EXACT].abs().max())
        table.append("| %s `[%d,%d,%d,%d] -> %d` | %s | %s | %.3f | %.2e | %.2f |" % (name, N, Cin, H, W, Cout, fmt(t[EXACT]), fmt(t[SPLIT]),
                                                                                 med[SPLIT] / med[EXACT], diff, scale))
        verdict.append("%s: bf16x3 is %s than the exact kernel (%.1f against %.1f us, ratio %.3f)."
                       % (name, "FASTER" if med[SPLIT] < med[EXACT] else "NOT faster", med[SPLIT], med[EXACT], med[SPLIT] / med[EXACT]))
        per_variant += variant_rows("conv_wino_bf16x3", name, run[SPLIT], SPLIT_VARIANTS)
    lines += table + [""] + verdict + ["", "Tile variants of the split kernel, forced one by one (4 windows each):", ""] + per_variant + [""]
    write_report(a.out, lines)


if __name__ == "__main__":
    main()
