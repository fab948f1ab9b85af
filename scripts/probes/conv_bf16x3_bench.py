#!/usr/bin/env python3
"""Exact fp32 direct kernel against the split-bf16 kernel (csrc/conv_bf16x3.hip) at conv2 and conv3 of the FlowNetC encoders, batch 8 @448x320
(16 samples: both towers), in ONE process: after a warm-up of both routes (which also lets each pick its tile variant), the two are timed
alternately with device events, ROUNDS windows of LAUNCHES launches each; reported: the median and the spread of the per-launch time, their
ratio, every tile variant of the split kernel on its own, and the largest difference between the two results.

    python scripts/probes/conv_bf16x3_bench.py [--out profiles/conv_bf16x3_bench.md]
"""
import statistics

from bf16x3_probe import LAUNCHES, ROUNDS, alternate, arguments, fmt, variant_rows, write_report  # (puts the repository on sys.path)

import torch  # noqa: E402

from flownet2_amd import ops  # noqa: E402

LAYERS = {"conv2": (16, 64, 160, 224, 128), "conv3": (16, 128, 80, 112, 256)}          # [N, Cin, H, W] -> Cout, 5x5 / 2 / 2
DIRECT, SPLIT = ops.CONV_ROUTE_DIRECT, ops.CONV_ROUTE_DIRECT | ops.CONV_ARITH_BF16X3
# registers of the build (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950) and dynamic LDS per workgroup of the tile variants
SPLIT_VARIANTS = [("32x4 px, MW 2 NP 4", 124, 70848), ("16x8 px, MW 2 NP 4", 126, 72896)]


def main():
    a = arguments("conv_bf16x3_bench")
    lines = ["# Direct 5x5 / 2 convolution: exact fp32 against split-bf16 (bf16x3)", "",
             "`scripts/probes/conv_bf16x3_bench.py` on %s: both routes in one process, warmed up, timed alternately with device events, %d windows of "
             "%d launches each; us per launch, median (min .. max)." % (torch.cuda.get_device_name(0), ROUNDS, LAUNCHES), ""]
    table = ["| layer | exact fp32 (conv_mfma) | bf16x3 (autotuned pick) | bf16x3 / exact | max abs difference | result scale |", "|---|---|---|---|---|---|"]
    per_variant = ["| layer | variant | VGPRs | LDS bytes / workgroup | us per launch |", "|---|---|---|---|---|"]
    verdict = []
    for name, (N, Cin, H, W, Cout) in LAYERS.items():
        d = ops.conv_desc(N, Cin, H, W, Cout, 5, 2, 2)
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn(N, Cin, H, W, device="cuda", generator=g)
        w = torch.randn(Cout, Cin, 5, 5, device="cuda", generator=g) * (2.0 / (Cin * 25)) ** 0.5
        b = torch.randn(Cout, device="cuda", generator=g) * 0.1
        out = {r: torch.empty((N, Cout, H // 2, W // 2), device="cuda") for r in (DIRECT, SPLIT)}
        packed = {r: ops.conv_pack_weights(w, d, r) for r in (DIRECT, SPLIT)}
        run = {r: (lambda r=r: ops.conv_forward(x, packed[r], b, d, r, False, True, 0.1, out=out[r])) for r in (DIRECT, SPLIT)}
        t = alternate(run)
        med = {r: statistics.median(t[r]) for r in run}
        diff = float((out[DIRECT] - out[SPLIT]).abs().max())
        scale = float(out[DIRECT].abs().max())
        table.append("| %s `[%d,%d,%d,%d] -> %d` | %s | %s | %.3f | %.2e | %.2f |" % (name, N, Cin, H, W, Cout, fmt(t[DIRECT]), fmt(t[SPLIT]),
                                                                                 med[SPLIT] / med[DIRECT], diff, scale))
        verdict.append("%s: bf16x3 is %s than the exact kernel (%.1f against %.1f us, ratio %.3f; the arithmetic floor is 6/16 x 28/25 = 0.42 of the "
                       "exact kernel's matrix time)." % (name, "FASTER" if med[SPLIT] < med[DIRECT] else "NOT faster", med[SPLIT], med[DIRECT], med[SPLIT] / med[DIRECT]))
        per_variant += variant_rows("conv_bf16x3", name, run[SPLIT], SPLIT_VARIANTS)
    lines += table + [""] + verdict + ["", "Tile variants of the split kernel, forced one by one (4 windows each):", ""] + per_variant + [""]
    write_report(a.out, lines)


if __name__ == "__main__":
    main()
