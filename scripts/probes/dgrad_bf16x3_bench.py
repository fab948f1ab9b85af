#!/usr/bin/env python3
"""Exact fp32 transposed-convolution route against the split-bf16 data gradient (csrc/tconv_bf16x3.hip) at conv2 and conv3 of the FlowNetC
encoders, batch 8 @448x320 (one tower: 8 samples; both towers as the training step runs them: 16), plain and with the ReLU derivative of
the layer in front folded in, in ONE process: after a warm-up of both routes (which also lets each pick its tile variant), the two are
timed alternately with device events, ROUNDS windows of LAUNCHES launches each; reported: the median and the spread of the per-launch
time, their ratio, every tile variant of the split kernel on its own, and the largest difference between the two results.

    python scripts/probes/dgrad_bf16x3_bench.py [--out profiles/dgrad_bf16x3_bench.md]

The 3x3 / 2 / 1 class of the route (conv4) was instantiated from the same template and measured once at conv4's shape (top_diff
[8,512,20,28] -> [8,256,40,56]): 335.8 us against the exact kernel's 157.7 us, ratio 2.13 (masked 2.08).  Not faster: the instantiation is
deleted, the class stays exact under the flag, and NOTE_3X3 below carries the figures into the report.
"""
import statistics

from bf16x3_probe import LAUNCHES, ROUNDS, alternate, arguments, fmt, variant_rows, write_report  # (puts the repository on sys.path)

import torch  # noqa: E402

from flownet2_amd import ops  # noqa: E402

# the layer's bottom [N, Cin, H, W] and Cout, 5x5 / 2 / 2: top_diff [N, Cout, H / 2, W / 2] -> bottom_diff [N, Cin, H, W]
LAYERS = {"conv2": (8, 64, 160, 224, 128), "conv3": (8, 128, 80, 112, 256), "conv2, both towers": (16, 64, 160, 224, 128),
          "conv3, both towers": (16, 128, 80, 112, 256)}
TCONV = 2                                   # FN2_BWD_ROUTE_TCONV
SPLIT = TCONV | ops.CONV_ARITH_BF16X3
# registers of the build (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950) and dynamic LDS per workgroup of the tile variants
SPLIT_VARIANTS = [("32x4 class positions, MW 2 NP 4", 242, 51456), ("16x8 class positions, MW 2 NP 4", 242, 58112)]


NOTE_3X3 = ("The 3x3 / 2 / 1 class of the route (conv4; conv5 and conv6 are not on this route at this size) was instantiated from the same template (5 k-steps per chunk of 16 channels: the 1 / 2 / 2 / 4 taps of the classes in pairs) and measured at conv4's shape, top_diff `[8,512,20,28] -> [8,256,40,56]`: 335.8 us against the exact kernel's 157.7 us plain (ratio 2.13), 337.7 against 162.4 masked (2.08); by tile variant 504.9 / 507.9 us (32x4 / 16x8 class positions) and 339.6 / 337.2 us (16x4 / 8x8).  A map of 20x28 class positions gives 160 - 320 workgroups of 64 channels for 512 slots, and 5 k-steps between two splits of the window do not cover them.  It is NOT faster: the instantiation is deleted and the class stays exact under the flag.")


def main():
    a = arguments("dgrad_bf16x3_bench")
    lines = ["# Data gradient of the 5x5 / 2 convolutions: exact fp32 against split-bf16 (bf16x3)", "",
             "`scripts/probes/dgrad_bf16x3_bench.py` on %s: both routes in one process, warmed up, timed alternately with device events, %d windows of "
             "%d launches each; us per launch, median (min .. max)." % (torch.cuda.get_device_name(0), ROUNDS, LAUNCHES), ""]
    table = ["| layer | form | exact fp32 (tconv_mfma) | bf16x3 (autotuned pick) | bf16x3 / exact | max abs difference | result scale |", "|---|---|---|---|---|---|---|"]
    per_variant = ["| layer | variant | VGPRs | LDS bytes / workgroup | us per launch |", "|---|---|---|---|---|"]
    verdict = []
    for name, (N, Cin, H, W, Cout) in LAYERS.items():
        d = ops.conv_desc(N, Cin, H, W, Cout, 5, 2, 2)
        assert ops.conv_backward_data_route(d, False, bf16x3=True) == SPLIT and ops.conv_backward_data_route(d, False) == TCONV
        g = torch.Generator(device="cuda").manual_seed(5)
        top = torch.randn(N, Cout, H // 2, W // 2, device="cuda", generator=g)
        w = torch.randn(Cout, Cin, 5, 5, device="cuda", generator=g) * (2.0 / (Cin * 25)) ** 0.5
        y = torch.randn(N, Cin, H, W, device="cuda", generator=g)
        packed = {r: ops.conv_backward_data_pack_weights(w, d, False, r) for r in (TCONV, SPLIT)}
        out = {}
        forms = {"plain": lambda r: out.__setitem__(r, ops.conv_backward_data(top, packed[r], d, False, r)),
                 "masked": lambda r: out.__setitem__(r, ops.conv_backward_data_masked(top, packed[r], d, False, r, y, 0.1))}
        for form, call in forms.items():
            run = {r: (lambda r=r: call(r)) for r in (TCONV, SPLIT)}
            t = alternate(run)
            med = {r: statistics.median(t[r]) for r in run}
            diff = float((out[TCONV] - out[SPLIT]).abs().max())
            scale = float(out[TCONV].abs().max())
            table.append("| %s `[%d,%d,%d,%d] -> [%d,%d,%d,%d]` | %s | %s | %s | %.3f | %.2e | %.2f |" %
                         (name, N, Cout, H // 2, W // 2, N, Cin, H, W, form, fmt(t[TCONV]), fmt(t[SPLIT]), med[SPLIT] / med[TCONV], diff, scale))
            verdict.append("%s, %s: bf16x3 is %s than the exact kernel (%.1f against %.1f us, ratio %.3f; the arithmetic floor is 6/16 x 26/25 = 0.39 of "
                           "the exact kernel's matrix time)." % (name, form, "FASTER" if med[SPLIT] < med[TCONV] else "NOT faster", med[SPLIT], med[TCONV],
                                                                med[SPLIT] / med[TCONV]))
        per_variant += variant_rows("tconv_bf16x3", name, lambda: forms["plain"](SPLIT), SPLIT_VARIANTS)
    lines += table + [""] + verdict + ["", "Tile variants of the split kernel, forced one by one (plain form, 4 windows each):", ""] + per_variant + [""]
    lines += [NOTE_3X3, ""]
    write_report(a.out, lines)


if __name__ == "__main__":
    main()
