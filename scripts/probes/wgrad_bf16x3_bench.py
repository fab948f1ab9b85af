#!/usr/bin/env python3
"""Exact fp32 weight gradient (csrc/conv_wgrad.hip) against the split-bf16 one (csrc/conv_wgrad_bf16x3.hip) at conv2 and conv3 of the
FlowNetC encoders, batch 8 @448x320 (both towers as the training step runs them: 16 samples; one tower: 8), in ONE process: after a
warm-up of both, the two are timed alternately with device events, ROUNDS windows of LAUNCHES calls each.  A call is the K-part kernel
plus the finalize pass (the same finalize kernels for both arithmetics); reported: the median and the spread of the per-call time, their
ratio, every tile variant of the split kernel on its own, and error / bound of both against the float64 reference of one weight slice.

    python scripts/probes/wgrad_bf16x3_bench.py [--out profiles/wgrad_bf16x3_bench.md] [--rounds 12]

The kernels' own times (K-part kernel and finalize apart) come from a kernel trace of this script in a run of its own
(--rounds 2 under a profiler); profiles/wgrad_bf16x3_bench.md carries them beside the table this script writes.
"""
import ctypes as C
import statistics

from bf16x3_probe import LAUNCHES, alternate, arguments, fmt, variant_rows, write_report  # (puts the repository on sys.path)

import torch  # noqa: E402

from flownet2_amd import _lib, ops  # noqa: E402

# the layer's bottom [N, Cin, H, W] and Cout, 5x5 / 2 / 2: a = top_diff [N, Cout, H / 2, W / 2], b = bottom
LAYERS = {"conv2, both towers": (16, 64, 160, 224, 128), "conv3, both towers": (16, 128, 80, 112, 256), "conv2": (8, 64, 160, 224, 128),
          "conv3": (8, 128, 80, 112, 256)}
# registers of the build (hipcc -O3 --save-temps, gfx950: VGPRs + AGPRs) and dynamic LDS per workgroup of the tile variants
SPLIT_VARIANTS = [("64 x 32 channels, MA 2", "168 + 200", 107008), ("32 x 32 channels, MA 1", "156 + 100", 96768)]


def main():
    a = arguments("wgrad_bf16x3_bench", rounds=True)
    L = _lib.lib()
    lines = ["# Weight gradient of the 5x5 / 2 convolutions: exact fp32 against split-bf16 (bf16x3)", "",
             "`scripts/probes/wgrad_bf16x3_bench.py` on %s: both kernels in one process, warmed up, timed alternately with device events, %d windows of "
             "%d calls each (a call = K-part kernel + finalize pass); us per call, median (min .. max)." % (torch.cuda.get_device_name(0), a.rounds, LAUNCHES), ""]
    table = ["| layer | K parts (exact / bf16x3) | exact fp32 (conv_wgrad) | bf16x3 | bf16x3 / exact | TFLOP/s exact / bf16x3 | error / bound exact / bf16x3 |",
             "|---|---|---|---|---|---|---|"]
    per_variant = ["| layer | variant | VGPRs + AGPRs | LDS bytes / workgroup | us per call |", "|---|---|---|---|---|"]
    verdict = []
    for name, (N, Cin, H, W, Cout) in LAYERS.items():
        d = ops.conv_desc(N, Cin, H, W, Cout, 5, 2, 2)
        assert ops.conv_backward_weights_arith(d, False, bf16x3=True) == ops.CONV_ARITH_BF16X3 and ops.conv_backward_weights_arith(d, False) == 0
        Ht, Wt = H // 2, W // 2
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn(N, Cin, H, W, device="cuda", generator=g)
        top = torch.randn(N, Cout, Ht, Wt, device="cuda", generator=g)
        dw = {False: torch.empty(Cout, Cin, 5, 5, device="cuda"), True: torch.empty(Cout, Cin, 5, 5, device="cuda")}
        run = {s: (lambda s=s: ops.conv_backward_weights(x, top, d, False, out=dw[s], bf16x3=s)) for s in (False, True)}
        t = alternate(run, a.rounds)
        med = {s: statistics.median(t[s]) for s in run}
        flops = 2.0 * N * Ht * Wt * Cout * Cin * 25
        # float64 reference of the gradients of 4 x 4 channel pairs, on the device
        ref = torch.ops.aten.convolution_backward(top[:, :4].double(), x[:, :4].double(), torch.zeros(4, 4, 5, 5, dtype=torch.float64, device="cuda"), None,
                                                  [2, 2], [2, 2], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        bound = 2e-6 * max(1.0, float(ref.abs().max())) * (N * Ht * Wt) ** 0.5
        err = {s: float((dw[s][:4, :4].double() - ref).abs().max()) / bound for s in run}
        ks = (int(ops.conv_wgrad_ksplit(N, Cout, Ht, Wt, Cin, H, W, 5, 2, 2)), int(L.fn2_conv_wgrad_bf16x3_ksplit(C.byref(d), 0)))
        table.append("| %s a `[%d,%d,%d,%d]` b `[%d,%d,%d,%d]` | %d / %d | %s | %s | %.3f | %.1f / %.1f | %.3f / %.3f |" %
                     (name, N, Cout, Ht, Wt, N, Cin, H, W, ks[0], ks[1], fmt(t[False]), fmt(t[True]), med[True] / med[False], flops / med[False] / 1e6,
                      flops / med[True] / 1e6, err[False], err[True]))
        verdict.append("%s: bf16x3 is %s than the exact kernel (%.1f against %.1f us per call, ratio %.3f)." %
                       (name, "FASTER" if med[True] < med[False] else "NOT faster", med[True], med[False], med[True] / med[False]))
        per_variant += variant_rows("conv_wgrad_bf16x3", name, run[True], SPLIT_VARIANTS, min(4, a.rounds))
    lines += table + [""] + verdict + ["", "Tile variants of the split kernel, forced one by one (up to 4 windows each); one workgroup of 4 waves per CU (by LDS) for both:", ""]
    lines += per_variant + [""]
    write_report(a.out, lines)


if __name__ == "__main__":
    main()
