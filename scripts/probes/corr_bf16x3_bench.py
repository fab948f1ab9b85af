#!/usr/bin/env python3
"""Exact fp32 Correlation forward (the layer's own dispatch: the unit kernel or corr_fwd_pair) against the split-bf16 kernel
(csrc/correlation_bf16x3.hip) at the three BASELINE shapes, plain and in the fused slice + ReLU form, in ONE process: after a warm-up of both
arithmetics (which also lets the split kernel pick its variant), the two are timed alternately with device events, ROUNDS windows of LAUNCHES
launches each.  Both go through fn2_correlation_forward_routed.  Reported: median and spread per launch, the ratio, every variant of the
split kernel on its own, the largest difference of the two results.

    python scripts/probes/corr_bf16x3_bench.py [--out profiles/corr_bf16x3_bench.md]
"""
import ctypes as C
import statistics

from bf16x3_probe import LAUNCHES, ROUNDS, alternate, arguments, fmt, variant_rows, write_report  # (puts the repository on sys.path)

import torch  # noqa: E402

from flownet2_amd import _lib, ops  # noqa: E402
from flownet2_amd._lib import check  # noqa: E402

SHAPES = {"A": (8, 256, 40, 56), "B": (4, 256, 48, 96), "C": (1, 256, 56, 128)}
OWN, SPLIT = ops.CORR_ROUTE_OWN, ops.CORR_ROUTE_OWN | ops.CONV_ARITH_BF16X3
TOPC, WIDE, C0 = 441, 473, 32          # the [conv_redir | corr] blob of FlowNetC: 32 + 441 channels
# patches per task, waves, registers of the build (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950), dynamic LDS per workgroup, workgroups per CU
SPLIT_VARIANTS = [("4 patches, 8 waves", 114, 86016, 1), ("2 patches, 4 waves", 150, 61440, 2)]


def main():
    a = arguments("corr_bf16x3_bench")
    L = _lib.lib()
    p = ops.corr_params(20, 1, 20, 1, 2)
    lines = ["# Correlation forward (FlowNetC instance): exact fp32 against split-bf16 (bf16x3)", "",
             "`scripts/probes/corr_bf16x3_bench.py` on %s: both arithmetics in one process, warmed up, timed alternately with device events, %d windows "
             "of %d launches each; us per launch, median (min .. max).  Both through `fn2_correlation_forward_routed`; fused = the top as channels "
             "[%d, %d) of a %d-channel blob with ReLU(0.1)." % (torch.cuda.get_device_name(0), ROUNDS, LAUNCHES, C0, C0 + TOPC, WIDE), ""]
    table = ["| shape | form | exact fp32 | bf16x3 | bf16x3 / exact | bf16x3 windows below exact | max abs difference | result scale |", "|---|---|---|---|---|---|---|---|"]
    per_variant = ["| shape | variant | VGPRs | LDS bytes / workgroup | workgroups / CU | plain, us per launch |", "|---|---|---|---|---|---|"]
    for name, (N, Cc, H, W) in SHAPES.items():
        assert int(L.fn2_correlation_route(C.byref(p), N, Cc, H, W, ops.ROUTE_BF16X3)) == SPLIT
        g = torch.Generator(device="cuda").manual_seed(5)
        b0 = torch.randn(N, Cc, H, W, device="cuda", generator=g)
        b1 = torch.randn(N, Cc, H, W, device="cuda", generator=g)
        st = ops._stream()
        run = {}
        outs = {}
        for form, (ch, c0, relu, slope) in {"plain": (TOPC, 0, 0, 0.0), "fused": (WIDE, C0, 1, 0.1)}.items():
            for r, what in ((OWN, "exact"), (SPLIT, "split")):
                top = torch.zeros((N, ch, H, W), device="cuda")
                outs[(form, what)] = top[:, c0:c0 + TOPC]

                def call(r=r, top=top, ch=ch, c0=c0, relu=relu, slope=slope):
                    check(L.fn2_correlation_forward_routed(C.byref(p), r, ops._ptr(b0), ops._ptr(b1), ops._ptr(top), N, Cc, H, W, ch, c0, relu, C.c_float(slope),
                                                           None, 0, st))
                run[(form, what)] = call
        t = alternate(run)
        torch.cuda.synchronize()
        for form in ("plain", "fused"):
            e, s = t[(form, "exact")], t[(form, "split")]
            diff = float((outs[(form, "exact")] - outs[(form, "split")]).abs().max())
            table.append("| %s `[%d,%d,%d,%d]` | %s | %s | %s | %.3f | %s | %.2e | %.2f |" % (name, N, Cc, H, W, form, fmt(e), fmt(s), statistics.median(s) / statistics.median(e),
                                                                                       "yes" if max(s) < min(e) else "NO", diff, float(outs[(form, "exact")].abs().max())))
        per_variant += variant_rows("correlation_bf16x3", name, run[("plain", "split")], SPLIT_VARIANTS)
    lines += table + ["", "Variants of the split kernel, forced one by one (4 windows each):", ""] + per_variant + [""]
    write_report(a.out, lines)


if __name__ == "__main__":
    main()
