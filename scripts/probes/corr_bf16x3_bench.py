#!/usr/bin/env python3
"""Exact fp32 Correlation forward (the layer's own dispatch: the unit kernel or corr_fwd_pair) against the split-bf16 kernel
(csrc/correlation_bf16x3.hip) at the three BASELINE shapes, plain and in the fused slice + ReLU form, in ONE process: after a warm-up of both
arithmetics (which also lets the split kernel pick its variant), the two are timed alternately with device events, ROUNDS windows of LAUNCHES
launches each.  Both go through fn2_correlation_forward_routed.  Reported: median and spread per launch, the ratio, every variant of the
split kernel on its own, the largest difference of the two results.

    python scripts/probes/corr_bf16x3_bench.py [--out profiles/corr_bf16x3_bench.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402

from flownet2_amd import _lib, ops  # noqa: E402
from flownet2_amd._lib import check  # noqa: E402

SHAPES = {"A": (8, 256, 40, 56), "B": (4, 256, 48, 96), "C": (1, 256, 56, 128)}
ROUNDS, LAUNCHES = 12, 20
OWN, SPLIT = ops.CORR_ROUTE_OWN, ops.CORR_ROUTE_OWN | ops.CONV_ARITH_BF16X3
TOPC, WIDE, C0 = 441, 473, 32          # the [conv_redir | corr] blob of FlowNetC: 32 + 441 channels
# patches per task, waves, registers of the build (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950), dynamic LDS per workgroup, workgroups per CU
SPLIT_VARIANTS = [("4 patches, 8 waves", 114, 86016, 1), ("2 patches, 4 waves", 150, 61440, 2)]


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "corr_bf16x3_bench.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("corr_bf16x3_bench: needs the GPU (no fallback: a CPU time says nothing)")
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
        for _ in range(3):                                    # warm-up: first launches, variant selection, clocks
            for k in run:
                window(run[k])
        t = {k: [] for k in run}
        for _ in range(ROUNDS):
            for k in run:
                t[k].append(window(run[k]))
        torch.cuda.synchronize()
        fmt = lambda v: "%.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))
        for form in ("plain", "fused"):
            e, s = t[(form, "exact")], t[(form, "split")]
            diff = float((outs[(form, "exact")] - outs[(form, "split")]).abs().max())
            table.append("| %s `[%d,%d,%d,%d]` | %s | %s | %s | %.3f | %s | %.2e | %.2f |" % (name, N, Cc, H, W, form, fmt(e), fmt(s), statistics.median(s) / statistics.median(e),
                                                                                       "yes" if max(s) < min(e) else "NO", diff, float(outs[(form, "exact")].abs().max())))
        try:
            for v in range(int(L.fn2_correlation_bf16x3_num_variants())):
                L.fn2_debug_set_correlation_bf16x3_variant(v)
                window(run[("plain", "split")])
                tv = [window(run[("plain", "split")]) for _ in range(4)]
                label, vgpr, lds, wgs = SPLIT_VARIANTS[v] if v < len(SPLIT_VARIANTS) else ("variant %d" % v, 0, 0, 0)
                per_variant.append("| %s | %d: %s | %d | %d | %d | %s |" % (name, v, label, vgpr, lds, wgs, fmt(tv)))
        finally:
            L.fn2_debug_set_correlation_bf16x3_variant(-1)
    lines += table + ["", "Variants of the split kernel, forced one by one (4 windows each):", ""] + per_variant + [""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
