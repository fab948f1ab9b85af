#!/usr/bin/env python3
"""Exact fp32 GEMM route of the Deconvolution{4, 2, 1} against the split-bf16 GEMM (csrc/deconv_bf16x3.hip) at deconv4 / deconv3 / deconv2
of FlowNetC, batch 8 @448x320, in ONE process: after a warm-up of both arithmetics (which also lets each kernel pick its tile variant), the
two are timed alternately with device events, ROUNDS windows of LAUNCHES launches each.  Timed: fn2_deconv_forward whole (GEMM + col2im +
bias + ReLU) in both arithmetics; the second pass alone (fn2_col2im_bias_relu_forward_into, the same launch in both); the exact GEMM launch
alone (fn2_conv_mfma_forward on the route's operand, as the dispatcher calls it).  The split GEMM's entry point is internal to the library:
its time alone is the whole call minus the second pass, and the exact GEMM is given both ways so that the subtraction can be judged.
Reported: median and spread per launch, the ratios, every tile variant of the split kernel on its own, the largest difference of the results.

    python scripts/probes/deconv_bf16x3_bench.py [--out profiles/deconv_bf16x3_bench.md]
"""
import ctypes as C
import statistics

from bf16x3_probe import LAUNCHES, ROUNDS, alternate, arguments, fmt, variant_rows, write_report  # (puts the repository on sys.path)

import torch  # noqa: E402

from flownet2_amd import _lib, ops  # noqa: E402
from flownet2_amd._lib import check  # noqa: E402

LAYERS = {"deconv4": (8, 1026, 10, 14, 256), "deconv3": (8, 770, 20, 28, 128), "deconv2": (8, 386, 40, 56, 64)}      # [N, Cin, H, W] -> Cout
GEMM, SPLIT = ops.DECONV_ROUTE_GEMM, ops.DECONV_ROUTE_GEMM | ops.CONV_ARITH_BF16X3
# rows x pixels of the workgroup tile, channels per chunk, registers of the build (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950),
# dynamic LDS per workgroup, workgroups per CU
SPLIT_VARIANTS = [("128x128, 64 ch", 236, 49344, 2), ("64x128, 64 ch", 158, 49344, 3), ("128x64, 128 ch", 160, 49536, 3)]


def main():
    a = arguments("deconv_bf16x3_bench")
    L = _lib.lib()
    lines = ["# Deconvolution 4x4 / 2 by GEMM + col2im: exact fp32 against split-bf16 (bf16x3) in the GEMM", "",
             "`scripts/probes/deconv_bf16x3_bench.py` on %s: both arithmetics in one process, warmed up, timed alternately with device events, %d windows "
             "of %d launches each; us per launch, median (min .. max).  Whole call = `fn2_deconv_forward` (GEMM + col2im + bias + ReLU); the exact GEMM "
             "alone is its own launch, the split GEMM alone is the whole call minus the second pass (the same launch in both arithmetics)."
             % (torch.cuda.get_device_name(0), ROUNDS, LAUNCHES), ""]
    table = ["| layer | whole call, exact fp32 | whole call, bf16x3 | bf16x3 / exact | windows apart | max abs difference | result scale |", "|---|---|---|---|---|---|---|"]
    parts = ["| layer | col2im + bias + ReLU alone | exact GEMM alone | exact GEMM = whole - second pass | bf16x3 GEMM = whole - second pass | GEMM bf16x3 / exact |",
             "|---|---|---|---|---|---|"]
    per_variant = ["| layer | variant | VGPRs | LDS bytes / workgroup | workgroups / CU | whole call, us per launch |", "|---|---|---|---|---|---|"]
    verdict = []
    for name, (N, Cin, H, W, Cout) in LAYERS.items():
        d = ops.conv_desc(N, Cin, H, W, Cout, 4, 2, 1)
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn(N, Cin, H, W, device="cuda", generator=g)
        w = torch.randn(Cin, Cout, 4, 4, device="cuda", generator=g) * (2.0 / (Cin * 4)) ** 0.5
        b = torch.randn(Cout, device="cuda", generator=g) * 0.1
        need = int(L.fn2_deconv_workspace_bytes(C.byref(d), GEMM))
        assert need == int(L.fn2_deconv_workspace_bytes(C.byref(d), SPLIT))
        ws = torch.empty(need // 4, device="cuda")
        out = {r: torch.empty((N, Cout, 2 * H, 2 * W), device="cuda") for r in (GEMM, SPLIT)}
        packed = {r: ops.conv_pack_weights(w, d, r, True) for r in (GEMM, SPLIT)}
        st = ops._stream()

        def whole(r):
            check(L.fn2_deconv_forward(C.byref(d), r, ops._ptr(x), Cin, 0, ops._ptr(packed[r]), ops._ptr(b), ops._ptr(out[r]), Cout, 0, 1, C.c_float(0.1),
                                       ops._ptr(ws), need, st))

        def second_pass():
            check(L.fn2_col2im_bias_relu_forward_into(ops._ptr(ws), ops._ptr(b), ops._ptr(out[GEMM]), N, Cout, 2 * H, 2 * W, 4, 1, 2, 1, C.c_float(0.1), Cout, 0, st))

        def exact_gemm():
            check(L.fn2_conv_mfma_forward(ops._ptr(x), ops._ptr(packed[GEMM]), None, ops._ptr(ws), N, Cin, H, W, Cin, 0, 16 * Cout, 16 * Cout, 0, 1, 1, 0, 0,
                                          C.c_float(0.0), st))

        run = {"exact": lambda: whole(GEMM), "split": lambda: whole(SPLIT), "col2im": second_pass, "gemm": exact_gemm}
        t = alternate(run)
        whole(GEMM), whole(SPLIT)
        torch.cuda.synchronize()
        med = {k: statistics.median(t[k]) for k in run}
        diff = float((out[GEMM] - out[SPLIT]).abs().max())
        scale = float(out[GEMM].abs().max())
        apart = max(t["split"]) < min(t["exact"])
        table.append("| %s `[%d,%d,%d,%d] -> %d` | %s | %s | %.3f | %s | %.2e | %.2f |" % (name, N, Cin, H, W, Cout, fmt(t["exact"]), fmt(t["split"]),
                                                                                      med["split"] / med["exact"], "yes" if apart else "NO", diff, scale))
        ge, gs = med["exact"] - med["col2im"], med["split"] - med["col2im"]
        parts.append("| %s | %s | %s | %.1f | %.1f | %.3f |" % (name, fmt(t["col2im"]), fmt(t["gemm"]), ge, gs, gs / ge))
        verdict.append("%s: the split route's windows (%.1f .. %.1f us) lie %s the exact route's (%.1f .. %.1f us); ratio of the medians %.3f whole call, %.3f "
                       "GEMM alone (the arithmetic floor is 6/16 = 0.375 of the exact kernel's matrix time)."
                       % (name, min(t["split"]), max(t["split"]), "BELOW" if apart else "NOT below", min(t["exact"]), max(t["exact"]), med["split"] / med["exact"], gs / ge))
        per_variant += variant_rows("deconv_bf16x3", name, run["split"], SPLIT_VARIANTS)
    lines += table + [""] + parts + [""] + verdict + ["", "Tile variants of the split kernel, forced one by one (4 windows each):", ""] + per_variant + [""]
    write_report(a.out, lines)


if __name__ == "__main__":
    main()
