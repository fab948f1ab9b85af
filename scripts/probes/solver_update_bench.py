"""The solver update (csrc/solver_update.hip) against torch.optim.Adam(fused=True).step() on FlowNetC's parameter set, in one process.

    python scripts/probes/solver_update_bench.py [--windows 12] [--launches 20] [--out profiles/solver_update.md]

Both optimizers step the SAME tensors (nets.init_params("C"): 48 blobs, about 39 M values) with the same gradients; warmed up, then timed
alternately with device events, `--windows` windows of `--launches` steps each; ms per step as median (min .. max) over the windows.  The
traffic roof beside them: Adam reads w, g, m, v and writes w, m, v = 7 arrays of 4 bytes per value, at the 6.29 TB/s a float4 copy
measures on an MI355X.  Variants of the update: clipping on (two more launches, one more read of g), write_update (one more array written),
SGD (5 arrays).  A measurement path without a GPU fails: there is no CPU timing.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from flownet2_amd import nets, ops  # noqa: E402
from flownet2_amd.solver import CaffeOptimizer, SolverParameter  # noqa: E402

COPY_TBS = 6.29       # measured float4 copy rate of an MI355X, TB/s


def windows(fns, n_windows, launches):
    """{name: [ms per step, one per window]}, the candidates alternating window by window."""
    out = {k: [] for k in fns}
    for _ in range(n_windows):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / launches)
    return out


def fmt(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("solver_update_bench: no GPU; nothing is timed on a CPU")
    dev = torch.device("cuda")
    P = [v.to(dev).requires_grad_(True) for v in nets.init_params("C", seed=0).values()]
    g = torch.Generator(device=dev).manual_seed(1)
    for p in P:
        p.grad = 1e-3 * torch.randn(p.shape, generator=g, device=dev)
    n = sum(p.numel() for p in P)
    adam = 'type: "Adam" base_lr: 1e-5 lr_policy: "fixed" momentum: 0.9 momentum2: 0.999 weight_decay: 0.0004 '
    decay = [0.0 if p.dim() == 1 else 1.0 for p in P]
    opts = {
        "torch.optim.Adam(fused=True).step()": torch.optim.Adam(P, lr=1e-5, fused=True),
        "CaffeOptimizer Adam": CaffeOptimizer(P, SolverParameter(adam), decay_mults=decay),
        "CaffeOptimizer Adam, clip_gradients on": CaffeOptimizer(P, SolverParameter(adam + "clip_gradients: 1000"), decay_mults=decay),
        "CaffeOptimizer Adam, write_update": CaffeOptimizer(P, SolverParameter(adam), decay_mults=decay, write_update=True),
        "CaffeOptimizer SGD": CaffeOptimizer(P, SolverParameter('type: "SGD" base_lr: 1e-5 lr_policy: "fixed" momentum: 0.9 weight_decay: 0.0004'), decay_mults=decay),
    }
    arrays = {"torch.optim.Adam(fused=True).step()": 7, "CaffeOptimizer Adam": 7, "CaffeOptimizer Adam, clip_gradients on": 8,
              "CaffeOptimizer Adam, write_update": 8, "CaffeOptimizer SGD": 5}
    fns = {k: o.step for k, o in opts.items()}
    for _ in range(3):                                     # warm-up: code objects, the tables, torch's fused state
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    # the raw launch, without the Optimizer wrapper (hooks, the rate, the ctypes call stay): what Solver.ApplyUpdate pays
    o = opts["CaffeOptimizer Adam"]
    params = o._update_params()
    fns["ops.solver_apply_update alone (Adam)"] = lambda: ops.solver_apply_update(o._table, params, 1e-5, 1.0, False)
    arrays["ops.solver_apply_update alone (Adam)"] = 7
    t = windows(fns, a.windows, a.launches)
    lines = ["# Solver update: one launch over every blob against torch's fused Adam", "",
             "`scripts/probes/solver_update_bench.py` on %s: FlowNetC's parameter set (%d blobs, %.1f M values, %d chunks of %d), every candidate "
             "stepping the same tensors in one process, warmed up, timed alternately with device events, %d windows of %d steps each; ms per step, "
             "median (min .. max).  Roof = arrays x %.0f MB at the %.2f TB/s a float4 copy measures."
             % (torch.cuda.get_device_name(0), len(P), n / 1e6, o._table.nchunks, ops.SOLVER_CHUNK, a.windows, a.launches, 4 * n / 1e6, COPY_TBS), "",
             "| step | ms per step | arrays moved | traffic roof, ms | roof / measured |", "|---|---|---|---|---|"]
    for k, v in t.items():
        roof = arrays[k] * 4 * n / (COPY_TBS * 1e12) * 1e3
        lines.append("| %s | %s | %d | %.3f | %.2f |" % (k, fmt(v), arrays[k], roof, roof / statistics.median(v)))
    ref, own = t["torch.optim.Adam(fused=True).step()"], t["CaffeOptimizer Adam"]
    verdict = ("BELOW torch's" if max(own) < min(ref) else "ABOVE torch's" if min(own) > max(ref) else "overlapping torch's")
    lines += ["", "CaffeOptimizer Adam: windows %.3f .. %.3f ms, %s (%.3f .. %.3f ms); ratio of the medians %.3f."
              % (min(own), max(own), verdict, min(ref), max(ref), statistics.median(own) / statistics.median(ref))]
    report = "\n".join(lines) + "\n"
    print(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
