"""What the six *_bf16x3_bench.py probes share: the timing window, the warm-up and the alternating rounds, the "median (min .. max)" cell,
the loop over the tile variants of a split kernel forced one by one, the command line and the report writer.  A probe keeps its layer
table, its callables and its texts."""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from flownet2_amd import _lib  # noqa: E402

ROUNDS, LAUNCHES = 12, 20


def arguments(name, rounds=False):
    """--out (default profiles/<name>.md) and, where the probe offers it, --rounds; a probe needs the GPU."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", name + ".md"))
    if rounds:
        ap.add_argument("--rounds", type=int, default=ROUNDS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("%s: needs the GPU (no fallback: a CPU time says nothing)" % name)
    return a


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES          # us per launch


def alternate(run, rounds=ROUNDS):
    """run: {key: callable}.  Three warm-up windows of each (first launches, variant selection, clocks), then `rounds` windows of each in
    turn: {key: [us per launch]}."""
    for _ in range(3):
        for k in run:
            window(run[k])
    t = {k: [] for k in run}
    for _ in range(rounds):
        for k in run:
            t[k].append(window(run[k]))
    return t


def fmt(v):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))


def variant_rows(knob, row, fn, variants, windows=4):
    """Table rows `| row | v: label | the variant's columns ... | time |` of fn() under every tile variant of fn2_<knob>_num_variants forced in
    turn (one window to settle, then `windows` timed ones); a variant that refuses the problem is left out.  variants[v]: (label, columns ...)."""
    L = _lib.lib()
    force = getattr(L, "fn2_debug_set_%s_variant" % knob)
    rows = []
    try:
        for v in range(int(getattr(L, "fn2_%s_num_variants" % knob)())):
            force(v)
            try:
                window(fn)
            except _lib.Fn2Error:                         # a variant of another geometry class
                continue
            tv = [window(fn) for _ in range(windows)]
            label, *cols = variants[v] if v < len(variants) else ("variant %d" % v,) + ("?",) * (len(variants[0]) - 1)
            rows.append("| %s | %d: %s | %s | %s |" % (row, v, label, " | ".join(str(c) for c in cols), fmt(tv)))
    finally:
        force(-1)
    return rows


def write_report(path, lines):
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)
