#!/usr/bin/env python
"""Per-layer GPU time of one deploy forward as the graph routes it (own kernels, GEMM route, library): a nets.GraphBackend whose layer ops
and custom layers run between two HIP events.  Each layer is timed in isolation (synchronised), so the sum exceeds the
pipelined step a little; the point is the ranking.
    python scripts/step_breakdown.py [--net C|2] [--batch 8 --height 320 --width 448] [--iters 10]"""
import argparse
import collections
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flownet2_amd import functional as Fn, nets  # noqa: E402

T = collections.OrderedDict()


def timed(label_fn, fn):
    def wrapper(*a, **k):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = fn(*a, **k)
        e1.record()
        torch.cuda.synchronize()
        lab = label_fn(a, k, y)
        T.setdefault(lab, []).append(e0.elapsed_time(e1) * 1e3)
        return y
    return wrapper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="C")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=448)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P = nets.init_params_flownet2(0, dev) if a.net == "2" else nets.init_params(a.net, 0, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    i0 = torch.rand(a.batch, 3, a.height, a.width, device=dev, generator=g) * 255
    i1 = torch.rand(a.batch, 3, a.height, a.width, device=dev, generator=g) * 255

    # a wrapping adapter: the layer ops of the graphs and the backend's custom layers, each between two HIP events; a listener notes the route
    be = nets.GraphBackend(Fn)
    layer_of = {id(v): k[:-2] for k, v in P.items() if k.endswith(".w")}

    def conv_label(args, k, y):
        x, PP, name = args[0], args[1], args[2]
        w = PP[name + ".w"]
        gf = 2.0 * y.shape[0] * y.shape[1] * y.shape[2] * y.shape[3] * w.shape[1] * w.shape[2] * w.shape[3] / 1e9
        return "%s%-12s %-20s k%ds%d %7.2f GF  %s" % (getattr(PP, "prefix", ""), name, tuple(x.shape), w.shape[2], args[3], gf, nets._LAST_ROUTE[0])

    def deconv_label(args, k, y):
        x, PP, name = args[0], args[1], args[2]
        w = PP[name + ".w"]
        gf = 2.0 * x.shape[0] * x.shape[2] * x.shape[3] * w.shape[0] * w.shape[1] * 16 / 1e9
        return "%-12s %-20s deconv %7.2f GF" % (name, tuple(x.shape), gf)

    def into_label(args, k, y):                     # own_conv(x, w, b, stride, pad, slope, act, out=blob, ...): a skip convolution or conv_redir
        x, w, o = args[0], args[1], k["out"]
        gf = 2.0 * o.shape[0] * w.shape[0] * o.shape[2] * o.shape[3] * w.shape[1] * w.shape[2] * w.shape[3] / 1e9
        return "%-12s %-20s k%ds%d %7.2f GF  %s" % (layer_of[id(w)], tuple(x.shape), w.shape[2], args[3], gf, "into concat blob" if y is not None else "(declined)")

    be.conv, be.deconv = timed(conv_label, be.conv), timed(deconv_label, be.deconv)
    own_conv, timed_into = be.own_conv, timed(into_label, be.own_conv)
    be.own_conv = lambda *args, **k: (timed_into if k.get("out") is not None else own_conv)(*args, **k)      # (a plain call is inside its conv row)
    be.own_deconv = timed(lambda args, k, y: "%-12s %-20s -> %d  %s" % ("deconv_relu", tuple(args[0].shape), args[1].shape[1], "own kernel" if y is not None else "(declined)"),
                          be.own_deconv)
    for nm, shown in (("predict_flow", "predict_flow_conv"), ("upsample_flow", "upsample_flow_deconv"), ("own_correlation_relu_into", "correlation_relu_into"),
                      ("resample",) * 2, ("flow_warp",) * 2, ("channel_norm",) * 2):
        setattr(be, nm, timed(lambda args, k, y, shown=shown: "%-12s %s" % (shown, tuple(args[0].shape)), getattr(be, nm)))
    cat = torch.cat
    torch.cat = timed(lambda args, k, y: "torch.cat -> %s" % (tuple(y.shape),), cat)
    fwd = (lambda: nets.flownet2_deploy_forward(P, i0, i1, be)) if a.net == "2" else (lambda: nets.deploy_forward(a.net, P, i0, i1, be))
    with torch.no_grad(), nets.listening(nets._note_route):
        for _ in range(3):
            fwd()
        T.clear()
        for _ in range(a.iters):
            fwd()
    tot = 0.0
    for lab, v in T.items():
        per_step = sum(v) / a.iters
        tot += per_step
        print("%8.1f us  x%-2d %s" % (per_step, len(v) // a.iters, lab))
    print("%8.1f us  sum of the wrapped calls" % tot)


if __name__ == "__main__":
    main()
