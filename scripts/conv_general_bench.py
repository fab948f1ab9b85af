#!/usr/bin/env python
"""Timing of the general-geometry convolution (csrc/conv_general.hip) next to what it stands in for, on the same tensors in one run:
the library convolution through torch at three shapes outside FlowNet's kernel families, and the specialised own route at one FlowNet
shape (the conv3_1 class), which states what generality costs; and (--rows geometry) four layers with groups or dilation
(include/flownet2_hip_conv_geometry.h) against the library; and (--rows volume, batch 4 unless --batch is given) three volumetric layers
(include/flownet2_hip_conv_volume.h) against the library's conv3d / conv_transpose3d.  Forward, data gradient and weight (+ bias) gradient.
Run on the GPU box:
    python scripts/conv_general_bench.py [--iters 20] [--repeats 5] [--batch 8] [--rows square|geometry|volume|all|launch]
Per (shape, pass) one line: the median over the repeats of the mean time per call of each side, the spread (min .. max over the repeats),
the ratio of the medians, and the largest difference between the two results over the result's scale.  The two sides alternate inside
every repeat; every shape is warmed up first (operands are packed outside the timed window, as a layer packs once per weight version)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flownet2_amd import ops  # noqa: E402

# name, transposed, Cin, H, W, Cout, kernel, stride, pad, the other side
SHAPES = [
    ("stem 11x11/4 3->96 @224x224", False, 3, 224, 224, 96, 11, 4, 0, "library"),
    ("3x3/1 48->24 @80x112", False, 48, 80, 112, 24, 3, 1, 1, "library"),
    ("deconv 4x4/2 32->16 @40x56", True, 32, 40, 56, 16, 4, 2, 1, "library"),
    ("conv3_1 class 3x3/1 256->256 @40x56", False, 256, 40, 56, 256, 3, 1, 1, "specialised"),
]
# name, transposed, Cin, H, W, Cout, kernel, stride, pad, dilation, group: against the library
GEOMETRY_SHAPES = [
    ("depthwise 3x3/1 256 @40x56", False, 256, 40, 56, 256, 3, 1, 1, 1, 256),
    ("dilated 3x3/1 d2 256->256 @40x56", False, 256, 40, 56, 256, 3, 1, 2, 2, 1),
    ("group-2 5x5/2 64->128 @160x224", False, 64, 160, 224, 128, 5, 2, 2, 1, 2),
    ("depthwise deconv 4x4/2 128 @40x56", True, 128, 40, 56, 128, 4, 2, 1, 1, 128),
]
# name, transposed, Cin, (D, H, W), Cout, kernel, stride, pad, group: three spatial axes, against the library
VOLUME_SHAPES = [
    ("3x3x3/1 32->32 @16x40x56", False, 32, (16, 40, 56), 32, 3, 1, 1, 1),
    ("deconv 4x4x4/2 32->16 @8x20x28", True, 32, (8, 20, 28), 16, 4, 2, 1, 1),
    ("depthwise 3x3x3/1 64 @16x40x56", False, 64, (16, 40, 56), 64, 3, 1, 1, 64),
]


def timeit(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters           # us per call


def library_passes(x, w, b, g, tr, s, p, d=1, group=1):
    conv = F.conv_transpose2d if tr else F.conv2d

    def backward(mask):
        return torch.ops.aten.convolution_backward(g, x, w, [b.shape[0]], [s, s], [p, p], [d, d], tr, [0, 0], group, mask)
    return {"forward": lambda: conv(x, w, b, stride=s, padding=p, dilation=d, groups=group), "data gradient": lambda: backward([True, False, False])[0],
            "weight + bias gradient": lambda: backward([False, True, True])[1]}


def library_volume_passes(x, w, b, g, tr, s, p, group):
    conv = F.conv_transpose3d if tr else F.conv3d

    def backward(mask):
        return torch.ops.aten.convolution_backward(g, x, w, [b.shape[0]], [s] * 3, [p] * 3, [1] * 3, tr, [0] * 3, group, mask)
    return {"forward": lambda: conv(x, w, b, stride=s, padding=p, groups=group), "data gradient": lambda: backward([True, False, False])[0],
            "weight + bias gradient": lambda: backward([False, True, True])[1]}


def volume_passes(x, w, b, g, geom, tr):
    pf, pd = ops.conv_volume_pack_weights(w, geom, tr), ops.conv_volume_pack_weights(w, geom, tr, backward=True)
    return {"forward": lambda: ops.conv_volume_forward(x, pf, b, geom, tr), "data gradient": lambda: ops.conv_volume_backward_data(g, pd, geom, tr),
            "weight + bias gradient": lambda: ops.conv_volume_backward_weights(x, g, geom, tr)[0]}


def measure(a, name, N, gflop, mine, theirs, other):
    print("%s, batch %d: %.2f GFLOP per pass" % (name, N, gflop), flush=True)
    for what in mine:
        f, r = mine[what], theirs[what]
        got, want = f(), r()                       # (also the warm-up of both sides at this shape)
        for _ in range(2):
            f(), r()
        torch.cuda.synchronize()
        diff = float((got - want[:, :got.shape[1]] if what == "data gradient" else got - want).abs().max()) / max(1.0, float(want.abs().max()))
        tm, tt = [], []
        for _ in range(a.repeats):
            tm.append(timeit(f, a.iters))
            tt.append(timeit(r, a.iters))
        m, t = statistics.median(tm), statistics.median(tt)
        print("   %-22s general %8.1f us (%.1f .. %.1f)  %6.2f TFLOP/s | %s %8.1f us (%.1f .. %.1f) | general / %s = %.2f | max diff / scale %.1e"
              % (what, m, min(tm), max(tm), gflop / m * 1e3, other, t, min(tt), max(tt), other, m / t, diff), flush=True)


def geometry_passes(x, w, b, g, geom, tr):
    pf, pd = ops.conv_geometry_pack_weights(w, geom, tr), ops.conv_geometry_pack_weights(w, geom, tr, backward=True)
    return {"forward": lambda: ops.conv_geometry_forward(x, pf, b, geom, tr), "data gradient": lambda: ops.conv_geometry_backward_data(g, pd, geom, tr),
            "weight + bias gradient": lambda: ops.conv_geometry_backward_weights(x, g, geom, tr)[0]}


def general_passes(x, w, b, g, desc, tr):
    pf, pd = ops.conv_general_pack_weights(w, desc, tr), ops.conv_general_pack_weights(w, desc, tr, backward=True)
    return {"forward": lambda: ops.conv_general_forward(x, pf, b, desc, tr), "data gradient": lambda: ops.conv_general_backward_data(g, pd, desc, tr),
            "weight + bias gradient": lambda: ops.conv_general_backward_weights(x, g, desc, tr)[0]}


def specialised_passes(x, w, b, g, desc, tr):
    route, broute = (ops.deconv_forward_route if tr else ops.conv_forward_route)(desc), ops.conv_backward_data_route(desc, tr)
    if not route or not broute or not ops.conv_backward_weights_supported(desc, tr):
        raise SystemExit("no specialised route for this shape")
    pf, pd = ops.conv_pack_weights(w, desc, route, tr), ops.conv_backward_data_pack_weights(w, desc, tr, broute)

    def wgrad():
        ops.conv_backward_bias(g, desc.Cout)
        return ops.conv_backward_weights(x, g, desc, tr)
    return {"forward": lambda: ops.conv_forward(x, pf, b, desc, route, tr, relu=False), "data gradient": lambda: ops.conv_backward_data(g, pd, desc, tr, broute),
            "weight + bias gradient": wgrad}


def launch_rows(a, gen):
    """The host side alone: one tiny layer (1 x 2 x 4 x 5 -> 3, 2x2 taps, stride 1, pad 0; the volumetric one with a depth of 2) through
    flownet2_amd.functional under set_general_convolution("own"), where the kernels take a few microseconds and the Python wrappers the
    rest.  Wall time per call over --calls calls with one synchronise at the end, after a warm-up; median over the repeats."""
    from flownet2_amd import functional as Fn
    Fn.set_general_convolution("own")
    layers = [("lib_conv2d", Fn.lib_conv2d, (1, 2, 4, 5), (3, 2, 2, 2), 3), ("lib_conv_transpose2d", Fn.lib_conv_transpose2d, (1, 2, 4, 5), (2, 3, 2, 2), 3),
              ("lib_conv3d", Fn.lib_conv3d, (1, 2, 2, 4, 5), (3, 2, 2, 2, 2), 3)]
    for name, f, xs, ws, Cout in layers:
        x, w, b = (torch.randn(s, device="cuda", generator=gen).requires_grad_(True) for s in (xs, ws, (Cout,)))
        with torch.no_grad():
            g = torch.ones_like(f(x, w, b, 1, 0))

        def forward():
            with torch.no_grad():
                f(x, w, b, 1, 0)

        def both():
            torch.autograd.grad(f(x, w, b, 1, 0), (x, w, b), g)
        for what, fn in (("forward", forward), ("forward + backward", both)):
            for _ in range(a.calls // 10):
                fn()
            torch.cuda.synchronize()
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e6 / a.calls)
            print("launch %-22s %-18s %8.1f us per call (%.1f .. %.1f)" % (name, what, statistics.median(t), min(t), max(t)), flush=True)
    if Fn.LIBRARY_FALLBACKS[0]:
        raise SystemExit("conv_general_bench: %d calls left the own kernels" % Fn.LIBRARY_FALLBACKS[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="default: 8, and 4 for the volume rows")
    ap.add_argument("--rows", choices=["square", "geometry", "volume", "all", "launch"], default="all",
                    help="launch: the host time of the opt-in path on one tiny layer (not part of all)")
    ap.add_argument("--calls", type=int, default=2000, help="calls per repeat of the launch rows")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_general_bench: needs the GPU (a CPU run measures nothing)")
    gen = torch.Generator(device="cuda").manual_seed(0)
    if a.rows == "launch":
        return launch_rows(a, gen)
    N = a.batch or 8
    rows = [r[:9] + (1, 1) + r[9:] for r in SHAPES] if a.rows in ("square", "all") else []
    rows += [r + ("library",) for r in GEOMETRY_SHAPES] if a.rows in ("geometry", "all") else []
    for name, tr, Cin, H, W, Cout, k, s, p, d, group, other in rows:
        square = d == 1 and group == 1
        desc = ops.conv_desc(N, Cin, H, W, Cout, k, s, p)
        geom = ops.conv_geometry(N, Cin, H, W, Cout, k, s, p, d, group)
        Ho, Wo = ops.conv_geometry_out_shape(geom, tr)
        x = torch.randn(N, Cin, H, W, device="cuda", generator=gen)
        w = torch.randn((Cin, Cout // group, k, k) if tr else (Cout, Cin // group, k, k), device="cuda", generator=gen) * 0.1
        b = torch.randn(Cout, device="cuda", generator=gen)
        g = torch.randn(N, Cout, Ho, Wo, device="cuda", generator=gen)
        gflop = 2.0 * N * Cin * (Cout // group) * k * k * (H * W if tr else Ho * Wo) / 1e9
        mine = general_passes(x, w, b, g, desc, tr) if square else geometry_passes(x, w, b, g, geom, tr)
        theirs = library_passes(x, w, b, g, tr, s, p, d, group) if other == "library" else specialised_passes(x, w, b, g, desc, tr)
        measure(a, name, N, gflop, mine, theirs, other)
    N = a.batch or 4
    for name, tr, Cin, size, Cout, k, s, p, group in (VOLUME_SHAPES if a.rows in ("volume", "all") else []):
        geom = ops.conv_volume(N, Cin, size, Cout, k, s, p, 1, group)
        out = ops.conv_volume_out_shape(geom, tr)
        x = torch.randn((N, Cin) + size, device="cuda", generator=gen)
        w = torch.randn((Cin, Cout // group, k, k, k) if tr else (Cout, Cin // group, k, k, k), device="cuda", generator=gen) * 0.1
        b = torch.randn(Cout, device="cuda", generator=gen)
        g = torch.randn((N, Cout) + out, device="cuda", generator=gen)
        voxels = size[0] * size[1] * size[2] if tr else out[0] * out[1] * out[2]
        gflop = 2.0 * N * Cin * (Cout // group) * k ** 3 * voxels / 1e9
        measure(a, name, N, gflop, volume_passes(x, w, b, g, geom, tr), library_volume_passes(x, w, b, g, tr, s, p, group), "library")

if __name__ == "__main__":
    main()
