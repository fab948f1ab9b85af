"""The bits of the six split-bf16 ("bf16x3") kernels, pinned: SHA-256 of the packed operand (where the kernel has one) and of the result of
every tile variant forced in turn, at the shapes of each kernel's own test file and at their own batch, against tests/golden/bf16x3_bits.json.

The fixture was written once, on an MI355X, from a build of the commit before the kernels came to share csrc/split_bf16.hpp's toolkit; a
change that means to move bits regenerates it (`python tests/test_bf16x3_bits.py --write`, on the GPU) and says so.  pytest only compares."""
import hashlib
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

import test_conv_bf16x3 as conv
import test_correlation_bf16x3 as corr
import test_deconv_bf16x3 as deconv
import test_dgrad_bf16x3 as dgrad
import test_wgrad_bf16x3 as wgrad
import test_wino_bf16x3 as wino
from bf16x3_helpers import forced_variants, host
from test_conv_backward_routes import rand

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16x3_bits.json")


def sha(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32 and np.isfinite(a).all() and a.size
    return hashlib.sha256(a.tobytes()).hexdigest()


def forward_conv(mod, k, transposed=False):
    """conv / deconv / Winograd forward: x seed 1, weights seed 2, bias seed 3; ReLU, bias, slope 0.1"""
    def results(name):
        n, Cin, H, W, Cout = mod.SHAPES[name]
        x, b = rand((n, Cin, H, W), 1), rand((Cout,), 3, 0.1)
        w = rand((Cin, Cout, k, k) if transposed else (Cout, Cin, k, k), 2, 0.1)
        packed = mod.pack(name, w)
        return packed, lambda: {"": mod.run(name, packed, x, b, True, 0.1)}
    return results


def dgrad_results(name):
    """stride-2 data gradient: top_diff seed 1, weights seed 2, the masking blob of dgrad.mask_of (seed 5); plain, and masked with slope 0.1"""
    n, Cin, H, W, Cout = dgrad.SHAPES[name]
    top, w, y = rand((n, Cout) + dgrad.top_hw(name), 1), rand((Cout, Cin, 5, 5), 2, 0.1), dgrad.mask_of(name, seed=5)
    packed = dgrad.pack(name, w)
    return packed, lambda: {"": dgrad.run(name, packed, top), "/masked": dgrad.run_masked(name, packed, top, y, 4, 0.1)}


def wgrad_results(name):
    """5x5/2 weight gradient: bottom blob seed 1, top_diff blob seed 2, the layer's channels a slice of each (wgrad.B_C0, wgrad.A_C0)"""
    n, Cin, H, W, Cout = wgrad.SHAPES[name]
    xb, gb = rand((n, Cin + 5, H, W), 1), rand((n, Cout + 6) + wgrad.top_hw(name), 2)
    return None, lambda: {"": wgrad.run(name, xb, gb)}


def corr_results(name):
    """Correlation forward with FlowNetC's parameters: blobs seed 1 and seed 2; ReLU, slope 0.1"""
    b0, b1 = rand(corr.SHAPES[name], 1), rand(corr.SHAPES[name], 2)
    return None, lambda: {"": corr.run(b0, b1, relu=True, slope=0.1)}


# kernel: (test module, the library's name of its variant functions, results)
KERNELS = {
    "conv": (conv, "conv_bf16x3", forward_conv(conv, 5)),
    "deconv": (deconv, "deconv_bf16x3", forward_conv(deconv, 4, True)),
    "dgrad": (dgrad, "tconv_bf16x3", dgrad_results),
    "wino": (wino, "conv_wino_bf16x3", forward_conv(wino, 3)),
    "wgrad": (wgrad, "conv_wgrad_bf16x3", wgrad_results),
    "corr": (corr, "correlation_bf16x3", corr_results),
}
CASES = [(k, name) for k in KERNELS for name in KERNELS[k][0].SHAPES]


def hashes(kernel, name):
    _, lib_name, results = KERNELS[kernel]
    packed, run = results(name)
    out = {}
    if packed is not None:
        out["%s/%s/packed" % (kernel, name)] = sha(host(packed))
    with forced_variants(lib_name) as (nv, force):
        for v in range(nv):
            force(v)
            for form, got in run().items():
                out["%s/%s/variant%d%s" % (kernel, name, v, form)] = sha(got)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,name", CASES)
def test_bits(kernel, name):
    with open(FIXTURE) as f:
        want = {k: h for k, h in json.load(f)["sha256"].items() if k.startswith("%s/%s/" % (kernel, name))}
    got = hashes(kernel, name)
    assert len(want) >= 2 and got.keys() == want.keys()
    moved = sorted(k for k in got if got[k] != want[k])
    assert not moved, moved


def write():
    out = {}
    for kernel, name in CASES:
        out.update(hashes(kernel, name))
    doc = {
        "made": "written once by tests/test_bf16x3_bits.py --write on the GPU named below, from a build of commit 585c9c2 (the last one before "
                "the six bf16x3 kernels shared csrc/split_bf16.hpp's toolkit)",
        "device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "numpy": np.__version__, "torch": torch.__version__,
        "sha256": out,
    }
    path = sys.argv[sys.argv.index("--write") + 1] if len(sys.argv) > sys.argv.index("--write") + 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d hashes to %s" % (len(out), path))


if __name__ == "__main__":
    assert "--write" in sys.argv, "usage: python tests/test_bf16x3_bits.py --write [path]"
    write()
