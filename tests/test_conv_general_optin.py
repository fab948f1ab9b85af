"""functional.set_general_convolution: the opt-in that moves lib_conv2d / lib_conv_transpose2d from the library convolution (through torch)
to the general kernels (csrc/conv_general.hip).  Under "own" nothing leaves the own kernels: no fallback is counted and FN2_STRICT=1 does
not raise; the default is today's behaviour bit for bit."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conv_general_cases import CONV, DECONV, case, out_hw, row_id, scale_of
from flownet2_amd import functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(False,) + CONV[2], (False,) + CONV[5], (True,) + DECONV[3]]


@pytest.fixture()
def switch():
    was = Fn.general_convolution()
    yield
    Fn.set_general_convolution(was)


def test_the_switch_takes_two_values_and_is_no_arithmetic_switch(switch):
    arith = {s.key: Fn.arithmetic(s.key) for s in Fn.ARITH_SWITCHES}
    assert Fn.general_convolution() == os.environ.get("FN2_CONV_GENERAL", "library")
    for bad in ("gemm", "", None):
        with pytest.raises(ValueError):
            Fn.set_general_convolution(bad)
    Fn.set_general_convolution("own")
    assert Fn.general_convolution() == "own"
    Fn.set_general_convolution("library")
    assert Fn.general_convolution() == "library"
    assert {s.key: Fn.arithmetic(s.key) for s in Fn.ARITH_SWITCHES} == arith and len(Fn.ARITH_SWITCHES) == 6
    assert "general" not in " ".join(s.key + s.env for s in Fn.ARITH_SWITCHES).lower()


def test_cpu_tensors_go_to_torch_under_either_value(switch):
    x, w = torch.randn(1, 3, 6, 7), torch.randn(4, 3, 3, 3)
    want = torch.nn.functional.conv2d(x, w, None, stride=2, padding=1)
    for name in ("library", "own"):
        Fn.set_general_convolution(name)
        before = Fn.LIBRARY_FALLBACKS[0]
        assert torch.equal(Fn.lib_conv2d(x, w, None, 2, 1), want) and Fn.LIBRARY_FALLBACKS[0] == before


def call(row, c, requires_grad=True):
    tr, N, Cin, H, W, Cout, k, s, p = row
    x, w, b = (torch.tensor(c[n], device="cuda").requires_grad_(requires_grad) for n in ("x", "w", "b"))
    return x, w, b, (Fn.lib_conv_transpose2d if tr else Fn.lib_conv2d)(x, w, b, s, p)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_own_runs_forward_and_backward_on_the_general_kernels(switch, row):
    c = case(row)
    N = row[1]
    Ho, Wo = out_hw(row)
    Fn.set_general_convolution("own")
    before = Fn.LIBRARY_FALLBACKS[0]
    x, w, b, top = call(row, c)
    top.backward(torch.tensor(c["g"], device="cuda"))
    assert Fn.LIBRARY_FALLBACKS[0] == before                          # nothing left the own kernels
    for what, got, ref, bound in (("forward", top.detach(), c["top"], 4e-6 * scale_of(c["top"])),
                                  ("data gradient", x.grad, c["gx"], 4e-6 * scale_of(c["gx"])),
                                  ("weight gradient", w.grad, c["gw"], 2e-6 * scale_of(c["gw"]) * math.sqrt(N * Ho * Wo)),
                                  ("bias gradient", b.grad, c["gb"], 2e-6 * scale_of(c["gb"]))):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print("%s %s: error %.3g, bound %.3g, ratio %.3f" % (what, row_id(row), err, bound, err / bound))
        assert got.shape == ref.shape and err <= bound, what
    # a second call gives the same bits; a call without a bias, under no_grad
    assert torch.equal(call(row, c)[3], top)
    with torch.no_grad():
        xs, ws = torch.tensor(c["x"], device="cuda"), torch.tensor(c["w"], device="cuda")
        nb = (Fn.lib_conv_transpose2d if row[0] else Fn.lib_conv2d)(xs, ws, None, row[7], row[8])
    assert float(np.abs(nb.cpu().numpy() - c["top_nobias"]).max()) <= 4e-6 * scale_of(c["top_nobias"])
    assert Fn.LIBRARY_FALLBACKS[0] == before


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_default_counts_one_fallback_per_call_and_equals_torch_bit_for_bit(switch, row):
    c = case(row)
    tr, s, p = row[0], row[7], row[8]
    Fn.set_general_convolution("library")
    before = Fn.LIBRARY_FALLBACKS[0]
    x, w, b, top = call(row, c, requires_grad=False)
    assert Fn.LIBRARY_FALLBACKS[0] == before + 1
    call(row, c, requires_grad=False)
    assert Fn.LIBRARY_FALLBACKS[0] == before + 2
    assert torch.equal(top, (torch.nn.functional.conv_transpose2d if tr else torch.nn.functional.conv2d)(x, w, b, stride=s, padding=p))


CHILD = """
import sys, torch
sys.path.insert(0, sys.argv[1])
from flownet2_amd import functional as Fn
assert Fn.general_convolution() == sys.argv[2]
x, w = torch.randn(2, 5, 9, 12, device="cuda"), torch.randn(33, 5, 4, 4, device="cuda", requires_grad=True)
xt, wt = torch.randn(2, 5, 4, 6, device="cuda"), torch.randn(5, 3, 4, 4, device="cuda", requires_grad=True)
try:
    (Fn.lib_conv2d(x, w, None, 2, 1).sum() + Fn.lib_conv_transpose2d(xt, wt, None, 2, 1).sum()).backward()
except RuntimeError as e:
    print("raised:", e)
    sys.exit(3)
torch.cuda.synchronize()
print("fallbacks:", Fn.LIBRARY_FALLBACKS[0])
"""


@pytest.mark.gpu
def test_strict_mode_in_a_child_process_raises_under_the_default_only():
    def child(value):
        env = dict(os.environ, FN2_STRICT="1")
        env.pop("FN2_CONV_GENERAL", None)
        if value != "library":
            env["FN2_CONV_GENERAL"] = value               # the switch's environment variable
        return subprocess.run([sys.executable, "-c", CHILD, ROOT, value], env=env, capture_output=True, text=True, timeout=300)
    own = child("own")
    assert own.returncode == 0 and "fallbacks: 0" in own.stdout, own.stdout + own.stderr
    lib = child("library")
    assert lib.returncode == 3 and "FN2_STRICT=1" in lib.stdout, lib.stdout + lib.stderr
