"""What the tests of the split-bf16 ("bf16x3") kernels share: the flag values of include/flownet2_hip.h and the forced-variant loop."""
import contextlib

from flownet2_amd import _lib, ops
from flownet2_amd._lib import check

BIT = ops.CONV_ARITH_BF16X3
F_FORCE, F_BF16X3 = ops.ROUTE_FORCE, ops.ROUTE_BF16X3


def host(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def forced_variants(name):
    """(number of tile variants, force(v)) of fn2_<name>_num_variants / fn2_debug_set_<name>_variant; leaves the autotuned pick in place."""
    L = _lib.lib()
    force = getattr(L, "fn2_debug_set_%s_variant" % name)
    try:
        yield int(getattr(L, "fn2_%s_num_variants" % name)()), lambda v: check(force(v))
    finally:
        check(force(-1))
