"""Forward-backward consistency, everything that needs no GPU: the header and its binding, the host-only entry point and the refusals of
include/flownet2_hip_flow_consistency.h, the float32 restatement against a 3 x 4 example worked by hand, FlowConsistency.merge / summary,
the PGM writer and the runners' output names."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flow_consistency_ref as CR
from flownet2_amd import _lib, evaluate
from flownet2_amd import functional as Fn
from flownet2_amd.evaluate import CONSISTENCY_COL as COL, CONSISTENCY_COLUMNS, CONSISTENCY_FLAGS, CONSISTENCY_K as K, FlowConsistency

WANT_COLUMNS = ["PIXELS", "NONFINITE", "OUTSIDE", "INCONSISTENT", "OCCLUDED", "BOUNDARY", "ERR_SUM", "ERR_MAX"]
NF, OUT, INC, BND = 1, 2, 4, 8


# ---- the header, the binding, sizes and refusals ----------------------------------------------------------------------------------
def test_header_declares_exactly_what_the_library_exports():
    with open(os.path.join(_lib.INCLUDE_DIR, "flownet2_hip_flow_consistency.h")) as f:
        body = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    want = ["fn2_flow_consistency_sizes", "fn2_flow_consistency"]
    assert re.findall(r"\b(fn2_\w+)\s*\(", body) == want and list(_lib.FLOW_CONSISTENCY_EXPORTS) == want
    symbols = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode().split()
    assert sorted(s for s in symbols if s.startswith("fn2_flow_consistency")) == sorted(want)
    L = _lib.lib()
    for name in want:
        restype, argtypes = _lib.FLOW_CONSISTENCY_PROTOTYPES[name]
        assert restype is C.c_int and getattr(L, name).argtypes == argtypes
    args = _lib.FLOW_CONSISTENCY_PROTOTYPES["fn2_flow_consistency"][1]
    assert len(args) == 21 and args[9] is C.c_void_p and args[10] is C.c_void_p      # double* results, unsigned char* flags: addresses
    # the enums reach the binding through the parser, in a table of their own; the main header and the other tables keep their sizes
    enum = _lib.FLOW_CONSISTENCY_CONSTANTS
    assert [enum["FN2_FLOW_CONSISTENCY_" + n] for n in WANT_COLUMNS] == list(range(8)) and enum["FN2_FLOW_CONSISTENCY_K"] == 8
    assert CONSISTENCY_FLAGS == dict(NONFINITE=NF, OUTSIDE=OUT, INCONSISTENT=INC, BOUNDARY=BND) and len(enum) == 13
    assert len(_lib.CONSTANTS) == 49 and len(_lib.FLOW_METRICS_CONSTANTS) == 16 and len(_lib.EXPORTS) == 159
    assert not set(enum) & (set(_lib.CONSTANTS) | set(_lib.FLOW_METRICS_CONSTANTS)) and not set(want) & set(_lib.PROTOTYPES)
    assert list(CONSISTENCY_COLUMNS) == WANT_COLUMNS and K == 8 and CR.sizes(1, 1, 1)[1] == 8


def test_sizes_grow_with_the_plane_and_are_per_sample():
    planes = [(1, 1), (5, 7), (8, 16), (32, 32), (32, 33), (67, 131), (320, 448), (384, 768), (1024, 2048)]
    per_sample = [CR.sizes(1, h, w)[0] for h, w in planes]
    assert per_sample == sorted(per_sample) and per_sample[0] == 2 * 8 * K and per_sample[3] == 2 * 8 * K and per_sample[4] == 2 * 2 * 8 * K
    assert per_sample[-1] == per_sample[-2] == 2 * 128 * 8 * K                     # two directions, at most 128 partial rows per sample
    for (h, w), one in zip(planes[:-1], per_sample):
        for n in (2, 3, 17):
            assert CR.sizes(n, h, w)[0] == n * one
    L = _lib.lib()
    assert L.fn2_flow_consistency_sizes(2, 5, 7, None, None) == CR.OK               # either out-pointer may be NULL
    nbytes = C.c_size_t(77)
    for shape in ((0, 5, 7), (1 << 10, 1 << 10, 1 << 10), (1 << 22, 1 << 21, 1 << 21)):
        assert L.fn2_flow_consistency_sizes(*shape, C.byref(nbytes), None) == CR.INVALID and nbytes.value == 77


def test_every_host_refusal_writes_nothing_and_names_the_argument():
    """Refusals are decided before any launch, so they need no device: the pointers are host buffers that nobody dereferences."""
    ws_bytes, _ = CR.sizes(2, 5, 7)
    buf = lambda n: (C.c_ubyte * n)(*([0x5A] * n))
    bufs = {k: buf(n) for k, n in (("fw", 560), ("bw", 560), ("results", 2 * 3 * K * 8), ("ws", ws_bytes), ("f0", 70), ("f1", 70), ("o0", 280),
                                   ("o1", 280), ("e0", 280), ("e1", 280), ("w0", 560), ("w1", 560))}
    outs = dict(flags=(bufs["f0"], bufs["f1"]), occ=(bufs["o0"], bufs["o1"]), err=(bufs["e0"], bufs["e1"]), warped=(bufs["w0"], bufs["w1"]))
    cases = CR.refusals(bufs["fw"], bufs["bw"], bufs["results"], outs, bufs["ws"], ws_bytes)
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels) == 21
    for label, want, names, thunk in cases:
        assert thunk() == want, label
        text = _lib.lib().fn2_last_error_string().decode()
        assert text.startswith("flow_consistency:") and names in text, (label, text)
    for k, b in bufs.items():
        assert bytes(b) == b"\x5a" * len(b), k


def test_python_refusals_need_no_device():
    z = torch.zeros(1, 2, 3, 4)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.flow_consistency(z, z)
    with pytest.raises(RuntimeError, match="not differentiable"):
        Fn.flow_consistency(z.clone().requires_grad_(True), z)
    with torch.no_grad(), pytest.raises(ValueError, match="no CPU path"):           # under no_grad the gradient check passes; the device check stays
        Fn.flow_consistency(z.clone().requires_grad_(True), z)
    import flownet2_amd
    assert flownet2_amd.flow_consistency is Fn.flow_consistency and flownet2_amd.FlowConsistency is FlowConsistency


# ---- the restatement on a case worked by hand ------------------------------------------------------------------------------------------
def _hand_case():
    fw = np.zeros((1, 2, 3, 4), np.float32)
    fw[0, 0] = 1.0                                                                  # (+1, 0) everywhere ...
    fw[0, :, 0, 0] = 0.5                                                            # ... but (0.5, 0.5) at (x, y) = (0, 0): a target between four pixels
    fw[0, 0, 2, 0] = np.nan                                                         # and NaN at (0, 2)
    bw = np.zeros((1, 2, 3, 4), np.float32)
    bw[0, 0] = -1.0                                                                 # (-1, 0) everywhere ...
    bw[0, 0, 1, 2] = -3.0                                                           # ... but (-3, 0) at (2, 1)
    return fw, bw


def test_restatement_on_a_3x4_case_worked_by_hand():
    """Direction 0, a = fw.  Column 3 points to x2 = 4: OUTSIDE.  (1, 1) samples bw at (2, 1) = (-3, 0): s = 4 > 0.01 * 10 + 0.5, err = 2.
    (0, 0) samples the mean of four (-1, 0): su = -0.5, sv = 0.5, s = 0.5 <= 0.01 * 1.5 + 0.5, err = sqrt(0.5); its flow differs from its
    neighbours' by (0.5, -0.5), so it and (1, 0) carry BOUNDARY (g = 0.25 and 0.125), while (0, 1) has the NaN of (0, 2) below it and
    carries none, like (1, 2).  Direction 1, a = bw.  Column 0 points to x2 = -1 and (2, 1) to x2 = -1: OUTSIDE; the four neighbours of
    (2, 1) see a step of 2 in u: BOUNDARY; (1, 2) samples the NaN of fw at (0, 2): NONFINITE, and so is (1, 1), whose lower-left tap is that NaN with weight 0 (0 * NaN is NaN, in
    FlowWarp too); (1, 0) samples (0.5, 0.5): err = sqrt(0.5)."""
    fw, bw = _hand_case()
    r = np.float32(np.sqrt(np.float32(0.5)))
    nan = np.float32(np.nan)
    d0, d1 = CR.ref32(fw, bw)
    assert d0["flags"][0, 0].tolist() == [[BND, BND, 0, OUT], [0, INC, 0, OUT], [NF, 0, 0, OUT]]
    assert d1["flags"][0, 0].tolist() == [[OUT, 0, BND, 0], [OUT, NF | BND, OUT, BND], [OUT, NF, BND, 0]]
    assert d0["occ"][0, 0].tolist() == [[0, 0, 0, 1], [0, 1, 0, 1], [1, 0, 0, 1]]
    assert d1["occ"][0, 0].tolist() == [[1, 0, 0, 0], [1, 1, 1, 0], [1, 1, 0, 0]]
    want0 = np.array([[r, 0, 0, nan], [0, 2, 0, nan], [nan, 0, 0, nan]], np.float32)
    want1 = np.array([[nan, r, 0, 0], [nan, nan, nan, 0], [nan, nan, 0, 0]], np.float32)
    for d, want in ((d0, want0), (d1, want1)):
        assert d["err"].dtype == np.float32 and d["occ"].dtype == np.float32 and d["flags"].dtype == np.uint8
        assert np.array_equal(d["err"][0, 0], want, equal_nan=True)
    assert np.array_equal(d0["warped"][0, 0, 1], np.array([-1, -3, -1, nan], np.float32), equal_nan=True)
    assert np.isnan(d1["warped"][0, 0, 2, 1]) and d1["warped"][0, 1, 2, 1] == 0       # the NaN tap reaches u alone

    def row(**kw):
        out = np.zeros(K)
        for k, v in kw.items():
            out[COL[k]] = v
        return out
    w0 = row(PIXELS=12, NONFINITE=1, OUTSIDE=3, INCONSISTENT=1, OCCLUDED=5, BOUNDARY=2, ERR_SUM=2.0 + float(r), ERR_MAX=2.0)
    w1 = row(PIXELS=12, NONFINITE=2, OUTSIDE=4, INCONSISTENT=0, OCCLUDED=6, BOUNDARY=4, ERR_SUM=float(r), ERR_MAX=float(r))
    assert np.array_equal(d0["rows"], np.stack([w0, w0])) and np.array_equal(d1["rows"], np.stack([w1, w1]))
    # the float64 evaluation agrees with the float32 sum within its own bound, and the bound is small
    for a, o, d in ((fw, bw, d0), (bw, fw, d1)):
        ref, bnd, full = CR.err_sum_bound(a, o)
        assert np.array_equal(full, ~np.isnan(d["err"][:, 0]))
        assert np.all(np.abs(d["rows"][:, COL["ERR_SUM"]] - ref) <= bnd) and np.all(bnd <= 1e-5 * ref) and np.all(bnd > 0)


def test_restatement_never_converts_what_it_must_not():
    """1e10, +-Inf and NaN at the pixel: NONFINITE and nothing else, no warning from a conversion; at a neighbour: no BOUNDARY flag."""
    import warnings
    for bad in (np.nan, np.inf, -np.inf, 1e10, -1e10):
        fw = np.zeros((1, 2, 3, 3), np.float32)
        bw = np.zeros((1, 2, 3, 3), np.float32)
        fw[0, 1, 1, 1] = bad
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            d0, d1 = CR.ref32(fw, bw)
        want = np.zeros((3, 3), np.uint8)
        want[1, 1] = NF
        assert np.array_equal(d0["flags"][0, 0], want), bad
        # bw is zero, so a pixel's target is the pixel and its right / lower / lower-right taps carry weight 0: 0 * 1e10 is 0, but
        # 0 * NaN and 0 * Inf are NaN (in FlowWarp too), so there the three pixels up and left of (1, 1) have no finite sample either
        if not np.isfinite(bad):
            want[0:2, 0:2] = NF
        assert np.array_equal(d1["flags"][0, 0], want), bad
        assert np.isnan(d0["err"][0, 0, 1, 1]) and np.nansum(d0["err"]) == 0


# ---- FlowConsistency -------------------------------------------------------------------------------------------------------------------
def test_merge_and_summary_by_hand():
    def row(**kw):
        out = np.zeros(K)
        for k, v in kw.items():
            out[COL[k]] = v
        return out
    a = FlowConsistency([row(PIXELS=20, NONFINITE=1, OUTSIDE=3, INCONSISTENT=4, OCCLUDED=8, BOUNDARY=5, ERR_SUM=8.0, ERR_MAX=3.0)],
                        [row(PIXELS=20, OUTSIDE=2, OCCLUDED=2, ERR_SUM=9.0, ERR_MAX=1.5)])
    b = FlowConsistency([row(PIXELS=20, OUTSIDE=20, OCCLUDED=20), row(PIXELS=20, ERR_SUM=2.0, ERR_MAX=4.5)], [row(PIXELS=20), row(PIXELS=20)])
    m = a.merge([b])
    assert len(m) == 3 and np.array_equal(m.rows_fw, np.concatenate([a.rows_fw, b.rows_fw])) and len(a) == 1 and len(b) == 2
    s = m.summary()
    assert list(s) == ["fw", "bw", "samples", "alpha", "beta"] and s["samples"] == 3 and s["alpha"] == [0.01, 0.5] and s["beta"] == [0.01, 0.002]
    assert list(s["fw"]) == ["occluded", "outside", "inconsistent", "nonfinite", "boundary", "err_mean", "err_max", "pixels"]
    assert s["fw"] == dict(occluded=28 / 60, outside=23 / 60, inconsistent=4 / 60, nonfinite=1 / 60, boundary=5 / 60, err_mean=10.0 / 36, err_max=4.5,
                           pixels=60)
    assert s["bw"]["err_mean"] == 9.0 / 58 and s["bw"]["occluded"] == 2 / 60
    one = b.sample(0).summary()["fw"]
    assert one["outside"] == 1.0 and math.isnan(one["err_mean"])                    # no pixel has an err: nan here, null in the file

    def refuse(token):
        raise AssertionError(f"{token} is not JSON")
    doc = json.loads(m.to_json(), parse_constant=refuse)
    assert doc["columns"] == WANT_COLUMNS and len(doc["lines"]) == 3 and doc["lines"][1]["fw"]["err_mean"] is None
    assert doc["summary"]["fw"]["pixels"] == 60 and np.array_equal(np.array(doc["rows_bw"]), m.rows_bw)
    assert math.isnan(FlowConsistency().summary()["fw"]["occluded"]) and json.loads(FlowConsistency().to_json())["lines"] == []
    # the runners' gather (one process): groups arrive in any order and land in list order; a missing entry is an error
    g = evaluate.gather_consistency(3, [([1, 2], b), ([0], a)])
    assert np.array_equal(g.rows_fw, m.rows_fw) and np.array_equal(g.rows_bw, m.rows_bw) and g.to_json() == m.to_json()
    with pytest.raises(RuntimeError, match=r"no result for list entries \[0\]"):
        evaluate.gather_consistency(3, [([1, 2], b)])
    with pytest.raises(ValueError, match="must be"):
        FlowConsistency(np.zeros((2, K + 1)), np.zeros((2, K + 1)))
    with pytest.raises(ValueError, match="forward rows"):
        FlowConsistency(np.zeros((2, K)), np.zeros((1, K)))
    with pytest.raises(ValueError, match="thresholds differ"):
        a.merge([FlowConsistency(alpha=(0.02, 0.5))])


# ---- the PGM writer and the output names ------------------------------------------------------------------------------------------------
def test_pgm_bytes(tmp_path):
    path = str(tmp_path / "m.pgm")
    evaluate.write_pgm(path, np.array([[0.0, 1.0, 0.0], [2.5, 0.0, -1.0]], np.float32))
    assert open(path, "rb").read() == b"P5\n3 2\n255\n" + bytes([0, 255, 0, 255, 0, 255])
    evaluate.write_pgm(path, np.zeros((1, 1, 2), np.float32))
    assert open(path, "rb").read() == b"P5\n2 1\n255\n\x00\x00"
    from PIL import Image
    evaluate.write_pgm(path, np.eye(3))
    assert np.array_equal(np.asarray(Image.open(path)), np.eye(3, dtype=np.uint8) * 255)      # another decoder reads it
    with pytest.raises(ValueError, match="plane"):
        evaluate.write_pgm(path, np.zeros((2, 2, 2)))


def test_runner_output_names():
    assert evaluate.bidirectional_names("a/b/out.flo") == ("a/b/out.bw.flo", "a/b/out.occ.pgm", "a/b/out.bw.occ.pgm")
    assert evaluate.bidirectional_names("x.y.flo") == ("x.y.bw.flo", "x.y.occ.pgm", "x.y.bw.occ.pgm")
    assert evaluate.bidirectional_names("noext") == ("noext.bw.flo", "noext.occ.pgm", "noext.bw.occ.pgm")
