"""Flow evaluation, everything that needs no GPU: the header and its binding, the host-only entry point and the refusals of
include/flownet2_hip_flow_metrics.h, FlowMetrics.merge / summary against hand-computed values, the KITTI flow PNG, the list parser and the
shard / gather / merge loop of flownet2_amd/evaluate.py driven by a stub predictor over gloo."""
import ctypes as C
import math
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import flow_metrics_ref as FR
from flownet2_amd import _lib, evaluate, flo
from flownet2_amd.evaluate import COL, COLUMNS, FlowMetrics, K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT_COLUMNS = ["VALID", "NONFINITE", "EPE_SUM", "EPE_SQ_SUM", "EPE_MAX", "OUTLIERS", "AE_SUM", "BAND_COUNT0", "BAND_COUNT1", "BAND_COUNT2",
                "BAND_EPE_SUM0", "BAND_EPE_SUM1", "BAND_EPE_SUM2", "OCC_COUNT", "OCC_EPE_SUM"]


# ---- the header, the binding, sizes and refusals ----------------------------------------------------------------------------------
def test_header_declares_exactly_what_the_binding_has():
    with open(os.path.join(_lib.INCLUDE_DIR, "flownet2_hip_flow_metrics.h")) as f:
        body = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    want = ["fn2_flow_metrics_sizes", "fn2_flow_metrics"]
    assert re.findall(r"\b(fn2_\w+)\s*\(", body) == want and list(_lib.FLOW_METRICS_EXPORTS) == want
    L = _lib.lib()
    for name in want:
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is C.c_int and getattr(L, name).argtypes == argtypes
    assert _lib.PROTOTYPES["fn2_flow_metrics"][1][11] is C.c_void_p                  # double* results travels as an address
    # the enum reaches the binding through the parser, in the order stated, and the Python side reads its columns from there -- in a table
    # of its own beside CONSTANTS, whose 49 entries of the other seven headers tests/test_abi_binding.py counts
    enum = _lib.FLOW_METRICS_CONSTANTS
    assert [enum["FN2_FLOW_METRICS_" + n] for n in WANT_COLUMNS] == list(range(15)) and enum["FN2_FLOW_METRICS_K"] == 15 and len(enum) == 16
    assert len(_lib.CONSTANTS) == 49 and not set(enum) & set(_lib.CONSTANTS)
    assert list(COLUMNS) == WANT_COLUMNS and K == 15 and FR.sizes(1, 1, 1)[1] == 15
    # the other seven lists keep their lengths; nothing went into the main header
    lengths = [len(getattr(_lib, n)) for n in ("EXPORTS", "SOLVER_EXPORTS", "CORR_ROUTE_EXPORTS", "CONV_GENERAL_EXPORTS", "CONV_GEOMETRY_EXPORTS",
                                               "CONV_VOLUME_EXPORTS", "LPQ_LOSS_EXPORTS")]
    assert lengths[0] == 159 and lengths[-1] == 6 and sum(lengths) + 2 == len(_lib.PROTOTYPES)
    assert not any("flow_metrics" in n for n in _lib.EXPORTS)


def test_sizes_grow_with_the_plane_and_are_per_sample():
    planes = [(1, 1), (5, 7), (8, 16), (32, 32), (32, 33), (67, 131), (320, 448), (384, 768), (1024, 2048)]
    per_sample = [FR.sizes(1, h, w)[0] for h, w in planes]
    assert per_sample == sorted(per_sample) and per_sample[0] == 8 * K and per_sample[3] == 8 * K and per_sample[4] == 2 * 8 * K
    assert per_sample[-1] == per_sample[-2] == 128 * 8 * K                         # at most 128 partial rows per sample
    for (h, w), one in zip(planes[:-1], per_sample):
        for n in (2, 3, 17):
            assert FR.sizes(n, h, w)[0] == n * one
    hw = np.arange(1, 5000)
    got = [FR.sizes(1, 1, int(x))[0] for x in hw]
    assert got == sorted(got)                                                       # no dip where H W stops being a multiple of 4
    assert _lib.lib().fn2_flow_metrics_sizes(2, 5, 7, None, None) == FR.OK         # either out-pointer may be NULL
    nbytes = C.c_size_t(77)
    assert _lib.lib().fn2_flow_metrics_sizes(0, 5, 7, C.byref(nbytes), None) == FR.INVALID and nbytes.value == 77
    assert _lib.lib().fn2_flow_metrics_sizes(1 << 10, 1 << 10, 1 << 10, C.byref(nbytes), None) == FR.INVALID and nbytes.value == 77
    assert _lib.lib().fn2_flow_metrics_sizes(1 << 22, 1 << 21, 1 << 21, C.byref(nbytes), None) == FR.INVALID and nbytes.value == 77      # wraps to 0 if multiplied at once
    assert FR.sizes(1, 1 << 15, (1 << 15) - 1)[0] == 128 * 8 * K                    # the largest plane but one row: 2^31 - 2^16 elements


def test_every_host_refusal_writes_nothing():
    """Refusals are decided before any launch, so they need no device: the pointers are host buffers that nobody dereferences."""
    ws_bytes, _ = FR.sizes(2, 5, 7)
    buf = lambda n: (C.c_ubyte * n)(*([0x5A] * n))
    bufs = {k: buf(n) for k, n in (("pred", 560), ("gt", 560), ("valid", 280), ("occ", 280), ("results", 3 * K * 8), ("epe_map", 280),
                                   ("ws", ws_bytes))}
    cases = FR.refusals(bufs["pred"], bufs["gt"], bufs["valid"], bufs["occ"], bufs["results"], bufs["epe_map"], bufs["ws"], ws_bytes)
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels) == 23
    for label, want, thunk in cases:
        assert thunk() == want, label
        assert _lib.lib().fn2_last_error_string().decode().startswith("flow_metrics"), label
    for k, b in bufs.items():
        assert bytes(b) == b"\x5a" * len(b), k


# ---- FlowMetrics ---------------------------------------------------------------------------------------------------------------------
def _row(**kw):
    r = np.zeros(K)
    for k, v in kw.items():
        r[COL[k]] = v
    return r


def test_merge_and_summary_by_hand():
    a = FlowMetrics([_row(VALID=4, EPE_SUM=8.0, EPE_SQ_SUM=20.0, EPE_MAX=3.5, OUTLIERS=1, AE_SUM=0.4, BAND_COUNT0=3, BAND_COUNT1=1,
                          BAND_EPE_SUM0=2.0, BAND_EPE_SUM1=6.0, OCC_COUNT=1, OCC_EPE_SUM=5.0)])
    b = FlowMetrics([_row(VALID=12, NONFINITE=2, EPE_SUM=6.0, EPE_SQ_SUM=9.0, EPE_MAX=7.25, OUTLIERS=3, AE_SUM=1.2, BAND_COUNT0=12,
                          BAND_EPE_SUM0=6.0, OCC_COUNT=3, OCC_EPE_SUM=3.0),
                     _row()])                                                       # a sample without ground truth
    m = a.merge([b])
    assert len(m) == 3 and np.array_equal(m.rows, np.concatenate([a.rows, b.rows])) and len(a) == 1 and len(b) == 2
    assert np.array_equal(a.merge([]).rows, a.rows) and len(FlowMetrics().merge([a, b])) == 3
    s = m.summary()
    assert list(s) == ["epe", "epe_pixel", "fl_all", "ae_deg", "s0_10", "s10_40", "s40plus", "epe_matched", "epe_unmatched", "epe_max", "pixels",
                       "samples", "nonfinite", "samples_without_ground_truth"]
    # two samples of unequal valid counts: the mean of the means (8/4 + 6/12) / 2 against the pixel-weighted (8 + 6) / 16
    assert s["epe"] == (8.0 / 4 + 6.0 / 12) / 2 == 1.25 and s["epe_pixel"] == 14.0 / 16 == 0.875
    assert s["fl_all"] == 100.0 * 4 / 16 and s["ae_deg"] == math.degrees(1.6 / 16)
    assert s["s0_10"] == 8.0 / 15 and s["s10_40"] == 6.0 and math.isnan(s["s40plus"])
    assert s["epe_matched"] == (14.0 - 8.0) / (16 - 4) and s["epe_unmatched"] == 8.0 / 4 and s["epe_max"] == 7.25
    assert (s["pixels"], s["samples"], s["nonfinite"], s["samples_without_ground_truth"]) == (16, 3, 2, 1)
    assert all(type(s[k]) is int for k in ("pixels", "samples", "nonfinite", "samples_without_ground_truth"))
    assert all(type(v) in (int, float) for v in s.values())


def test_summary_zero_denominators_are_nan_without_a_warning():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for m in (FlowMetrics(), FlowMetrics([_row()]), FlowMetrics([_row(NONFINITE=5)])):
            s = m.summary()
            for k in ("epe", "epe_pixel", "fl_all", "ae_deg", "s0_10", "s10_40", "s40plus", "epe_matched", "epe_unmatched"):
                assert math.isnan(s[k]), k
            assert s["pixels"] == 0 and s["samples"] == len(m)
    assert math.isnan(FlowMetrics().summary()["epe_max"]) and FlowMetrics([_row()]).summary()["epe_max"] == 0.0
    assert FlowMetrics([_row()]).summary()["samples_without_ground_truth"] == 1
    assert FlowMetrics([_row(NONFINITE=5)]).summary()["samples_without_ground_truth"] == 0       # it has ground truth; the prediction is bad
    no_occ = FlowMetrics([_row(VALID=2, EPE_SUM=3.0)]).summary()
    assert math.isnan(no_occ["epe_unmatched"]) and no_occ["epe_matched"] == 1.5
    with pytest.raises(ValueError, match="rows must be"):
        FlowMetrics(np.zeros((2, K + 1)))


def test_json_is_strict_and_the_exit_status_follows_nonfinite():
    import json

    def refuse(token):
        raise AssertionError(f"{token} is not JSON")
    m = FlowMetrics([_row(VALID=2, EPE_SUM=3.0, EPE_MAX=2.0, BAND_COUNT0=2, BAND_EPE_SUM0=3.0), _row(NONFINITE=3)])
    doc = json.loads(m.to_json(), parse_constant=refuse)                          # NaN, Infinity and -Infinity would come through here
    s = m.summary()
    assert math.isnan(s["s40plus"]) and math.isnan(s["epe_unmatched"])             # summary() itself keeps nan ...
    assert doc["summary"]["s40plus"] is None and doc["summary"]["epe_unmatched"] is None and doc["summary"]["s10_40"] is None   # ... the file has null
    assert doc["summary"]["epe"] == 1.5 and doc["summary"]["nonfinite"] == 3 and doc["summary"] == evaluate.json_ready(s)
    assert doc["columns"] == WANT_COLUMNS and np.array_equal(np.array(doc["rows"]), m.rows)
    assert json.loads(FlowMetrics().to_json(), parse_constant=refuse)["summary"]["epe_max"] is None
    assert evaluate.exit_status(s) == 1 and evaluate.exit_status(s, allow_nonfinite=True) == 0
    clean = FlowMetrics([_row(VALID=2, EPE_SUM=3.0)]).summary()
    assert evaluate.exit_status(clean) == 0 and evaluate.exit_status(clean, allow_nonfinite=True) == 0


def test_reference_rows_on_a_case_worked_by_hand():
    """The float64 restatement itself, on four pixels whose numbers can be checked by eye."""
    pred = np.array([[[[3.0, 0.0, 1.0, np.inf]], [[4.0, 0.0, 1.0, 0.0]]]], np.float32)
    gt = np.array([[[[0.0, 0.0, 1.0, 2.0]], [[0.0, 30.0, np.nan, 0.0]]]], np.float32)
    occ = np.array([[[[0.0, 1.0, 1.0, 1.0]]]], np.float32)
    rows = FR.ref64(pred, gt, None, occ)
    want = _row(VALID=2, NONFINITE=1, EPE_SUM=35.0, EPE_SQ_SUM=925.0, EPE_MAX=30.0, OUTLIERS=2, AE_SUM=math.atan2(5.0, 1.0) + math.atan2(30.0, 1.0),
                BAND_COUNT0=1, BAND_COUNT1=1, BAND_EPE_SUM0=5.0, BAND_EPE_SUM1=30.0, OCC_COUNT=1, OCC_EPE_SUM=30.0)
    assert np.allclose(rows[0], want, rtol=1e-15, atol=0) and np.array_equal(rows[0], rows[1])
    B = FR.bound(pred, gt, None, occ)
    assert np.all(B["bound"][:, FR.COUNT_COLUMNS] == 0) and np.all(B["bound"][:, [COL["EPE_SUM"], COL["EPE_SQ_SUM"], COL["EPE_MAX"], COL["AE_SUM"]]] > 0)
    assert np.all(B["bound"][:, FR.SUM_COLUMNS] <= 1e-5 * np.maximum(rows[:, FR.SUM_COLUMNS], 1e-30))
    assert FR.clear_of_edges(pred, gt, None, occ)
    on_edge = np.array([[[[3.0]], [[0.0]]]], np.float32)
    assert not FR.clear_of_edges(on_edge, np.zeros_like(on_edge))                   # epe == outlier_abs
    assert not FR.clear_of_edges(np.zeros((1, 2, 1, 1), np.float32), np.array([[[[6.0]], [[8.0]]]], np.float32))      # |gt| == band0


# ---- the KITTI flow PNG ------------------------------------------------------------------------------------------------------------
def _kitti_case():
    rng = np.random.default_rng(5)
    flow = rng.integers(-512 * 64, 512 * 64, (2, 7, 9)).astype(np.float32) / 64
    valid = (rng.random((1, 7, 9)) < 0.7).astype(np.float32)
    return flow, valid


@pytest.mark.parametrize("filter_type", range(5))
def test_kitti_png_write_then_read(tmp_path, filter_type):
    flow, valid = _kitti_case()
    path = str(tmp_path / "k.png")
    evaluate.write_kitti_flow(path, flow, valid, filter_type=filter_type)
    raw = open(path, "rb").read()
    ihdr = raw[16:29]
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">IIBBBBB", ihdr) == (9, 7, 16, 2, 0, 0, 0)
    scan = zlib.decompress(raw[raw.index(b"IDAT") + 4:raw.index(b"IEND") - 8])
    assert {scan[y * (9 * 6 + 1)] for y in range(7)} == {filter_type}              # every scanline really carries this filter
    u, v = evaluate.read_kitti_flow(path)
    assert u.dtype == np.float32 and u.shape == (2, 7, 9) and v.shape == (1, 7, 9)
    assert np.array_equal(v, valid) and np.array_equal(u[:, valid[0] != 0], flow[:, valid[0] != 0])
    assert np.all(u[:, valid[0] == 0] == -512.0)                                    # an invalid pixel is written (0, 0, 0)
    gt, gv, go = evaluate.read_ground_truth(path)
    assert np.array_equal(gt, u) and np.array_equal(gv, v) and go is None
    from PIL import Image
    assert Image.open(path).size == (9, 7)                                          # another decoder accepts the file


def test_png_filter_type_may_change_from_line_to_line(tmp_path):
    """An encoder picks a filter per scanline; 37 lines that cycle through the five types, wider than tall and then taller than wide (the
    decoder walks anti-diagonals), decode to the image."""
    rng = np.random.default_rng(11)
    for h, w in ((37, 53), (53, 9)):
        rgb = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
        rgb[h // 2] = rgb[h // 2 - 1]                                               # a repeated line and a flat run: ties in the Paeth choice
        rgb[:, w // 2:w // 2 + 3] = 513
        lines, prev = [], bytearray(6 * w)
        for y in range(h):
            row = bytearray(rgb[y].astype(">u2").tobytes())
            lines.append(bytes([y % 5]) + bytes(evaluate._filter_row(y % 5, row, prev, 6)))
            prev = row
        path = str(tmp_path / f"mixed{h}.png")
        open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + evaluate._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0))
                               + evaluate._chunk(b"IDAT", zlib.compress(b"".join(lines)[:100])) + evaluate._chunk(b"IDAT", b"")
                               + evaluate._chunk(b"IEND", b""))
        with pytest.raises(Exception):                                              # a truncated stream is an error, not a short image
            evaluate.read_png16_rgb(path)
        data = zlib.compress(b"".join(lines))
        open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + evaluate._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0))
                               + evaluate._chunk(b"IDAT", data[:40]) + evaluate._chunk(b"tEXt", b"k\0v") + evaluate._chunk(b"IDAT", data[40:])
                               + evaluate._chunk(b"IEND", b""))                       # the stream split over two IDAT chunks
        assert np.array_equal(evaluate.read_png16_rgb(path), rgb)
    bad = b"\x05" + bytes(6)
    open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + evaluate._chunk(b"IHDR", struct.pack(">IIBBBBB", 1, 1, 16, 2, 0, 0, 0))
                           + evaluate._chunk(b"IDAT", zlib.compress(bad)) + evaluate._chunk(b"IEND", b""))
    with pytest.raises(ValueError, match="unknown filter type 5"):
        evaluate.read_png16_rgb(path)


def test_kitti_png_spelt_out_by_hand(tmp_path):
    """A 2 x 3 (H x W) file, every byte stated: row 0 unfiltered, row 1 with the Up filter (each byte minus the one above it)."""
    px = lambda r, g, b: struct.pack(">HHH", r, g, b)
    row0 = px(32768, 32768, 1) + px(32768 + 64, 32768 - 64, 1) + px(0, 0, 0)              # (0, 0) valid, (1, -1) valid, invalid
    row1 = px(32768 + 96, 32768 + 32, 1) + px(65535, 1, 7) + px(32768 - 640, 32768 + 6400, 1)
    up = bytes((b - a) & 255 for a, b in zip(row0, row1))
    scan = b"\x00" + row0 + b"\x02" + up
    assert scan[:7].hex() == "00800080000001" and up[:6].hex() == "006000200000"
    chunk = lambda kind, data: struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    raw = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", bytes.fromhex("00000003" "00000002" "10" "02" "00" "00" "00")) + chunk(b"IDAT", zlib.compress(scan)) \
        + chunk(b"IEND", b"")
    path = str(tmp_path / "hand.png")
    open(path, "wb").write(raw)
    flow, valid = evaluate.read_kitti_flow(path)
    assert flow[0].tolist() == [[0.0, 1.0, -512.0], [1.5, 32767 / 64, -10.0]]
    assert flow[1].tolist() == [[0.0, -1.0, -512.0], [0.5, -32767 / 64, 100.0]]
    assert valid[0].tolist() == [[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]]


def test_kitti_png_refuses_other_kinds_by_name(tmp_path):
    from PIL import Image
    p8 = str(tmp_path / "rgb8.png")
    Image.fromarray(np.zeros((4, 5, 3), np.uint8)).save(p8)
    with pytest.raises(ValueError, match=r"bit depth 8, colour type 2.*16-bit RGB"):
        evaluate.read_kitti_flow(p8)
    g16 = str(tmp_path / "grey16.png")
    Image.fromarray(np.zeros((4, 5), np.uint16)).save(g16)
    with pytest.raises(ValueError, match=r"bit depth 16, colour type 0"):
        evaluate.read_kitti_flow(g16)
    ok = str(tmp_path / "ok.png")
    evaluate.write_kitti_flow(ok, np.zeros((2, 4, 5)))
    raw = bytearray(open(ok, "rb").read())
    assert raw[28] == 0
    raw[28] = 1                                                                     # IHDR's interlace byte (the CRC is not what is checked first)
    bad = str(tmp_path / "adam7.png")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="interlaced PNG"):
        evaluate.read_kitti_flow(bad)
    with pytest.raises(ValueError, match="not a PNG"):
        evaluate.read_png16_rgb(os.path.join(ROOT, "tests", "golden", "chairs", "0000000-gt.npz"))
    with pytest.raises(ValueError, match="outside the format's range"):
        evaluate.write_kitti_flow(ok, np.full((2, 1, 1), 600.0))


# ---- ground truth and lists --------------------------------------------------------------------------------------------------------
def test_ground_truth_readers(tmp_path):
    rng = np.random.default_rng(2)
    flow = rng.standard_normal((2, 4, 6)).astype(np.float32)
    pf = str(tmp_path / "a.flo")
    flo.write_flo(pf, flow)
    got, valid, occ = evaluate.read_ground_truth(pf)
    assert np.array_equal(got, flow) and got.flags["C_CONTIGUOUS"] and valid is None and occ is None
    mask = (rng.random((4, 6)) < 0.5)
    pm = str(tmp_path / "m.npy")
    np.save(pm, mask.astype(np.uint8) * 255)
    assert np.array_equal(evaluate.read_ground_truth(pf, pm)[1], mask[np.newaxis].astype(np.float32))
    g = evaluate.read_ground_truth(pf, pm, "occ")
    assert g[1] is None and np.array_equal(g[2], mask[np.newaxis].astype(np.float32))
    from PIL import Image
    pi = str(tmp_path / "m.png")
    Image.fromarray(mask.astype(np.uint8) * 255).save(pi)
    assert np.array_equal(evaluate.read_ground_truth(pf, pi)[1], mask[np.newaxis].astype(np.float32))
    pz = str(tmp_path / "a.npz")
    np.savez(pz, flow=flow.transpose(1, 2, 0), valid=mask, occ=~mask)
    got, valid, occ = evaluate.read_ground_truth(pz, pm)
    assert np.array_equal(got, flow) and np.array_equal(valid[0], mask) and np.array_equal(occ[0], ~mask)
    np.savez(pz, flow=flow)
    assert np.array_equal(evaluate.read_ground_truth(pz)[0], flow)
    chairs = evaluate.read_ground_truth(os.path.join(ROOT, "tests", "golden", "chairs", "0000000-gt.npz"))[0]
    assert chairs.shape == (2, 384, 512) and chairs.dtype == np.float32
    with pytest.raises(ValueError, match="does not match the flow"):
        np.save(pm, np.zeros((3, 6)))
        evaluate.read_ground_truth(pf, pm)
    with pytest.raises(ValueError, match="must be .flo, .npz or a KITTI flow .png"):
        evaluate.read_ground_truth(str(tmp_path / "a.pfm"))
    with pytest.raises(ValueError, match="mask_as"):
        evaluate.read_ground_truth(pf, pm, "matched")


def test_list_parser():
    text = ["a0.png a1.png a.flo\n", "\n", "# a comment\n", "  b0.ppm\tb1.ppm  b.png  b_occ.png \n", "c0 c1 c.npz"]
    assert evaluate.parse_list(text) == [("a0.png", "a1.png", "a.flo", None), ("b0.ppm", "b1.ppm", "b.png", "b_occ.png"), ("c0", "c1", "c.npz", None)]
    assert evaluate.parse_list([]) == []
    with pytest.raises(ValueError, match=r"list line 2: expected `img0 img1 gt \[mask\]`, got 2 fields"):
        evaluate.parse_list(["a b c", "a b"])
    with pytest.raises(ValueError, match="list line 1: .* got 5 fields"):
        evaluate.parse_list(["a b c d e"])


# ---- the data-set loop with a stub predictor -----------------------------------------------------------------------------------------
STUB = r'''
import importlib.util, os, sys
import numpy as np
root, listfile, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import torch.distributed as dist
import flow_metrics_ref as FR
from flownet2_amd import evaluate, parallel
spec = importlib.util.spec_from_file_location("run_flownet_many", os.path.join(root, "scripts", "run_flownet_many.py"))
RM = importlib.util.module_from_spec(spec); spec.loader.exec_module(RM)
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    dist.init_process_group("gloo")
read_image = lambda path: np.load(path)
predict = lambda i0, i1: (i1 - i0)[:, :2] * np.float32(0.25)                      # a "net" whose output depends on its own pair alone
metrics = lambda pred, gt, valid, occ: evaluate.FlowMetrics(FR.ref64(pred, gt, valid, occ)[:-1])
with open(listfile) as f:
    entries = evaluate.parse_list(f)
for batch in (1, 2, 3):
    seen = []
    m = evaluate.evaluate(entries, RM.groups_of, read_image, predict, metrics, batch=batch, prefetch=1, mask_as="occ",
                          on_group=lambda ents, fm: seen.append(len(ents)))
    assert max(seen) <= batch and sum(seen) == len(parallel.shard(entries)) and (parallel.world() > 1 or batch == 1 or max(seen) > 1)
    if parallel.rank() == 0:
        open(out % batch, "w").write(m.to_json())
    else:
        assert m is None
if parallel.world() > 1:
    dist.barrier(); dist.destroy_process_group()
'''


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_evaluator_same_json_for_any_batch_and_world(tmp_path):
    rng = np.random.default_rng(9)
    lines, want = [], []
    for k in range(7):
        h, w = (6, 8) if k not in (3, 4) else (5, 7)                                # two image sizes: groups break where the size changes
        i0 = rng.integers(0, 256, (1, 3, h, w)).astype(np.float32)
        i1 = rng.integers(0, 256, (1, 3, h, w)).astype(np.float32)
        gt = (rng.standard_normal((2, h, w)) * 20).astype(np.float32)
        gt[0, 0, 0] = np.nan
        names = [str(tmp_path / f"{k}_{n}") for n in ("i0.npy", "i1.npy", "gt.npz", "occ.npy")]
        np.save(names[0], i0); np.save(names[1], i1)
        occ = rng.random((h, w)) < 0.3
        if k % 2:
            np.savez(names[2], flow=gt, valid=rng.random((h, w)) < 0.9)
        else:
            np.savez(names[2], flow=gt.transpose(1, 2, 0))
        np.save(names[3], occ)
        lines.append(" ".join(names[:3] + ([names[3]] if k in (1, 2, 6) else [])))
        want.append((i0, i1, gt))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    cmd = lambda world: [sys.executable, "-c", STUB, ROOT, str(lst), str(tmp_path / f"w{world}b%d.json")]
    procs = [subprocess.Popen(cmd(1), env=env)]                                     # one process, then two over gloo; each runs batch 1, 2, 3
    procs += [subprocess.Popen(cmd(2), env=dict(env, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    assert [p.wait(timeout=300) for p in procs] == [0, 0, 0]
    outs = {(world, batch): open(tmp_path / f"w{world}b{batch}.json", "rb").read() for world in (1, 2) for batch in (1, 2, 3)}
    first = outs[1, 1]
    assert all(v == first for v in outs.values()), [k for k, v in outs.items() if v != first]
    import json
    doc = json.loads(first)
    assert doc["columns"] == WANT_COLUMNS and len(doc["rows"]) == 7 and doc["summary"]["samples"] == 7
    # list order: row k is pair k's (its pixel count is its own plane's, minus the NaN and the masked pixels)
    assert [r[COL["VALID"]] + r[COL["NONFINITE"]] <= (35 if k in (3, 4) else 48) - 1 for k, r in enumerate(doc["rows"])] == [True] * 7
    rows = np.array(doc["rows"])
    i0, i1, gt = want[5]
    alone = FR.ref64((i1 - i0)[:, :2] * np.float32(0.25), gt[np.newaxis], np.load(str(tmp_path / "5_gt.npz"))["valid"][np.newaxis, np.newaxis])
    assert np.array_equal(rows[5], alone[0])
    assert rows[1, COL["OCC_COUNT"]] > 0 and rows[0, COL["OCC_COUNT"]] == 0 and doc["summary"] == evaluate.json_ready(FlowMetrics(rows).summary())
