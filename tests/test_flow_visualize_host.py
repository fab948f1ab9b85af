"""Flow visualisation, everything that needs no GPU: the header and its binding, the host-only entry point and the refusals of
include/flownet2_hip_flow_visualize.h, the colour wheel and the restatements (flow_visualize_ref) on cases whose bytes are known by hand,
the bounds where they must be 0, the PNG writer and reader, and the legend."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import flow_visualize_ref as VR
from flownet2_amd import _lib, visualize
from flownet2_amd import functional as Fn

SAMPLE, BATCH, FIXED = VR.NORM["SAMPLE"], VR.NORM["BATCH"], VR.NORM["FIXED"]


# ---- the header, the binding, sizes and refusals ----------------------------------------------------------------------------------------
def test_header_declares_exactly_what_the_library_exports():
    with open(os.path.join(_lib.INCLUDE_DIR, "flownet2_hip_flow_visualize.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    want = ["fn2_flow_visualize_sizes", "fn2_flow_color", "fn2_flow_error_map"]
    assert re.findall(r"\b(fn2_\w+)\s*\(", body) == want and list(_lib.FLOW_VISUALIZE_EXPORTS) == want
    functions, _, constants = _lib.parse_header(text)                               # includable, and parsable, on its own
    assert list(functions) == want and constants == _lib.FLOW_VISUALIZE_CONSTANTS
    symbols = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode().split()
    assert sorted(s for s in symbols if s.startswith(("fn2_flow_visualize", "fn2_flow_color", "fn2_flow_error_map"))) == sorted(want)
    L = _lib.lib()
    for name in want:
        restype, argtypes = _lib.FLOW_VISUALIZE_PROTOTYPES[name]
        assert restype is C.c_int and getattr(L, name).argtypes == argtypes
    color, error = _lib.FLOW_VISUALIZE_PROTOTYPES["fn2_flow_color"][1], _lib.FLOW_VISUALIZE_PROTOTYPES["fn2_flow_error_map"][1]
    assert len(color) == 11 and color[5] is C.c_float and color[6] is C.c_void_p and color[9] is C.c_size_t      # max_flow, rgb, workspace_bytes
    assert len(error) == 11 and error[7] is C.c_float and error[9] is C.c_void_p
    # the enum reaches the binding through the parser, in a table of its own; the other tables keep their sizes
    assert _lib.FLOW_VISUALIZE_CONSTANTS == dict(FN2_FLOW_COLOR_NORM_SAMPLE=0, FN2_FLOW_COLOR_NORM_BATCH=1, FN2_FLOW_COLOR_NORM_FIXED=2)
    assert len(_lib.CONSTANTS) == 49 and len(_lib.FLOW_METRICS_CONSTANTS) == 16 and len(_lib.FLOW_CONSISTENCY_CONSTANTS) == 13
    assert not set(want) & (set(_lib.PROTOTYPES) | set(_lib.FLOW_CONSISTENCY_PROTOTYPES))


def test_sizes_are_one_float_per_workgroup():
    planes = [(1, 1), (5, 7), (8, 16), (32, 32), (32, 33), (67, 131), (320, 448), (384, 768), (1024, 2048)]
    per_sample = [VR.sizes(1, h, w) for h, w in planes]
    assert per_sample == [4 * VR.chunks(h, w) for h, w in planes] and per_sample[3] == 4 and per_sample[4] == 8
    assert per_sample[-1] == per_sample[-2] == 4 * 128                              # at most 128 partial maxima per sample
    for (h, w), one in zip(planes[:-1], per_sample):
        for n in (2, 3, 17):
            assert VR.sizes(n, h, w) == n * one
    L = _lib.lib()
    assert L.fn2_flow_visualize_sizes(2, 5, 7, None) == VR.OK                       # the out-pointer may be NULL
    nbytes = C.c_size_t(77)
    for _, shape, _ in VR.BAD_SHAPES:
        assert L.fn2_flow_visualize_sizes(shape[0], shape[2], shape[3], C.byref(nbytes)) == VR.INVALID and nbytes.value == 77


def test_every_host_refusal_writes_nothing_and_names_the_argument():
    """Refusals are decided before any launch, so they need no device: the pointers are host buffers that nobody dereferences."""
    ws_bytes = VR.sizes(2, 5, 7)
    buf = lambda n: (C.c_ubyte * n)(*([0x5A] * n))
    bufs = {k: buf(n) for k, n in (("flow", 560), ("gt", 560), ("valid", 280), ("occ", 280), ("rgb", 210), ("maxrad", 8), ("ws", ws_bytes))}
    cases = VR.refusals(bufs["flow"], bufs["gt"], bufs["valid"], bufs["occ"], bufs["rgb"], bufs["maxrad"], bufs["ws"], ws_bytes)
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels) == 5 + 16 + 5 + 6 + 4
    for label, want, prefix, names, thunk in cases:
        assert thunk() == want, label
        text = _lib.lib().fn2_last_error_string().decode()
        assert text.startswith(prefix) and names in text, (label, text)
    for k, b in bufs.items():
        assert bytes(b) == b"\x5a" * len(b), k


def test_python_refusals_need_no_device():
    z = torch.zeros(1, 2, 3, 4)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.flow_to_color(z)
    with pytest.raises(ValueError, match="no CPU path"):
        Fn.flow_error_map(z, z)
    with pytest.raises(RuntimeError, match="not differentiable"):
        Fn.flow_to_color(z.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="not differentiable"):
        Fn.flow_error_map(z, z.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="'sample' or 'batch'"):
        Fn.flow_to_color(z, norm="fixed")
    import flownet2_amd
    assert flownet2_amd.flow_to_color is Fn.flow_to_color and flownet2_amd.flow_error_map is Fn.flow_error_map
    assert "flow_to_color" in flownet2_amd.__all__ and "flow_error_map" in flownet2_amd.__all__


# ---- the wheel and the restatements by hand --------------------------------------------------------------------------------------------
def test_wheel_check_points():
    w = VR.WHEEL
    assert w.shape == (55, 3) and w.min() == 0 and w.max() == 255
    want = {0: (255, 0, 0), 15: (255, 255, 0), 21: (0, 255, 0), 25: (0, 255, 255), 36: (0, 0, 255), 49: (255, 0, 255), 54: (255, 0, 43)}
    for k, rgb in want.items():
        assert tuple(w[k]) == rgb, k
    assert tuple(w[1]) == (255, 17, 0) and tuple(w[16]) == (213, 255, 0) and tuple(w[26]) == (0, 232, 255) and tuple(w[37]) == (19, 0, 255)


def _flow(u, v, shape=(1, 2, 2, 3)):
    f = np.zeros(shape, np.float32)
    f[:, 0], f[:, 1] = u, v
    return f


def test_colour_restatement_by_hand():
    white, black = [255, 255, 255], [0, 0, 0]
    rgb, maxrad = VR.color32(_flow(0.0, 0.0))
    assert rgb.shape == (1, 2, 3, 3) and rgb.dtype == np.uint8 and np.all(rgb == 255) and maxrad.tolist() == [1.0]      # a maximum of 0 is 1
    assert np.all(VR.color32(_flow(-0.0, -0.0))[0] == 255)
    # the four axes at the maximum: rn == 1 exactly, so the byte is the wheel's.  u > 0: atan2f(-0, -u) = -pi, entry 0; v < 0: a = 1/2,
    # fk = 40.5, between entries 40 (78, 0, 255) and 41 (98, 0, 255); u < 0: a = 0, fk = 27: entry 27 (0, 209, 255); v > 0: fk = 13.5
    assert VR.color32(_flow(2.0, 0.0))[0][0, 0, 0].tolist() == [255, 0, 0]
    assert VR.color32(_flow(0.0, -2.0))[0][0, 0, 0].tolist() == [88, 0, 255]
    assert VR.color32(_flow(-2.0, 0.0))[0][0, 0, 0].tolist() == [0, 209, 255]
    assert VR.color32(_flow(0.0, 2.0))[0][0, 0, 0].tolist() == [255, 229, 0]       # entries 13 (255, 221, 0) and 14 (255, 238, 0)
    # the seam: v = -0.0f sends +0 to atan2f, +pi, entry 54
    assert VR.color32(_flow(2.0, -0.0))[0][0, 0, 0].tolist() == [255, 0, 43]
    # half the maximum: half way to white; beyond a fixed maximum: three quarters of the hue
    f = _flow(2.0, 0.0)
    f[0, 0, 0, 0] = 1.0
    rgb, maxrad = VR.color32(f)
    assert rgb[0, 0, 0].tolist() == [255, 127, 127] and rgb[0, 0, 1].tolist() == [255, 0, 0] and maxrad.tolist() == [2.0]
    rgb, maxrad = VR.color32(f, FIXED, 1.5)
    assert rgb[0, 0, 0].tolist() == [255, 85, 85] and rgb[0, 0, 1].tolist() == [191, 0, 0] and maxrad.tolist() == [1.5]
    # unknown flow is black and takes no part in the maximum; the batch shares the largest maximum
    g = np.concatenate([f, _flow(0.0, 4.0)])
    g[0, 1, 1, 2] = np.nan
    g[0, 0, 1, 1] = 1e10
    g[1, 0, 0, 0] = -np.inf
    rgb, maxrad = VR.color32(g)
    assert rgb[0, 1, 2].tolist() == black and rgb[0, 1, 1].tolist() == black and rgb[1, 0, 0].tolist() == black and maxrad.tolist() == [2.0, 4.0]
    assert rgb[0, 0, 1].tolist() == [255, 0, 0] and rgb[1, 1, 1].tolist() == [255, 229, 0]
    rgb, maxrad = VR.color32(g, BATCH)
    assert maxrad.tolist() == [4.0, 4.0] and rgb[0, 0, 1].tolist() == [255, 127, 127] and rgb[0, 1, 2].tolist() == black
    nothing = np.full((1, 2, 2, 2), np.nan, np.float32)
    rgb, maxrad = VR.color32(nothing)
    assert not rgb.any() and maxrad.tolist() == [1.0]
    assert white == VR.color32(_flow(0.0, 0.0), FIXED, 3.0)[0][0, 0, 0].tolist()


def test_colour_bounds_are_zero_where_the_arithmetic_is_exact():
    # zero flow: every channel exact; a constant flow: every pixel is the maximum pixel, rn exact; a saturated channel exact everywhere
    b = VR.color_bounds(_flow(0.0, 0.0))
    assert not b["in"][1].any() and np.all(b["in"][0] == 255) and not b["either"].any()
    f = VR.smooth_flow((2, 2, 16, 64), 11)
    f[0, :, 3, 5] = 0
    f[1, :, 0, 0] = (40.0, 9.0)                                                      # one pixel ten times the rest: the unique maximum
    for norm, max_flow in ((SAMPLE, None), (BATCH, None), (FIXED, 4.0)):
        b = VR.color_bounds(f, norm, max_flow)
        out, delta = b["in"]
        assert not delta[0, 3, 5].any() and np.all(out[0, 3, 5] == 255)
        k0 = np.floor((np.arctan2(-f[:, 1].astype(np.float64), -f[:, 0].astype(np.float64)) / np.pi + 1) * 27).astype(int)
        inner = (k0 >= 1) & (k0 <= 13)                                               # RY: R is 255 at both nodes, B is 0 at both
        assert inner.sum() > 100 and not delta[inner][:, 0].any() and np.all(out[inner][:, 0] == 255)
        assert 0 < delta.max() < 5e-3 and 0 < b["over"][1].max() < 5e-3
        if norm != FIXED:
            assert b["rn"][1, 0, 0] == 1.0 and b["d_rn"][1, 0, 0] == 0 and not b["either"].any() and b["rn"].max() == 1.0
            assert (b["d_rn"][0] > 0).sum() == 16 * 64 - 1 if norm == BATCH else b["d_rn"][0].min() == 0
        else:
            assert (b["rn"] > 1).any() and b["d_rn"][1, 0, 0] > 0
    # the restatement passes its own check, with few values left loose
    for norm, max_flow in ((SAMPLE, None), (BATCH, None), (FIXED, 4.0)):
        wrong, loose, delta = VR.color_check(VR.color32(f, norm, max_flow)[0], f, norm, max_flow)
        assert wrong == 0 and loose <= 0.03 and delta < 5e-3
    off = VR.color32(f)[0].copy()
    off[1, 2, 3, 1] ^= 2
    assert VR.color_check(off, f)[0] == 1


def test_error_map_restatement_by_hand():
    gt = _flow(30.0, 40.0, (1, 2, 1, 12))                                           # |gt| = 50: the relative term is epe / 2.5, the absolute one epe / 3
    pred = gt.copy()
    epes = [0.0, 0.125, 0.1875, 0.5, 1.0, 2.0, 2.5, 2.75, 6.0, 12.0, 30.0, 48.0]     # n = epe / 3: the absolute term is the smaller one
    pred[0, 0, 0] += np.array(epes, np.float32)
    rgb = VR.error_map32(pred, gt)
    bins = [0, 0, 1, 2, 3, 4, 4, 4, 6, 7, 8, 9]                                      # 0.0417 | 0.0625 (an edge: lo <= n) | ... | 10 | 16 (an edge)
    assert rgb.shape == (1, 1, 12, 3) and [tuple(c) for c in rgb[0, 0]] == [tuple(VR.BIN_COLORS[b]) for b in bins]
    assert tuple(VR.BIN_COLORS[5]) == (254, 224, 144) and tuple(VR.BIN_COLORS[4]) == (224, 243, 248)
    small = _flow(3.0, 4.0, (1, 2, 1, 3))                                            # |gt| = 5: the relative term is epe / 0.25
    p2 = small.copy()
    p2[0, 0, 0] += np.array([0.75, 3.0, 6.0], np.float32)                            # min(0.25, 3) | min(1, 12) | min(2, 24)
    assert [tuple(c) for c in VR.error_map32(p2, small)[0, 0]] == [tuple(VR.BIN_COLORS[b]) for b in (3, 5, 6)]
    zero = _flow(0.0, 0.0, (1, 2, 1, 3))                                             # mag == 0: the absolute term alone
    p3 = zero.copy()
    p3[0, 1, 0] = (0.0, 1.5, 60.0)
    assert [tuple(c) for c in VR.error_map32(p3, zero)[0, 0]] == [tuple(VR.BIN_COLORS[b]) for b in (0, 4, 9)]
    # black without ground truth, the last bin for a prediction that is not a number, halved under occ
    g4, p4 = gt[:, :, :, :6].copy(), gt[:, :, :, :6].copy()
    g4[0, 0, 0, 0], g4[0, 1, 0, 1], p4[0, 0, 0, 2], p4[0, 1, 0, 3] = np.nan, 1e10, np.nan, -np.inf
    valid = np.ones((1, 1, 1, 6), np.float32)
    valid[0, 0, 0, 4] = 0
    occ = np.zeros((1, 1, 1, 6), np.float32)
    occ[0, 0, 0, 3:] = 1
    rgb = VR.error_map32(p4, g4, valid, occ)
    assert [tuple(c) for c in rgb[0, 0]] == [(0, 0, 0), (0, 0, 0), (165, 0, 38), (82, 0, 19), (0, 0, 0), (24, 27, 74)]
    assert VR.error_check(rgb, p4, g4, valid, occ) == (0, 0.0)
    wrong, loose = VR.error_check(VR.error_map32(pred, gt), pred, gt)
    assert wrong == 0 and loose == 4 / 12                                            # the four pixels on an edge may take either bin
    for shape in ((3, 2, 7, 67), (2, 2, 36, 60)):
        case = VR.error_case(shape, 5)
        wrong, loose = VR.error_check(VR.error_map32(*case), *case)
        assert wrong == 0 and loose <= 0.03


# ---- the PNG writer and reader, the legend ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5, 3), (7, 67, 3)])
def test_png_round_trip(tmp_path, shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    p1, p2 = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    visualize.write_png(p1, a)
    visualize.write_png(p2, a.copy())
    data = open(p1, "rb").read()
    assert data == open(p2, "rb").read()                                            # a function of the array
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[-12:] == struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND"))
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", data[16:29])
    assert data[12:16] == b"IHDR" and (w, h, depth, colour, comp, filt, interlace) == (shape[1], shape[0], 8, 2 if len(shape) == 3 else 0, 0, 0, 0)
    back = visualize.read_png8(p1)
    assert back.dtype == np.uint8 and back.shape == shape and np.array_equal(back, a)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(p1)), a)                            # another decoder reads it


def test_png_refusals_and_other_filters(tmp_path):
    path = str(tmp_path / "x.png")
    for bad in (np.zeros((2, 2), np.float32), np.zeros((2, 2, 4), np.uint8), np.zeros((2,), np.uint8), np.zeros((0, 3), np.uint8)):
        with pytest.raises(ValueError, match="write_png"):
            visualize.write_png(path, bad)
    a = np.random.default_rng(1).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    from PIL import Image
    Image.fromarray(a).save(path, optimize=True)                                    # an encoder that picks filters per line
    assert np.array_equal(visualize.read_png8(path), a)
    visualize.write_png(path, a)
    data = bytearray(open(path, "rb").read())
    data[40] ^= 1
    open(path, "wb").write(bytes(data))
    with pytest.raises(ValueError, match="CRC"):
        visualize.read_png8(path)
    visualize.write_png(path, torch.from_numpy(a))                                  # a tensor goes in as it is
    assert np.array_equal(visualize.read_png8(path), a)


def test_the_legend():
    flow = visualize.color_wheel(65)
    assert flow.shape == (1, 2, 65, 65) and flow.dtype == np.float32
    rgb, maxrad = VR.color32(flow)
    assert maxrad.tolist() == [32.0]
    assert rgb[0, 32, 32].tolist() == [255, 255, 255]                               # the centre: zero flow
    y, x = np.mgrid[0:65, 0:65]
    outside = (x - 32) ** 2 + (y - 32) ** 2 > 32 ** 2
    assert np.all(flow[0][:, outside] > 1e9) and not rgb[0][outside].any() and rgb[0][~outside].max(-1).min() == 255
    assert flow[0, 0, 32, 64] == 32 and flow[0, 1, 32, 64] == 0 and rgb[0, 32, 64].tolist() == [255, 0, 0]      # the rim at u > 0: red
    assert rgb[0, 32, 48].tolist() == [255, 127, 127]                               # half way out
    seam = flow.copy()
    seam[0, 1, 32, 33:] = -0.0                                                      # u > 0, v = -0.0f: the other side of the seam, still red
    assert VR.color32(seam)[0][0, 32, 64].tolist() == [255, 0, 43]
    assert rgb[0, 0, 32].tolist() == [88, 0, 255] and rgb[0, 64, 32].tolist() == [255, 229, 0] and rgb[0, 32, 0].tolist() == [0, 209, 255]
    with pytest.raises(ValueError, match="size"):
        visualize.color_wheel(0)


# ---- the runners' refusals -------------------------------------------------------------------------------------------------------------
def test_batch_normalisation_is_refused_when_the_list_is_sharded(tmp_path):
    """--color-norm batch makes a picture depend on the group its pair fell into: with more than one process only --color-max may decide.
    The refusal comes from the argument parser, before any device or process group is touched."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    listfile = tmp_path / "list.txt"
    listfile.write_text("")
    cmd = [sys.executable, os.path.join(root, "scripts", "run_flownet_many.py"), str(listfile), "--color", "--color-norm", "batch"]
    p = subprocess.run(cmd, env=dict(os.environ, WORLD_SIZE="2"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 2 and b"--color-norm batch" in p.stdout and b"--color-max" in p.stdout
    help_text = subprocess.run(cmd[:2] + ["--help"], stdout=subprocess.PIPE, timeout=300).stdout.decode()
    assert "refused with more than one process unless --color-max" in " ".join(help_text.split())
