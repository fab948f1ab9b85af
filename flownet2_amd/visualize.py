"""Flow visualisation: the pictures of the visualisation kernels (csrc/flow_visualize.hip, include/flownet2_hip_flow_visualize.h) and the
way to a file.  flow_to_color and flow_error_map are functional's; color_wheel is the flow field whose colouring is the legend; write_png /
read_png8 are an 8-bit PNG writer and its reading counterpart on zlib alone -- no image library is needed to get a picture out.

write_png is a function of the array: filter 0 on every line, one IDAT chunk, zlib at a fixed level, no time stamp or text chunk.  So the
same array gives the same file bytes, and two runs can be compared with cmp.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

from .evaluate import _PNG_MAGIC, _chunk, _unfilter

_ZLIB_LEVEL = 6
UNKNOWN_FLOW = 1e10      # the .flo convention: a value above 1e9 is unknown flow


def flow_to_color(flow, max_flow=None, norm="sample"):
    """functional.flow_to_color: the Middlebury colour coding of a device flow [N,2,H,W] -> uint8 [N,H,W,3] on the device."""
    from . import functional
    return functional.flow_to_color(flow, max_flow=max_flow, norm=norm)


def flow_error_map(pred, gt, valid=None, occ=None, abs_thresh=3.0, rel_thresh=0.05):
    """functional.flow_error_map: the KITTI-style error image of device flows [N,2,H,W] -> uint8 [N,H,W,3] on the device."""
    from . import functional
    return functional.flow_error_map(pred, gt, valid=valid, occ=occ, abs_thresh=abs_thresh, rel_thresh=rel_thresh)


def color_wheel(size):
    """The legend as a flow field: float32 [1,2,size,size] with u = x - c, v = y - c for c = (size - 1) / 2 inside the disc of radius c
    and the .flo unknown-flow value outside it.  Its colouring under per-sample normalisation is the colour wheel: white at the centre,
    full saturation on the rim, black outside."""
    size = int(size)
    if size < 1:
        raise ValueError(f"color_wheel: size must be positive, got {size}")
    c = np.float32(size - 1) / np.float32(2)
    v, u = np.meshgrid(np.arange(size, dtype=np.float32) - c, np.arange(size, dtype=np.float32) - c, indexing="ij")
    inside = u.astype(np.float64) ** 2 + v.astype(np.float64) ** 2 <= float(c) ** 2
    unknown = np.float32(UNKNOWN_FLOW)
    return np.stack([np.where(inside, u, unknown), np.where(inside, v, unknown)])[np.newaxis].astype(np.float32)


def write_png(path, array):
    """uint8 [H,W,3] (RGB) or [H,W] (grey) -> a non-interlaced 8-bit PNG; a device tensor is brought to the host first."""
    if hasattr(array, "detach"):
        array = array.detach().cpu().numpy()
    a = np.asarray(array)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.size == 0:
        raise ValueError(f"write_png: need uint8 [H,W,3] or [H,W], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    lines = np.zeros((h, 1 + a.size // h), np.uint8)            # filter type 0 in front of every scanline
    lines[:, 1:] = a.reshape(h, -1)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(lines.tobytes(), _ZLIB_LEVEL)) + _chunk(b"IEND", b""))


def read_png8(path):
    """A non-interlaced 8-bit RGB or grey PNG -> uint8 [H,W,3] or [H,W] (all five filter types; every chunk's CRC is checked).  Anything
    else is refused by name."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, head, ended = 8, [], None, False
    while pos + 12 <= len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or data[pos + 8 + n:pos + 12 + n] != struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: chunk {kind!r} is cut short or fails its CRC")
        pos += 12 + n
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
    if head is None or not ended:
        raise ValueError(f"{path}: no IHDR or no IEND chunk")
    w, h, depth, colour, _, _, interlace = head
    if depth != 8 or colour not in (0, 2):
        raise ValueError(f"{path}: bit depth {depth}, colour type {colour}: read_png8 reads 8-bit grey (0) or RGB (2)")
    if interlace != 0:
        raise ValueError(f"{path}: interlaced PNG (Adam7) is not supported")
    bpp = 3 if colour == 2 else 1
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (w * bpp + 1):
        raise ValueError(f"{path}: {len(raw)} bytes of image data, expected {h * (w * bpp + 1)}")
    out = _unfilter(raw, h, w, bpp)
    return out if bpp == 3 else out[:, :, 0]
