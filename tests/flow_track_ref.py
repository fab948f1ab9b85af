"""Point-trajectory references for the tests: the arithmetic of include/flownet2_hip_flow_track.h op by op in NumPy float32 (ref32: tracks,
positions, states and steps, which the kernel must equal bit for bit, and the rows; reseed32), a float64 evaluation of DISP_SUM with an
error bound from the operation count (disp_sum_bound), seeded inputs (make_sequence) and the raw C ABI calls.  No file of the reference
tree is read, and no tolerance here comes from the kernel's output.

ref32 rounds once per NumPy operation: every array is float32 and every scalar an np.float32, so a + b, a * b and np.sqrt (correctly
rounded) are the kernel's operations (which are compiled without contraction) in the kernel's association.

The bound on DISP_SUM, with U = 2^-24 (every fp32 operation: half an ulp, relative U; sqrtf is correctly rounded, so U as well).  Starred
values are the float64 evaluation's.  The first and the last position of a point are float32 values that the tracker CHOSE (they are
compared bit for bit on their own), so the float64 evaluation starts from them, and which points are alive is decided by the states.

  dx = x - x0                                  d_dx = U |dx*|
  dx dx                                        d_p = (2 |dx*| d_dx + d_dx^2) (1 + U) + U dx*^2
  s = dx dx + dy dy                            d_s = (d_px + d_py) (1 + U) + U s*
  d = sqrtf(s)                                 |sqrt(s) - sqrt(s*)| <= min(d_s / sqrt(s*), sqrt(d_s)) =: d_r;  d_e = d_r + U (d* + d_r)
  DISP_SUM                                     sum of d_e over the alive points
  the fp64 additions: P of them, relative 2^-53 each on non-negative terms                   + P 2^-53 (sum*)
A few multiples of the smallest subnormal (TINY) cover products that underflow."""
import ctypes as C

import numpy as np

from flownet2_amd import _lib
from flownet2_amd.evaluate import TRACK_COL as COL, TRACK_K as K, TRACK_STOP as STOP

U = 2.0 ** -24
TINY = 16 * 2.0 ** -149
OK, INVALID, WORKSPACE = 0, -1, -3
ALPHA = (0.01, 0.5)
BOUNDARY = 8                                                                         # FN2_FLOW_CONSISTENCY_FLAG_BOUNDARY, the default stop_mask
F = np.float32
LIMIT = F(1e9)
NF, OUT, INC, MARK = STOP["NONFINITE"], STOP["OUTSIDE"], STOP["INCONSISTENT"], STOP["MARKED"]


def _ok(t):
    with np.errstate(invalid="ignore"):
        return np.abs(t) <= LIMIT                                                   # False for NaN and +-Inf


def _inside(x, y, H, W):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (y >= 0) & (x < F(W)) & (y < F(H))


def _sample(flow, x, y, live):
    """The bilinear value (u, v) of flow [2,H,W] at the points (x, y) where `live` (those have passed the inside test); the others are
    sampled at (0, 0) and their value is not used.  Step 1 of the header."""
    _, H, W = flow.shape
    x, y = np.where(live, x, F(0)), np.where(live, y, F(0))
    ixL, iyT = np.minimum(x.astype(np.int32), W - 1), np.minimum(y.astype(np.int32), H - 1)      # truncation of a value in [0, W)
    ixR, iyB = np.minimum(ixL + 1, W - 1), np.minimum(iyT + 1, H - 1)
    assert ixL.min(initial=0) >= 0 and iyT.min(initial=0) >= 0
    al, be = x - ixL.astype(F), y - iyT.astype(F)
    one = F(1)
    wTL, wTR, wBL, wBR = (one - al) * (one - be), al * (one - be), (one - al) * be, al * be
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in (0, 1):
            p = flow[c]
            out.append(((wTL * p[iyT, ixL] + wTR * p[iyT, ixR]) + wBL * p[iyB, ixL]) + wBR * p[iyB, ixR])
    assert out[0].dtype == F and al.dtype == F
    return out


def ref32(fw, bw, points, state=None, stop=None, stop_mask=BOUNDARY, alpha=ALPHA):
    """fw, bw float32 [N,T,2,H,W], points float32 [N,2,P], state uint8 [N,P] or None, stop uint8 [N,T,1,H,W] or None -> dict of tracks
    [N,T+1,2,P], points_out [N,2,P], state uint8 [N,P], steps int32 [N,P], rows float64 [N + 1, K]."""
    fw, bw, points = np.ascontiguousarray(fw, F), np.ascontiguousarray(bw, F), np.ascontiguousarray(points, F)
    N, T, _, H, W = fw.shape
    P = points.shape[2]
    a1, a2 = F(alpha[0]), F(alpha[1])
    given = np.zeros((N, P), np.uint8) if state is None else np.asarray(state, np.uint8)
    tracks = np.full((N, T + 1, 2, P), np.nan, F)
    tracks[:, 0] = points
    out_p, out_s, out_n = points.copy(), given.copy(), np.zeros((N, P), np.int32)
    for n in range(N):
        x, y = points[n, 0].copy(), points[n, 1].copy()
        st = given[n].astype(np.int32)
        fresh = st == 0
        st = np.where(fresh & ~(_ok(x) & _ok(y)), NF, st)
        st = np.where(fresh & (st == 0) & ~_inside(x, y, H, W), OUT, st)
        steps = np.zeros(P, np.int32)
        for t in range(T):
            live = st == 0
            au, av = _sample(fw[n, t], x, y, live)
            s1 = live & ~(_ok(au) & _ok(av))
            s2 = np.zeros(P, bool)
            if stop is not None:
                xs, ys = np.where(live, x, F(0)), np.where(live, y, F(0))
                jx = np.minimum((xs + F(0.5)).astype(np.int32), W - 1)
                jy = np.minimum((ys + F(0.5)).astype(np.int32), H - 1)
                s2 = live & ~s1 & ((stop[n, t, 0][jy, jx].astype(np.uint32) & np.uint32(stop_mask)) != 0)
            go = live & ~s1 & ~s2
            with np.errstate(invalid="ignore", over="ignore"):
                x2, y2 = x + au, y + av
            s3 = go & ~_inside(x2, y2, H, W)
            go = go & ~s3
            bu, bv = _sample(bw[n, t], x2, y2, go)
            s4 = go & ~(_ok(bu) & _ok(bv))
            go = go & ~s4
            with np.errstate(invalid="ignore", over="ignore"):
                su, sv = au + bu, av + bv
                s = su * su + sv * sv
                m = (au * au + av * av) + (bu * bu + bv * bv)
                s5 = go & (s > a1 * m + a2)
            assert s.dtype == F and m.dtype == F and x2.dtype == F
            go = go & ~s5
            st = np.where(s1 | s4, NF, np.where(s2, MARK, np.where(s3, OUT, np.where(s5, INC, st))))
            x, y = np.where(go, x2, x), np.where(go, y2, y)
            steps += go
            tracks[n, t + 1, 0] = np.where(go, x, F(np.nan))
            tracks[n, t + 1, 1] = np.where(go, y, F(np.nan))
        out_p[n, 0], out_p[n, 1], out_s[n], out_n[n] = x, y, st.astype(np.uint8), steps
    return dict(tracks=tracks, points_out=out_p, state=out_s, steps=out_n, rows=rows_of(points, given, out_p, out_s, out_n))


def _disp32(points, points_out, state):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = points_out[:, 0] - points[:, 0], points_out[:, 1] - points[:, 1]
        d = np.sqrt(dx * dx + dy * dy)
    assert d.dtype == F
    return np.where(state == 0, d, F(0))


def rows_of(points, given, points_out, state, steps):
    """[N + 1, K] float64 rows: exact counts, DISP_SUM as the float64 sum of the float32 displacements, DISP_MAX exact."""
    N, P = state.shape
    rows = np.zeros((N + 1, K), np.float64)
    rows[:N, COL["POINTS"]] = P
    rows[:N, COL["ALIVE"]] = (state == 0).sum(1)
    for name in ("NONFINITE", "OUTSIDE", "INCONSISTENT", "MARKED"):
        rows[:N, COL[name]] = ((state == STOP[name]) & (given == 0)).sum(1)
    rows[:N, COL["STEPS_SUM"]] = steps.sum(1)
    rows[:N, COL["STEPS_MAX"]] = steps.max(1)
    d = _disp32(points, points_out, state).astype(np.float64)
    rows[:N, COL["DISP_SUM"]] = d.sum(1)
    rows[:N, COL["DISP_MAX"]] = d.max(1)
    rows[N] = rows[:N].sum(0)
    for name in ("STEPS_MAX", "DISP_MAX"):
        rows[N, COL[name]] = rows[:N, COL[name]].max()
    return rows


EXACT_COLUMNS = [COL[n] for n in ("POINTS", "ALIVE", "NONFINITE", "OUTSIDE", "INCONSISTENT", "MARKED", "STEPS_SUM", "STEPS_MAX", "DISP_MAX")]


def disp_sum_bound(points, points_out, state):
    """In float64 from the float32 positions (module docstring): (DISP_SUM* [N + 1], bound on |computed - DISP_SUM*| [N + 1])."""
    alive = np.asarray(state) == 0
    N, P = alive.shape
    p0 = np.where(alive[:, None], points, 0).astype(np.float64)
    p1 = np.where(alive[:, None], points_out, 0).astype(np.float64)
    d_p, s = [], 0.0
    for c in (0, 1):
        dx = p1[:, c] - p0[:, c]
        d_dx = U * np.abs(dx)
        d_p.append((2 * np.abs(dx) * d_dx + d_dx ** 2) * (1 + U) + U * dx ** 2 + TINY)
        s = s + dx ** 2
    d_s = (d_p[0] + d_p[1]) * (1 + U) + U * s
    d = np.sqrt(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        d_r = np.minimum(np.where(s > 0, d_s / np.where(s > 0, d, 1.0), np.inf), np.sqrt(d_s))
    d_e = d_r + U * (d + d_r) + TINY
    ref, bnd = np.where(alive, d, 0.0).sum(1), np.where(alive, d_e, 0.0).sum(1)
    bnd = bnd + P * 2.0 ** -53 * ref
    return np.append(ref, ref.sum()), np.append(bnd, bnd.sum() + N * 2.0 ** -53 * ref.sum())


def cells(H, W, cell):
    return -(-H // cell), -(-W // cell)


def reseed32(points, state, size, cell):
    """fn2_flow_track_reseed restated: (points, state, born) as new arrays."""
    H, W = size
    ch, cw = cells(H, W, cell)
    points, state = np.array(points, F), np.array(state, np.uint8)
    N, _, P = points.shape
    assert P == ch * cw
    born = np.zeros((N, P), np.uint8)
    half = F(0.5) * F(cell - 1)
    for n in range(N):
        x, y = points[n, 0], points[n, 1]
        live = (state[n] == 0) & _ok(x) & _ok(y) & _inside(x, y, H, W)
        covered = np.zeros(P, bool)
        cx = np.where(live, x, F(0)).astype(np.int32) // cell
        cy = np.where(live, y, F(0)).astype(np.int32) // cell
        covered[(cy * cw + cx)[live]] = True
        fill = (state[n] != 0) & ~covered
        slot = np.arange(P)
        gx = np.minimum((slot % cw * cell).astype(F) + half, F(W - 1))
        gy = np.minimum((slot // cw * cell).astype(F) + half, F(H - 1))
        points[n, 0], points[n, 1] = np.where(fill, gx, x), np.where(fill, gy, y)
        state[n] = np.where(fill, 0, state[n])
        born[n] = fill
    return points, state, born


def grid(N, H, W, cell=1):
    return reseed32(np.zeros((N, 2, cells(H, W, cell)[0] * cells(H, W, cell)[1]), F), np.ones((N, cells(H, W, cell)[0] * cells(H, W, cell)[1]), np.uint8),
                    (H, W), cell)[0]


def make_sequence(shape, T, seed, marks=True, bad=True):
    """shape = (N, H, W) -> (fw, bw float32 [N,T,2,H,W], stop uint8 [N,T,1,H,W]).  Per frame a smooth forward flow of about a pixel, given
    in closed form, and the backward flow as minus the forward flow at the point that maps to the pixel (two fixed-point steps of the
    closed form, plus a little noise), so most points are consistent with sub-pixel targets everywhere; a pasted rectangle moves
    differently in the forward flow alone (an occluder); `marks`: stop carries the BOUNDARY bit on about 1.5 % of the pixels and the
    other bits at random; `bad`: one unknown-flow value (1e10) in fw and one NaN in bw per sample, in frame 0."""
    N, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fw, bw = np.zeros((N, T, 2, H, W), np.float64), np.zeros((N, T, 2, H, W), np.float64)
    scale = (min(1.0, W / 48.0), min(1.0, H / 48.0))
    for n in range(N):
        for t in range(T):
            par = [(rng.uniform(0.3, 1.2) * scale[c], rng.uniform(0.02, 0.1), rng.uniform(0.02, 0.1), rng.uniform(0, 6.28, 2), rng.uniform(-0.8, 0.8) * scale[c])
                   for c in (0, 1)]
            f = lambda qx, qy: [amp * np.sin(fx * qx + ph[0]) * np.cos(fy * qy + ph[1]) + off for amp, fx, fy, ph, off in par]
            fw[n, t] = f(x, y)
            u, v = f(x, y)
            for _ in range(2):                                                      # p + f(p) = q, from p = q - f(q)
                u, v = f(x - u, y - v)
            bw[n, t] = [-u, -v]
    bw = bw + rng.normal(0, 0.03, bw.shape)
    if H >= 3 and W >= 4:
        y0, x0, h, w = H // 4, W // 4, max(1, H // 4), max(1, W // 4)
        fw[:, :, 0, y0:y0 + h, x0:x0 + w] += 2.5
        fw[:, :, 1, y0:y0 + h, x0:x0 + w] -= 1.5
    stop = rng.integers(0, 8, (N, T, 1, H, W)).astype(np.uint8)                      # bits 1, 2, 4: not in the default mask
    if marks:
        stop |= (rng.random(stop.shape) < 0.015).astype(np.uint8) * np.uint8(BOUNDARY)
        stop[:, 0, 0, H // 2, W // 2] |= BOUNDARY
    fw, bw = fw.astype(F), bw.astype(F)
    if bad:
        fw[:, 0, 0, H - 1 - H // 8, W // 8] = 1e10
        bw[:, 0, 1, H // 8, W - 1 - W // 8] = np.nan
    return fw, bw, stop


# ---- the raw C ABI -----------------------------------------------------------------------------------------------------------------
def f(x):
    return C.c_float(float(x))


def ptr(t):
    """Device (torch) tensor, ctypes buffer, int address or None -> c_void_p."""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, int):
        return C.c_void_p(t)
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(C.addressof(t))


def sizes(N, T, H, W, P):
    nbytes, k = C.c_size_t(), C.c_int()
    assert _lib.lib().fn2_flow_track_sizes(int(N), int(T), int(H), int(W), int(P), C.byref(nbytes), C.byref(k)) == OK
    return nbytes.value, k.value


def call(fw, bw, points, shape, results, state_out, ws, ws_bytes, stop=None, stop_mask=BOUNDARY, state_in=None, alpha=ALPHA, tracks=None,
         points_out=None, steps=None, stream=None):
    N, T, H, W, P = shape
    return _lib.lib().fn2_flow_track(ptr(fw), ptr(bw), ptr(stop), int(stop_mask), ptr(points), ptr(state_in), int(N), int(T), int(H), int(W),
                                     int(P), f(alpha[0]), f(alpha[1]), ptr(results), ptr(tracks), ptr(points_out), ptr(state_out),
                                     C.cast(ptr(steps), C.POINTER(C.c_int)), ptr(ws), int(ws_bytes), stream)


def call_reseed(points, state, born, N, H, W, cell, ws, ws_bytes, stream=None):
    return _lib.lib().fn2_flow_track_reseed(ptr(points), ptr(state), ptr(born), int(N), int(H), int(W), int(cell), ptr(ws), int(ws_bytes), stream)


def refusals(bufs, ws_bytes):
    """(label, expected status, the argument the error string must name, the string's prefix, thunk) for every call the header says is
    refused on the host, for shape N, T, H, W, P = 2, 3, 5, 7, 35 (reseed: cell 2, P = 12).  bufs: name -> any non-null host address; a
    refusal dereferences none of them."""
    S, nan = (2, 3, 5, 7, 35), float("nan")
    out = []

    def add(label, want, names, shape=S, alpha=ALPHA, nbytes=ws_bytes, **null):
        b = {k: (None if k in null else v) for k, v in bufs.items()}
        out.append((label, want, names, "flow_track:", lambda: call(
            b["fw"], b["bw"], b["points"], shape, b["results"], b["state_out"], b["ws"], nbytes, stop=b["stop"], state_in=b["state_in"], alpha=alpha,
            tracks=b["tracks"], points_out=b["points_out"], steps=b["steps"])))

    for name in ("fw", "bw", "points", "state_out", "results"):
        add(name + " NULL", INVALID, name, **{name: 1})
    add("N = 0", INVALID, "shape", shape=(0, 3, 5, 7, 35))
    add("T = 0", INVALID, "shape", shape=(2, 0, 5, 7, 35))
    add("H < 0", INVALID, "shape", shape=(2, 3, -5, 7, 35))
    add("W = 0", INVALID, "shape", shape=(2, 3, 5, 0, 35))
    add("P = 0", INVALID, "shape", shape=(2, 3, 5, 7, 0))
    add("flows of 2^31 elements", INVALID, "2^31", shape=(1 << 5, 1 << 5, 1 << 10, 1 << 10, 35))
    add("N T 2 H W wraps to 0 in 64 bits", INVALID, "2^31", shape=(1 << 21, 1 << 21, 1 << 11, 1 << 10, 35))
    add("H W alone is 2^30", INVALID, "2^31", shape=(1, 1, 1 << 15, 1 << 15, 35))
    add("tracks of 2^31 elements", INVALID, "2^31", shape=(2, 3, 5, 7, 1 << 28))
    add("every extent the largest int", INVALID, "2^31", shape=(2 ** 31 - 1,) * 5)
    add("alpha1 NaN", INVALID, "alpha1", alpha=(nan, 0.5))
    add("alpha1 < 0", INVALID, "alpha1", alpha=(-0.01, 0.5))
    add("alpha2 NaN", INVALID, "alpha2", alpha=(0.01, nan))
    add("alpha2 < 0", INVALID, "alpha2", alpha=(0.01, -0.5))
    add("workspace NULL", WORKSPACE, "workspace", ws=1)
    add("workspace too small", WORKSPACE, "workspace", nbytes=2 * K * 8 - 1)

    def reseed(label, want, names, N=2, H=5, W=7, cell=2, nbytes=24, **null):
        b = {k: (None if k in null else v) for k, v in bufs.items()}
        out.append((label, want, names, "flow_track_reseed:", lambda: call_reseed(b["points"], b["state_in"], b["born"], N, H, W, cell, b["ws"], nbytes)))

    reseed("reseed points NULL", INVALID, "points", points=1)
    reseed("reseed state NULL", INVALID, "state", state_in=1)
    reseed("reseed N = 0", INVALID, "shape", N=0)
    reseed("reseed W < 0", INVALID, "shape", W=-7)
    reseed("reseed cell = 0", INVALID, "cell", cell=0)
    reseed("reseed 2^31 elements", INVALID, "2^31", N=4, H=1 << 14, W=1 << 14, cell=1)
    reseed("reseed workspace NULL", WORKSPACE, "workspace", ws=1)
    reseed("reseed workspace too small", WORKSPACE, "workspace", nbytes=23)
    return out


# ---- the cases the GPU test and the validity test share -----------------------------------------------------------------------------
# name -> (N, T, H, W, P or None for the dense grid)
ORDINARY = {"subpixel": (2, 3, 7, 67, 100), "aligned": (1, 4, 16, 64, None), "ragged": (3, 2, 33, 67, None)}


def start_points(N, H, W, P, seed):
    """The dense pixel grid (P None) or P random sub-pixel points inside the plane, float32 [N,2,P]."""
    if P is None:
        return grid(N, H, W)
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, W - 0.01, (N, P)), rng.uniform(0, H - 0.01, (N, P))], 1).astype(F)


def ordinary_case(name):
    """(fw, bw, stop, points) of ORDINARY[name]: make_sequence with marks and bad values, seeded by the shape."""
    N, T, H, W, P = ORDINARY[name]
    fw, bw, stop = make_sequence((N, H, W), T, seed=H * 1000 + W)
    return fw, bw, stop, start_points(N, H, W, P, seed=W)
