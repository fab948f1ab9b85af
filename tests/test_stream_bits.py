"""The bits of the seven streaming-reduction kernel files (csrc/l1loss.hip, lpq_loss.hip, flow_metrics.hip, flow_consistency.hip,
flow_visualize.hip, flow_track.hip, unsup_loss.hip), pinned: SHA-256 of the raw bytes of every output -- result rows, maps, flag planes,
RGB, tracks, points, states, steps, gradients and loss scalars -- of each kernel through the C ABI, on the seeded inputs and at every shape
of each kernel's own test file, against tests/golden/stream_bits.json.  Outputs hold NaN where the headers say so (the EPE map at a pixel
that is not counted, a stopped point's track), so what is hashed is bytes, never values.

The fixture was written once, on an MI355X, from a build of the commit before the kernels came to share csrc/stream_reduce.hpp's toolkit;
a change that means to move bits regenerates it (`python tests/test_stream_bits.py --write`, on the GPU) and says so.  pytest only
compares."""
import hashlib
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

import flow_track_ref as TR
import lpq_cases as LC
import unsup_loss_ref as UR
import test_flow_consistency as fc
import test_flow_metrics as fm
import test_flow_track as ft
import test_flow_visualize as fv
import test_lpq_loss as lpq
import test_unsup_loss as ul
from flownet2_amd import ops

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_bits.json")


def sha(a):
    a = np.ascontiguousarray(a)
    assert a.size
    return hashlib.sha256(a.tobytes()).hexdigest()


def metrics_results(name):
    """flow_metrics: the module's own case; the rows of a call without and with the EPE map, and the map"""
    shape, offset, _ = fm.CASES[name]
    rows, _ = fm._run_arrays(fm._inputs(name), shape, offset, epe_map=False)
    rows_map, emap = fm._run_arrays(fm._inputs(name), shape, offset, epe_map=True)
    return {"rows": rows, "with_map/rows": rows_map, "with_map/epe_map": emap}


def consistency_results(name):
    """flow_consistency: every kind of the module; rows, and per direction the flag, occ, err and warped maps"""
    out = {}
    for kind in fc.KINDS:
        rows, maps = fc.run_arrays(*fc._inputs(name, kind), offset=fc.SHAPES[name][1])
        out[kind + "/rows"] = rows
        for d in range(2):
            for key, a in maps[d].items():
                out["%s/%s%d" % (kind, key, d)] = a
    return out


def visualize_results(name):
    """flow_visualize: every kind under each of the three norms (picture and the radius used), and the error image of the module's case"""
    out = {}
    offset = fv.SHAPES[name][1]
    for kind in fv.KINDS:
        for norm_name, norm in (("sample", fv.SAMPLE), ("batch", fv.BATCH), ("fixed", fv.FIXED)):
            rgb, used = fv.run_color(fv._flow(name, kind), norm, fv.FIXED_MAX if norm == fv.FIXED else 0.0, offset)
            out["%s/%s/rgb" % (kind, norm_name)] = rgb
            out["%s/%s/maxrad" % (kind, norm_name)] = used
    out["error/rgb"] = fv.run_error(*fv._error_case(name), offset=offset)
    return out


def track_results(name):
    """flow_track: every kind of the module; rows, tracks, last positions, states and steps"""
    out = {}
    for kind in ft.KINDS:
        d = ft._inputs(name, kind)
        rows, host = ft.run_arrays(d["fw"], d["bw"], d["points"], stop=d["stop"], state=d["state"], alpha=d["alpha"], offset=ft.SHAPES[name][5])
        out[kind + "/rows"] = rows
        for key, a in host.items():
            out["%s/%s" % (kind, key)] = a
    return out


RESEED = {"1x36x60_cell4": (1, 36, 60, 4), "2x5x7_cell2": (2, 5, 7, 2), "1x3x5_cell1": (1, 3, 5, 1), "2x33x67_cell8": (2, 33, 67, 8)}


def reseed_results(name):
    """flow_track_reseed at the shapes of the module's reseeding test: the grid from slots that are all stopped; then the slots after one
    tracker step (the kernel's own, on make_sequence's flows scaled as there) reseeded"""
    N, H, W, cell = RESEED[name]
    ch, cw = TR.cells(H, W, cell)
    P = ch * cw
    p0, s0, b0 = ft.run_reseed(np.full((N, 2, P), np.nan, np.float32), np.full((N, P), ft.STOP["OUTSIDE"], np.uint8), (H, W), cell)
    fw, bw, stop = TR.make_sequence((N, H, W), 1, seed=H + cell)
    fw = (fw * np.float32(max(1.0, cell / 2))).astype(np.float32)
    _, moved = ft.run_arrays(fw, bw, p0, stop=stop, outputs=("points_out",))
    p1, s1, b1 = ft.run_reseed(moved["points_out"], moved["state"], (H, W), cell)
    return {"grid/points": p0, "grid/state": s0, "grid/born": b0, "moved/points": p1, "moved/state": s1, "moved/born": b1}


# unsup_loss: (label, smoothness order, two directions, parameters): both orders and one and two directions under gamma = 0.5 without an
# edge weight (sqrtf alone) and under the defaults (a general gamma: powf, and expf for the edge weight)
UNSUP_FORMS = [
    ("exact/order1/two", 1, True, UR.EXACT), ("exact/order2/one", 2, False, UR.EXACT), ("exact/order2/two", 2, True, UR.EXACT),
    ("general/order1/one", 1, False, {}), ("general/order1/two", 1, True, {}), ("general/order2/two", 2, True, {}),
]


def unsup_results(name):
    """unsup_loss forward and backward: every kind of the module under UNSUP_FORMS; rows, loss and the gradients"""
    out = {}
    for kind in ul.KINDS:
        for label, order, two, kw in UNSUP_FORMS:
            got = ul.run(ul._case(name, kind), UR.params(smooth_order=order, **kw), offset=ul.SHAPES[name][1], two=two, total_diff=0.75)
            key = "%s/%s/" % (kind, label)
            out[key + "rows"], out[key + "loss"] = got["rows"], got["loss"]
            for d, g in enumerate(got["diff"]):
                out["%sdiff%d" % (key, d)] = g
    return out


def lpq_results(name):
    """lpq_loss forward and backward, single calls: every (p, q, p_epsilon) of lpq_cases.PQ_CASES, so every way a power is taken"""
    out = {}
    for pq in LC.PQ_CASES:
        for key, a in lpq._run(name, pq).items():
            if a is not None:
                out["p%g_q%g_pe%g/%s" % (pq + (key,))] = a
    return out


def lpq_multi_results(name):
    """lpq_loss forward and backward, the one-launch form over the module's five scales, called twice as there"""
    p, q, pe = LC.PQ_CASES[int(name[2:])]
    shapes, weights = lpq.MULTI_SHAPES, lpq.MULTI_WEIGHTS
    n = len(shapes)
    one, multi, sync_bytes = LC.sizes(n)
    ins = [LC.make_inputs(s, True, seed=100 + k) for k, s in enumerate(shapes)]
    b0s, b1s = [lpq._dev(a) for a, _ in ins], [lpq._dev(b) for _, b in ins]
    total_diff = torch.tensor([1.75], device="cuda")
    ws = torch.zeros(multi, dtype=torch.uint8, device="cuda")
    sync = torch.zeros(sync_bytes, dtype=torch.uint8, device="cuda")
    losses, total = torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
    d0s, d1s = [lpq._empty(s) for s in shapes], [lpq._empty(s) for s in shapes]
    for _ in range(2):
        assert LC.forward_multi(b0s, b1s, shapes, weights, p, q, pe, LC.Q_EPS, False, True, losses, total, ws, multi, sync) == LC.OK
    assert LC.backward_multi(b0s, b1s, d0s, d1s, shapes, weights, p, q, pe, LC.Q_EPS, False, True, total_diff, ws, multi) == LC.OK
    torch.cuda.synchronize()
    out = {"losses": losses.cpu().numpy(), "total": total.cpu().numpy(), "sync": sync.cpu().numpy()}
    for k in range(n):
        out["scale%d/loss_norm" % k] = ws[k * one:k * one + 8].cpu().numpy()
        out["scale%d/d0" % k], out["scale%d/d1" % k] = d0s[k].cpu().numpy(), d1s[k].cpu().numpy()
    return out


# l1loss: a blob of under 64 elements (one wave, partly idle) and one of 2 * 3 * 256 * C elements (six workgroups in either form, all four
# waves of each at work); both forms, with and without the plateau
L1_SHAPES = {"1x2x3x5": (1, 2, 3, 5), "2x2x24x32": (2, 2, 24, 32)}
L1_FORMS = {
    "l1": dict(normalize_by_num_entries=True),
    "l1_plateau": dict(plateau=0.05),
    "l2": dict(l2_per_location=True, normalize_by_num_entries=True),
    "l2_prescale_plateau": dict(l2_per_location=True, l2_prescale_by_channels=True, plateau=0.05),
}
L1_WEIGHTS = [0.32, 0.08]


def _l1_inputs(shape_name, two):
    b0, b1 = LC.make_inputs(L1_SHAPES[shape_name], two, seed=7 + sorted(L1_SHAPES).index(shape_name))
    return torch.from_numpy(b0).cuda(), (torch.from_numpy(b1).cuda() if two else None)


def l1_results(name):
    """l1loss forward and backward, single calls (one and two bottoms) and the one-launch form over both shapes, called twice"""
    p = ops.l1_params(**L1_FORMS[name])
    out = {}
    for shape_name in L1_SHAPES:
        for two in (True, False):
            b0, b1 = _l1_inputs(shape_name, two)
            loss, ws = ops.l1loss_forward(p, b0, b1)
            d0, d1 = ops.l1loss_backward(p, b0, b1, 0.32, ws)
            torch.cuda.synchronize()
            key = "%s/%s/" % (shape_name, "two" if two else "one")
            out[key + "loss"], out[key + "loss_norm"], out[key + "d0"] = loss.cpu().numpy(), ws[:8].cpu().numpy(), d0.cpu().numpy()
            if two:
                out[key + "d1"] = d1.cpu().numpy()
    pairs = [_l1_inputs(shape_name, True) for shape_name in L1_SHAPES]
    b0s, b1s = [a for a, _ in pairs], [b for _, b in pairs]
    for _ in range(2):
        total, losses, ws = ops.l1loss_forward_multi(p, b0s, b1s, L1_WEIGHTS)
    d0s, d1s = ops.l1loss_backward_multi(p, b0s, b1s, L1_WEIGHTS, torch.tensor(1.75, device="cuda"), ws, need1=True)
    torch.cuda.synchronize()
    out["multi/total"], out["multi/losses"] = total.cpu().numpy(), losses.cpu().numpy()
    one = ws.numel() // len(pairs)
    for k in range(len(pairs)):
        out["multi/scale%d/loss_norm" % k] = ws[k * one:k * one + 8].cpu().numpy()
        out["multi/scale%d/d0" % k], out["multi/scale%d/d1" % k] = d0s[k].cpu().numpy(), d1s[k].cpu().numpy()
    return out


# kernel: (its cases, case -> {output: array})
KERNELS = {
    "flow_metrics": (fm.CASES, metrics_results),
    "flow_consistency": (fc.SHAPES, consistency_results),
    "flow_visualize": (fv.SHAPES, visualize_results),
    "flow_track": (ft.SHAPES, track_results),
    "flow_track_reseed": (RESEED, reseed_results),
    "unsup_loss": (ul.SHAPES, unsup_results),
    "lpq_loss": (LC.SHAPES, lpq_results),
    "lpq_loss_multi": (["pq%d" % k for k in range(len(LC.PQ_CASES))], lpq_multi_results),
    "l1loss": (L1_FORMS, l1_results),
}
CASES = [(k, name) for k in KERNELS for name in KERNELS[k][0]]


def hashes(kernel, name):
    return {"%s/%s/%s" % (kernel, name, key): sha(a) for key, a in KERNELS[kernel][1](name).items()}


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
        "made": "written once by tests/test_stream_bits.py --write on the GPU named below, from a build of commit 6a1c2fe (the last one before "
                "the seven streaming-reduction kernel files shared csrc/stream_reduce.hpp's toolkit)",
        "device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "numpy": np.__version__, "torch": torch.__version__,
        "sha256": out,
    }
    path = sys.argv[sys.argv.index("--write") + 1] if len(sys.argv) > sys.argv.index("--write") + 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d hashes to %s" % (len(out), path))


if __name__ == "__main__":
    assert "--write" in sys.argv, "usage: python tests/test_stream_bits.py --write [path]"
    write()
