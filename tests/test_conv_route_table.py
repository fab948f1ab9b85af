"""The host side of csrc/conv_route.cpp, pinned: what every decision, size, support and count query of the forward, data-gradient and
weight-gradient groups answers for every route value, and (where no GPU is visible) the code and text of every call refused on NULL blobs,
against tests/golden/conv_route_table.json.  None of these functions asks the device.

The fixture was written once from a build of the commit before conv_route.cpp was re-cut around its three tables of kernel families
(`python tests/test_conv_route_table.py --write`); pytest only compares.  The dispatcher's oddities are part of what is pinned: the size
queries answer non-zero for a base route whose family does not take the layer (fn2_conv_packed_weight_floats has no `takes` in front of
it; ops.conv_pack_weights and the Caffe adapter read those numbers), and the NULL refusal has two spellings.

Descriptors: every case of test_conv_forward_routes.FWD, of test_conv_backward_routes.DGRAD and WGRAD, every Convolution / Deconvolution of
the deploy and training graphs those two files enumerate (one per geometry), and four invalid descriptors -- each at N = 1 and N = 8, with
batch-invariant mode off and on.  Route values: 0 .. 6, each also | 0x100 (so 0x100 alone is among them), for both values of `transposed`.

A line of the fixture is the list of answers in the order queries() asks them, run-length coded (-n: the value before it n more times);
a batch-invariant line that equals the line of the same descriptor and batch with the mode off says so instead."""
import ctypes as C
import json
import os
import subprocess
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pytest
import torch

from flownet2_amd import _lib, ops
from test_conv_backward_routes import DGRAD, WGRAD, family_training_layers, flownetc_training_layers
from test_conv_forward_routes import FWD, production_layers
from test_train_parity_family import CASES as FAMILY_CASES

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_route_table.json")
ARITH = 0x100                                                   # FN2_CONV_ARITH_BF16X3
ROUTES = [r | a for a in (0, ARITH) for r in range(7)]          # every route value of the three groups, and one past them
BATCHES = (1, 8)
SAME = "as inv=0"                                               # a line of batch-invariant mode that equals the line before it

# Texts that moved when the split-bf16 rows of fn2_conv_forward (DIRECT | BF16X3, WINOGRAD | BF16X3) came to pass the
# dispatcher's shared checks before their kernel's own: {text of the fixture: text now}.  The code is FN2_ERR_INVALID_ARG either way.
# (With real blobs, which this file never passes, the slice refusal of the same two rows moves in the same way: "conv_bf16x3: channel slice
# outside the blob" / "conv_wino_bf16x3: ..." -> "conv_forward: channel slice outside its blob", FN2_ERR_INVALID_ARG either way.)
TEXT_MOVED = {"conv_bf16x3: null blob": "conv_forward: NULL blob", "conv_wino_bf16x3: null blob": "conv_forward: NULL blob"}


def descriptors():
    """{name: (own N, Cin, H, W, Cout, kernel, stride, pad)}, in a fixed order."""
    out = {}
    for n, (_, tr, N, Cin, H, W, Cout, k, s, p) in FWD.items():
        out["fwd/" + n] = (N, Cin, H, W, Cout, k, s, p)
    for n, (_, tr, N, Cin, H, W, Cout, k, s, p) in DGRAD.items():
        out["dgrad/" + n] = (N, Cin, H, W, Cout, k, s, p)
    for (N, Cin, H, W, Cout, k, s, p, tr) in WGRAD:
        out["wgrad/%dx%dx%d-%d-k%d" % (Cin, H, W, Cout, k)] = (N, Cin, H, W, Cout, k, s, p)
    layers = [l[1:] for l in production_layers()] + flownetc_training_layers()
    for case, (B, H, W) in FAMILY_CASES.items():
        layers += family_training_layers(case, B, H, W)
    seen = set()
    for (_, kind, N, Cin, H, W, Cout, k, s, p) in layers:
        if (kind, Cin, H, W, Cout, k, s, p) not in seen:        # one per geometry: the batch is asked at 1 and 8 anyway
            seen.add((kind, Cin, H, W, Cout, k, s, p))
            out["graph/%s%dx%dx%d-%d-k%ds%dp%d" % (kind[0], Cin, H, W, Cout, k, s, p)] = (N, Cin, H, W, Cout, k, s, p)
    out["invalid/zero-channels"] = (2, 0, 16, 24, 64, 3, 1, 1)
    out["invalid/kernel-larger-than-the-padded-map"] = (2, 64, 2, 3, 64, 7, 2, 1)
    out["invalid/stride-0"] = (2, 64, 16, 24, 64, 3, 0, 1)
    out["invalid/negative-pad"] = (2, 64, 16, 24, 64, 3, 1, -1)
    return out


def queries(d):
    """[(key, answer)] of every query for one descriptor, in a fixed order; the key names the function and its route / flags / transposed."""
    L, p, out = _lib.lib(), C.byref(d), []
    for f in range(8):
        out.append(("fn2_conv_route flags=%d" % f, L.fn2_conv_route(p, f)))
        out.append(("fn2_deconv_route flags=%d" % f, L.fn2_deconv_route(p, f)))
    for tr in (0, 1):
        out.append(("fn2_conv_backward_data_route tr=%d" % tr, L.fn2_conv_backward_data_route(p, tr)))
        for f in range(8):
            out.append(("fn2_conv_backward_data_route_flags tr=%d flags=%d" % (tr, f), L.fn2_conv_backward_data_route_flags(p, tr, f)))
            out.append(("fn2_conv_backward_weights_arith tr=%d flags=%d" % (tr, f), L.fn2_conv_backward_weights_arith(p, tr, f)))
        for name in ("fn2_conv_backward_weights_supported", "fn2_conv_backward_weights_workspace_bytes", "fn2_conv_backward_weights_bias_fused"):
            out.append(("%s tr=%d" % (name, tr), getattr(L, name)(p, tr)))
    for r in ROUTES:
        for name in ("fn2_conv_packed_weight_floats", "fn2_conv_workspace_bytes", "fn2_deconv_packed_weight_floats", "fn2_deconv_workspace_bytes"):
            out.append(("%s route=0x%x" % (name, r), getattr(L, name)(p, r)))
        for tr in (0, 1):
            at = "tr=%d route=0x%x" % (tr, r)
            for name in ("fn2_conv_backward_data_packed_weight_floats", "fn2_conv_backward_data_pack_workspace_bytes", "fn2_conv_backward_data_workspace_bytes",
                         "fn2_conv_backward_data_computed_channels", "fn2_conv_backward_data_masked_supported"):
                out.append(("%s %s" % (name, at), getattr(L, name)(p, tr, r)))
            Cp = L.fn2_conv_backward_data_computed_channels(p, tr, r)
            out.append(("fn2_conv_backward_data_workspace_bytes_with_room %s room=Cin" % at, L.fn2_conv_backward_data_workspace_bytes_with_room(p, tr, r, d.Cin)))
            out.append(("fn2_conv_backward_data_workspace_bytes_with_room %s room=computed" % at, L.fn2_conv_backward_data_workspace_bytes_with_room(p, tr, r, Cp)))
            out.append(("fn2_conv_backward_weights_workspace_bytes_arith tr=%d arith=0x%x" % (tr, r), L.fn2_conv_backward_weights_workspace_bytes_arith(p, tr, r)))
    return [(k, int(v)) for k, v in out]


def rle(values):
    out = []
    for v in values:
        assert v >= 0
        if out and out[-1] < 0 and prev == v:
            out[-1] -= 1
        elif out and prev == v:
            out.append(-1)
        else:
            out.append(v)
        prev = v
    return out


def unrle(coded):
    out = []
    for v in coded:
        out += [out[-1]] * -v if v < 0 else [v]
    return out


def answer_lines(names=None):
    """{"<descriptor> N=<n> inv=<0|1>": [(key, answer)]}; batch-invariant mode is left as it was found."""
    lines, was = {}, ops.get_batch_invariant()
    try:
        for name, (_, *geom) in descriptors().items():
            if names is not None and name not in names:
                continue
            for N in BATCHES:
                for inv in (0, 1):
                    ops.set_batch_invariant(bool(inv))
                    lines["%s N=%d inv=%d" % (name, N, inv)] = queries(ops.conv_desc(N, *geom))
    finally:
        ops.set_batch_invariant(was)
    return lines


# ---------------------------------------------------------------------------------------------------------------------------------------
# the refused calls: every blob pointer NULL, so every call ends at a NULL check at the latest and nothing is launched


def refused(d):
    """[(key, code, text)] of every dispatch and pack call on NULL blobs, for every route value."""
    L, p, out = _lib.lib(), C.byref(d), []

    def call(key, code):
        out.append((key, int(code), L.fn2_last_error_string().decode() if code else ""))

    for tr in (0, 1):
        call("fn2_conv_backward_weights tr=%d" % tr, L.fn2_conv_backward_weights(p, tr, None, d.Cin, 0, None, d.Cout, 0, None, 0, None, 0, None))
        call("fn2_conv_backward_weights_bias tr=%d" % tr, L.fn2_conv_backward_weights_bias(p, tr, None, None, None, None, 0, None, 0, None))
    # call by call, every route value in turn: what a call answers seldom depends on the route, and the fixture's lines are run-length coded
    for r in ROUTES:
        call("fn2_conv_forward route=0x%x" % r, L.fn2_conv_forward(p, r, None, d.Cin, 0, None, None, None, d.Cout, 0, 1, C.c_float(0.1), None, 0, None))
    for r in ROUTES:
        call("fn2_deconv_forward route=0x%x" % r, L.fn2_deconv_forward(p, r, None, d.Cin, 0, None, None, None, d.Cout, 0, 0, C.c_float(0.1), None, 0, None))
    for r in ROUTES:
        call("fn2_conv_pack_weights route=0x%x" % r, L.fn2_conv_pack_weights(p, r, None, None, None))
    for r in ROUTES:
        call("fn2_deconv_pack_weights route=0x%x" % r, L.fn2_deconv_pack_weights(p, r, None, None, None))
    for tr in (0, 1):
        for r in ROUTES:
            call("fn2_conv_backward_data_pack_weights tr=%d route=0x%x" % (tr, r), L.fn2_conv_backward_data_pack_weights(p, tr, r, None, None, None, 0, None))
        for r in ROUTES:
            call("fn2_conv_backward_data tr=%d route=0x%x" % (tr, r),
                 L.fn2_conv_backward_data(p, tr, r, None, d.Cout, 0, None, None, d.Cin, 0, d.Cin, None, 0, None))
        for r in ROUTES:
            call("fn2_conv_backward_data_masked tr=%d route=0x%x" % (tr, r),
                 L.fn2_conv_backward_data_masked(p, tr, r, None, d.Cout, 0, None, None, d.Cin, 0, None, d.Cin, 0, C.c_float(0.1), None))
        for r in ROUTES:
            call("fn2_conv_backward_weights_arith_run tr=%d arith=0x%x" % (tr, r),
                 L.fn2_conv_backward_weights_arith_run(p, tr, r, None, d.Cin, 0, None, d.Cout, 0, None, 0, None, 0, None))
    return out


def template(text, d, key):
    """The text with the descriptor's geometry and the call's route value taken out (<G>, <R>, <X>): exact again once they are put back."""
    r = int(key.rsplit("=0x", 1)[1], 16) if "=0x" in key else None
    geom = "{kernel %d, stride %d, pad %d} %d -> %d on %d x %d" % (d.kernel, d.stride, d.pad, d.Cin, d.Cout, d.Hin, d.Win)
    text = text.replace(geom, "<G>")
    if r is not None:
        text = text.replace("route %d" % r, "route <R>").replace("arithmetic 0x%x" % r, "arithmetic <X>")
    return text


def refusal_lines(names=None):
    """{descriptor: [(key, code, text template)]}, each descriptor at its own batch, batch-invariant mode off."""
    assert not ops.get_batch_invariant()
    lines = {}
    for name, geom in descriptors().items():
        if names is None or name in names:
            d = ops.conv_desc(*geom)
            lines[name] = [(key, code, template(text, d, key)) for key, code, text in refused(d)]
    return lines


# ---------------------------------------------------------------------------------------------------------------------------------------

GROUPS = ["fwd", "dgrad", "wgrad", "graph", "invalid"]


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def names_of(group):
    return {n for n in descriptors() if n.startswith(group + "/")}


@pytest.mark.parametrize("group", GROUPS)
def test_queries_answer_what_they_answered(group):
    want = {k: v for k, v in fixture()["answers"].items() if k.startswith(group + "/")}
    got = answer_lines(names_of(group))
    assert got.keys() == want.keys() and len(got) == 4 * len(names_of(group)) >= 16
    moved = []
    for line, answers in got.items():
        was = unrle(want[line] if want[line] != SAME else want[line.replace("inv=1", "inv=0")])
        assert len(was) == len(answers), line
        moved += ["%s: %s = %d, was %d" % (line, key, v, w) for (key, v), w in zip(answers, was) if v != w]
    assert not moved, "%d answers moved, the first: %s" % (len(moved), moved[:8])


@pytest.mark.parametrize("group", GROUPS)
def test_null_blobs_are_refused_as_they_were(group):
    if torch.cuda.is_available():
        pytest.skip("the refused calls are pinned where no device is visible")
    doc = fixture()
    want = {k: v for k, v in doc["refused"].items() if k.startswith(group + "/")}
    got = refusal_lines(names_of(group))
    assert got.keys() == want.keys() and len(got) >= 4
    moved = []
    for name, calls in got.items():
        was = [doc["refusals"][i] for i in unrle(want[name])]
        assert len(was) == len(calls), name
        for (key, code, text), (wcode, wtext) in zip(calls, was):
            assert code != 0, (name, key)          # nothing ran
            if code != wcode or text != TEXT_MOVED.get(wtext, wtext):
                moved.append("%s: %s = (%d, %r), was (%d, %r)" % (name, key, code, text, wcode, wtext))
    assert not moved, "%d refusals moved, the first: %s" % (len(moved), moved[:8])


def test_moved_texts_are_texts_of_the_fixture():
    texts = {t for _, t in fixture()["refusals"]}
    assert set(TEXT_MOVED) <= texts and all(new != old for old, new in TEXT_MOVED.items())


def test_run_length_code_round_trips():
    for v in ([], [0], [5, 5], [0, 0, 0, 7, 7, 1, 0, 0], [3, 0, 3, 3, 3, 3]):
        assert unrle(rle(v)) == v
    assert rle([0, 0, 0, 7, 7]) == [0, -2, 7, -1]


def write():
    assert not torch.cuda.is_available(), "the refused calls are recorded where no device is visible"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    commit = subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"]).decode().strip()
    assert not subprocess.check_output(["git", "-C", root, "status", "--porcelain", "--", "flownet2_amd/csrc", "include"]).strip(), "library sources differ from HEAD"
    answers = {line: rle([v for _, v in a]) for line, a in answer_lines().items()}
    answers = {line: SAME if line.endswith("inv=1") and a == answers[line.replace("inv=1", "inv=0")] else a for line, a in answers.items()}
    table, refused_lines = [], {}
    for name, calls in refusal_lines().items():
        idx = []
        for _, code, text in calls:
            if [code, text] not in table:
                table.append([code, text])
            idx.append(table.index([code, text]))
        refused_lines[name] = rle(idx)
    keys = [k for k, _ in queries(ops.conv_desc(1, 64, 16, 24, 64, 3, 1, 1))]
    path = sys.argv[sys.argv.index("--write") + 1] if len(sys.argv) > sys.argv.index("--write") + 1 else FIXTURE
    dump = lambda v: json.dumps(v, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{\n"made": %s,\n' % json.dumps(
            "written once by tests/test_conv_route_table.py --write, on a host without a GPU, from a build of commit %s (the last one before "
            "csrc/conv_route.cpp was re-cut around its tables of kernel families)" % commit))
        f.write('"answers_per_line": %d,\n' % len(keys))
        f.write('"refusals": [\n%s\n],\n' % ",\n".join(dump(t) for t in table))
        f.write('"answers": {\n%s\n},\n' % ",\n".join("%s:%s" % (json.dumps(k), dump(v)) for k, v in answers.items()))
        f.write('"refused": {\n%s\n}\n}\n' % ",\n".join("%s:%s" % (json.dumps(k), dump(v)) for k, v in refused_lines.items()))
    print("wrote %d answer lines of %d answers, %d refusal lines over %d distinct refusals, %d bytes to %s"
          % (len(answers), len(keys), len(refused_lines), len(table), os.path.getsize(path), path))


if __name__ == "__main__":
    assert "--write" in sys.argv, "usage: python tests/test_conv_route_table.py --write [path]"
    write()
