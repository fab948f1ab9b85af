#!/usr/bin/env python
"""Score a net against ground truth over a list of image pairs: AEPE, Fl-all, the angular error, Sintel's bands and matched / unmatched
split (flownet2_amd/evaluate.py on the fused metrics kernel csrc/flow_metrics.hip).  The reference tree has no such script: its numbers
come from the solver's test nets, i.e. from the L1 training loss.

    python scripts/eval_flownet.py model.caffemodel deploy.prototxt.template list.txt        # run_flownet.py's first form (or seed:S ...)
    python scripts/eval_flownet.py [--net C|S|2] [--weights w.caffemodel|w.caffemodel.h5|w.npz] list.txt
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 scripts/eval_flownet.py --net 2 --weights w.caffemodel list.txt

list.txt lines: `img0 img1 gt [mask]`; gt is a .flo, a .npz (`flow`, optional `valid` / `occ`) or a KITTI flow .png; the mask (any image,
or .npy; non-zero = set) is read as `valid` or, with --mask occ, as `occ` (Sintel's occlusion maps).

The prediction is the runner's: the net at the adapted (x64) size, resampled and rescaled to the target size (run_flownet.py's loading,
run_flownet_many.py's grouping into batches of equal image size and its sharding of the list over the ranks, images and ground truth read
ahead of the GPU on a thread).  The kernel compares that prediction with the ground truth; each rank scores its shard, the rows are
gathered over gloo, rank 0 merges them in list order and prints one summary (strict JSON: a mean over no pixel is null).  --json OUT holds
the summary and the per-sample rows: in the default batch-invariant mode the file has the same bytes for any --batch and any number of processes.
--occ-from-consistency: for list lines that bring no occlusion mask, the net also runs backwards, (img1, img0), in the same step, and the
forward-backward check (functional.flow_consistency, thresholds --alpha) gives the `occ` plane, so the matched / unmatched split exists for
such data too (FlyingChairs, KITTI without its noc maps); the JSON then records "occ_source": "consistency" and the thresholds.
--error-maps DIR writes every pair's KITTI-style error image (functional.flow_error_map with --outlier's thresholds: blue below the Fl
criterion, red above, black without ground truth, dimmed to half where the pair's occlusion mask -- the data's, or with
--occ-from-consistency the check's -- is set) as DIR/<list index>.png; --color-maps DIR the colour-coded prediction, normalised per pair
or with --color-max F by F.  Neither changes a byte of the JSON.
Exits with status 1 when a valid pixel had a NaN or Inf prediction (they are in no sum), unless --allow-nonfinite."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet2_amd import evaluate, parallel  # noqa: E402
from flownet2_amd import functional as Fn  # noqa: E402
import run_flownet as RF  # noqa: E402
import run_flownet_many as RM  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    # the first form is recognised as run_flownet.py recognises it: by its deploy prototxt (template)
    proto = any(p.endswith((".prototxt", ".template")) for p in RF._positionals(sys.argv[1:])) and "--net" not in sys.argv
    if proto:
        ap.add_argument("caffemodel", help="path to model (or seed:S / seed:C / seed:2)")
        ap.add_argument("deployproto", help="path to deploy prototxt template")
    else:
        ap.add_argument("--net", choices=["C", "S", "2"], default="C")
        ap.add_argument("--weights", default=None)
    ap.add_argument("listfile")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prefetch", type=int, default=2, help="groups the reading thread may run ahead of the GPU")
    ap.add_argument("--mask", choices=["valid", "occ"], default="valid", help="what a list line's fourth field is")
    ap.add_argument("--outlier", type=float, nargs=2, default=[3.0, 0.05], metavar=("ABS", "REL"), help="Fl: EPE > ABS px and > REL |gt|")
    ap.add_argument("--bands", type=float, nargs=2, default=[10.0, 40.0], metavar=("B0", "B1"), help="edges of the three |gt| bands")
    ap.add_argument("--json", default=None, metavar="OUT", help="write the summary and the per-sample rows")
    ap.add_argument("--epe-maps", default=None, metavar="DIR", help="write every pair's EPE map as DIR/<list index>.npy")
    ap.add_argument("--error-maps", default=None, metavar="DIR", help="write every pair's error image as DIR/<list index>.png")
    ap.add_argument("--color-maps", default=None, metavar="DIR", help="write every pair's colour-coded prediction as DIR/<list index>.png")
    ap.add_argument("--color-max", type=float, default=None, metavar="F", help="with --color-maps: the radius drawn at full saturation "
                    "(default: each prediction's own largest radius)")
    ap.add_argument("--occ-from-consistency", action="store_true", help="lines without an occlusion mask: occ from the forward-backward check")
    ap.add_argument("--alpha", type=float, nargs=2, default=[0.01, 0.5], metavar=("A1", "A2"), help="inconsistent: |a+b|^2 > A1 (|a|^2+|b|^2) + A2")
    ap.add_argument("--allow-nonfinite", action="store_true")
    ap.add_argument("--no-batch-invariant", action="store_true", help="let kernel selection depend on the batch size (see run_flownet_many.py)")
    ap.add_argument("--gpu", type=int, default=None, help="device index (default: LOCAL_RANK)")
    Fn.add_arithmetic_flags(ap, RM.ARITH)
    Fn.add_general_convolution_flag(ap)
    a = ap.parse_args()
    if proto:
        if not a.caffemodel.startswith("seed:") and not os.path.exists(a.caffemodel):
            raise SystemExit("caffemodel does not exist: " + a.caffemodel)
        if not os.path.exists(a.deployproto):
            raise SystemExit("deploy-proto does not exist: " + a.deployproto)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")              # the rows are gathered as Python objects; ranks may share one GPU
    dev = torch.device("cuda", a.gpu if a.gpu is not None else int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(dev)
    Fn.set_batch_invariant(not a.no_batch_invariant)
    Fn.apply_arithmetic_flags(a, RM.ARITH)
    Fn.apply_general_convolution_flag(a)
    with open(a.listfile) as f:
        entries = evaluate.parse_list(f)
    for e in entries:
        for path in e:
            if path is not None and not os.path.exists(path):
                raise SystemExit("file does not exist: " + path)
    if a.color_max is not None and not a.color_maps:
        raise SystemExit("--color-max needs --color-maps")
    for d in (a.epe_maps, a.error_maps, a.color_maps):
        if d:
            os.makedirs(d, exist_ok=True)

    up = lambda x: None if x is None else torch.from_numpy(x).to(dev, non_blocking=True)
    if proto:
        predict = lambda i0, i1: RF.infer_prototxt(a.caffemodel, a.deployproto, up(i0), up(i1), dev)
    else:
        P, mean = RF.load_params(a.net, a.weights, dev)
        predict = lambda i0, i1: RF.infer(a.net, P, up(i0), up(i1), mean)

    if a.occ_from_consistency:
        one_way = predict
        predict = lambda i0, i1: one_way(np.concatenate([i0, i1]), np.concatenate([i1, i0]))      # rows 0 .. n-1 forward, n .. 2n-1 backward

    def metrics(pred, gt, valid, occ, has_occ=None):
        with torch.no_grad():
            occ = up(occ)
            if a.occ_from_consistency:
                n = pred.shape[0] // 2
                pred, back = pred[:n].contiguous(), pred[n:].contiguous()
                if not all(has_occ):
                    found = Fn.flow_consistency(pred, back, alpha=tuple(a.alpha)).occ_fw
                    given = torch.tensor(has_occ, device=dev).view(n, 1, 1, 1)
                    occ = found if occ is None else torch.where(given, occ, found)
            gt, valid = up(gt), up(valid)
            m = Fn.flow_metrics(pred, gt, valid, occ, outlier=tuple(a.outlier), bands=tuple(a.bands), epe_map=bool(a.epe_maps))
            # the pictures of this group, for save_maps
            m.error_rgb = Fn.flow_error_map(pred, gt, valid, occ, abs_thresh=a.outlier[0], rel_thresh=a.outlier[1]) if a.error_maps else None
            m.color_rgb = Fn.flow_to_color(pred.contiguous(), max_flow=a.color_max) if a.color_maps else None
            return m

    def save_maps(ents, m):
        from flownet2_amd import visualize
        for directory, rgb in ((a.error_maps, m.error_rgb), (a.color_maps, m.color_rgb)):
            if directory:
                rgb = rgb.cpu().numpy()
                for k, e in enumerate(ents):
                    visualize.write_png(os.path.join(directory, "%06d.png" % e[4]), rgb[k])
        m.error_rgb = m.color_rgb = None                        # written: the rows stay until the gather, the pictures need not
        if not a.epe_maps:
            return
        maps = m.epe_map.cpu().numpy()
        for k, e in enumerate(ents):
            np.save(os.path.join(a.epe_maps, "%06d.npy" % e[4]), maps[k, 0])

    result = evaluate.evaluate(entries, RM.groups_of, RF.read_image, predict, metrics, batch=a.batch, prefetch=a.prefetch, mask_as=a.mask,
                               on_group=save_maps if (a.epe_maps or a.error_maps or a.color_maps) else None, occ_present=a.occ_from_consistency)
    status = 0
    if parallel.rank() == 0:
        s = result.summary()
        if a.json:
            with open(a.json, "w") as f:
                f.write(result.to_json({"occ_source": "consistency", "alpha": list(a.alpha)} if a.occ_from_consistency else None))
        print(json.dumps(evaluate.json_ready(s), allow_nan=False))
        status = evaluate.exit_status(s, a.allow_nonfinite)
        if status:
            print(f"{s['nonfinite']} valid pixels had a NaN or Inf prediction (--allow-nonfinite to accept)", file=sys.stderr)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return status


if __name__ == "__main__":
    sys.exit(main())
