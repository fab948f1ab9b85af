#!/usr/bin/env python
"""py3 re-authoring of scripts/run-flownet-many.py on the MI355X path, sharded over the GPUs of a node.

    python scripts/run_flownet_many.py [--net C|S|2] list.txt                                  # 1 GPU
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 scripts/run_flownet_many.py list.txt

list.txt lines: `img0 img1 out.flo` (run-flownet-many.py:27-36).  The reference re-creates the caffe.Net for every
entry (:77-81 inside the loop at :38); here each rank builds the net once, takes every world-th entry
(flownet2_amd.parallel.shard -- no collective on the data path) and batches pairs of equal size.

* Bit-exact outputs whatever the batching / sharding (default; `--no-batch-invariant` trades it for speed): the net runs
  in flownet2_amd.functional's batch-invariant mode, in which no summation order depends on the batch size, so a pair's
  .flo has the same bytes from `run_flownet.py` (batch 1), from this script on 1 GPU and from any N-GPU sharding of the list.
* Host side: every image is decoded ONCE (the size of the next group's first image decides the grouping), by a prefetch
  thread that stays `--prefetch` groups ahead of the GPU and hands over pinned staging buffers (asynchronous H2D copies);
  the .flo files are written by a second thread, so decode, compute and encode of consecutive groups overlap.
* The process group (only a final barrier -- the data path has no exchange) uses gloo: ranks may even share one GPU.
* `--bidirectional`: every pair also runs backwards, (img1, img0), in the same step, and the two flows are checked against each other
  (functional.flow_consistency, one launch).  Beside out.flo the script then writes out.bw.flo (the bytes of a plain run on the swapped
  line), out.occ.pgm and out.bw.occ.pgm (8-bit binary PGM, 255 = occluded, in frame 0 and in frame 1); `--consistency-json PATH` holds
  the per-line summaries, with the same bytes for any --batch and any number of processes.  out.flo keeps the bytes it has without
  the flag (batch-invariant mode).
* `--color`: beside out.flo the script writes out.png, the Middlebury colour coding of the flow (functional.flow_to_color, on the device;
  with --bidirectional also out.bw.png).  Without `--color-max F` every picture is normalised by its own flow's largest radius, so a
  pair's picture does not depend on --batch or on the number of processes; with it, by F, and pictures compare.  `--color-norm batch`
  (the largest radius of the group a pair was computed in) depends on the grouping by construction: it is refused with more than one
  process unless --color-max is given, which then decides.
"""
import argparse
import os
import queue
import sys
import threading

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet2_amd import evaluate, flo, parallel, visualize  # noqa: E402
from flownet2_amd import functional as Fn  # noqa: E402
import run_flownet as RF  # noqa: E402


ARITH = ("conv", "deconv", "wino", "corr")          # the switches of functional.ARITH_SWITCHES this script offers, as --<key>-arith


def color_names(out):
    """What --color writes beside the forward flow `out` (x.flo): (x.png, x.bw.png); a name without the .flo suffix is extended as it
    stands."""
    stem = out[:-4] if out.endswith(".flo") else out
    return stem + ".png", stem + ".bw.png"


def groups_of(entries, batch, read):
    """Yield (entries, img0 [n,3,H,W], img1) groups of at most `batch` consecutive pairs of equal size; every file is read once."""
    pending = None                         # (entry, img0, img1) that closed the previous group
    it = iter(entries)
    while True:
        group = []
        if pending is not None:
            group.append(pending)
            pending = None
        for e in it:
            item = (e, read(e[0]), read(e[1]))
            if group and item[1].shape != group[0][1].shape:
                pending = item
                break
            group.append(item)
            if len(group) == batch:
                break
        if not group:
            return
        yield [g[0] for g in group], np.concatenate([g[1] for g in group]), np.concatenate([g[2] for g in group])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listfile")
    ap.add_argument("--net", choices=["C", "S", "2"], default="C")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prefetch", type=int, default=2, help="groups the decode thread may run ahead of the GPU")
    ap.add_argument("--no-batch-invariant", action="store_true", help="let kernel selection depend on the batch size (faster library "
                    "calls; a pair's bits then depend on the batch it was computed in)")
    ap.add_argument("--gpu", type=int, default=None, help="device index (default: LOCAL_RANK)")
    ap.add_argument("--bidirectional", action="store_true", help="also run (img1, img0); write out.bw.flo, out.occ.pgm and out.bw.occ.pgm")
    ap.add_argument("--consistency-json", default=None, metavar="PATH", help="with --bidirectional: the per-line consistency summaries")
    ap.add_argument("--alpha", type=float, nargs=2, default=[0.01, 0.5], metavar=("A1", "A2"), help="inconsistent: |a+b|^2 > A1 (|a|^2+|b|^2) + A2")
    ap.add_argument("--beta", type=float, nargs=2, default=[0.01, 0.002], metavar=("B1", "B2"), help="motion boundary: |grad|^2 > B1 |a|^2 + B2")
    ap.add_argument("--color", action="store_true", help="also write out.png (with --bidirectional: out.bw.png), the flow's colour coding")
    ap.add_argument("--color-max", type=float, default=None, metavar="F", help="with --color: the radius drawn at full saturation, the same "
                    "for every picture (default: see --color-norm)")
    ap.add_argument("--color-norm", choices=["sample", "batch"], default="sample", help="with --color and without --color-max: normalise by "
                    "the largest radius of the pair's own flow (sample), or of the group it was computed in (batch: the picture then depends "
                    "on --batch and on the sharding, so it is refused with more than one process unless --color-max is given)")
    Fn.add_arithmetic_flags(ap, ARITH)
    Fn.add_general_convolution_flag(ap)
    a = ap.parse_args()
    if a.consistency_json and not a.bidirectional:
        ap.error("--consistency-json needs --bidirectional")
    if (a.color_max is not None or a.color_norm != "sample") and not a.color:
        ap.error("--color-max and --color-norm need --color")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.color and a.color_norm == "batch" and a.color_max is None and world > 1:
        ap.error("--color-norm batch depends on how the list is sharded: give --color-max, or run one process")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")              # control plane only; the data path has no collective
    dev = torch.device("cuda", a.gpu if a.gpu is not None else int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(dev)
    Fn.set_batch_invariant(not a.no_batch_invariant)
    Fn.apply_arithmetic_flags(a, ARITH)
    Fn.apply_general_convolution_flag(a)
    entries = [l.split() for l in open(a.listfile) if l.strip()]
    mine = parallel.shard([e + [i] for i, e in enumerate(entries)])      # the list index travels with the entry (the JSON is in list order)
    parts = []                                                            # --bidirectional: (list indices, FlowConsistency) per group
    P, mean = RF.load_params(a.net, a.weights, dev)

    staged = queue.Queue(maxsize=max(1, a.prefetch))
    done = queue.Queue()
    errors = []

    def producer():
        try:
            for ents, i0, i1 in groups_of(mine, a.batch, RF.read_image):
                staged.put((ents, torch.from_numpy(i0).pin_memory(), torch.from_numpy(i1).pin_memory()))
        except BaseException as e:      # noqa: BLE001 -- surfaced on the main thread
            errors.append(e)
        finally:
            staged.put(None)

    def writer():
        try:
            while True:
                item = done.get()
                if item is None:
                    return
                ents, flow, occ, rgb, ev = item
                ev.synchronize()
                arr = flow.numpy()
                n = len(ents)
                for k, e in enumerate(ents):
                    flo.write_flo(e[2], arr[k])
                    if rgb is not None:
                        png_name, bw_png_name = color_names(e[2])
                        visualize.write_png(png_name, rgb[k].numpy())
                        if occ is not None:
                            visualize.write_png(bw_png_name, rgb[n + k].numpy())
                    if occ is not None:
                        bw_name, occ_name, bw_occ_name = evaluate.bidirectional_names(e[2])
                        flo.write_flo(bw_name, arr[n + k])
                        evaluate.write_pgm(occ_name, occ[k, 0].numpy())
                        evaluate.write_pgm(bw_occ_name, occ[n + k, 0].numpy())
        except BaseException as e:      # noqa: BLE001
            errors.append(e)

    tp, tw = threading.Thread(target=producer, daemon=True), threading.Thread(target=writer, daemon=True)
    tp.start(); tw.start()
    while True:
        item = staged.get()
        if item is None:
            break
        ents, h0, h1 = item
        i0, i1 = h0.to(dev, non_blocking=True), h1.to(dev, non_blocking=True)
        occ_host = None
        if a.bidirectional:
            n = i0.shape[0]
            flow = RF.infer(a.net, P, torch.cat([i0, i1]), torch.cat([i1, i0]), mean)      # rows 0 .. n-1 forward, n .. 2n-1 backward
            with torch.no_grad():
                c = Fn.flow_consistency(flow[:n], flow[n:], alpha=tuple(a.alpha), beta=tuple(a.beta))
            occ = torch.cat([c.occ_fw, c.occ_bw])
            occ_host = torch.empty(occ.shape, dtype=occ.dtype, pin_memory=True)
            occ_host.copy_(occ, non_blocking=True)
            parts.append(([e[-1] for e in ents], c))
        else:
            flow = RF.infer(a.net, P, i0, i1, mean)
        rgb_host = None
        if a.color:
            with torch.no_grad():
                rgb = Fn.flow_to_color(flow.detach().contiguous(), max_flow=a.color_max, norm=a.color_norm)
            rgb_host = torch.empty(rgb.shape, dtype=rgb.dtype, pin_memory=True)
            rgb_host.copy_(rgb, non_blocking=True)
        host = torch.empty(flow.shape, dtype=flow.dtype, pin_memory=True)
        host.copy_(flow, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        done.put((ents, host, occ_host, rgb_host, ev))
    done.put(None)
    tw.join(); tp.join()
    if errors:
        raise errors[0]
    my_rank = parallel.rank()
    if a.consistency_json:
        result = evaluate.gather_consistency(len(entries), parts, alpha=a.alpha, beta=a.beta)
        if my_rank == 0:
            with open(a.consistency_json, "w") as f:
                f.write(result.to_json())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if my_rank == 0:
        print(f"{len(entries)} pairs, {world} rank(s), batch-invariant {'off' if a.no_batch_invariant else 'on'}")


if __name__ == "__main__":
    main()
