#!/usr/bin/env python3
"""Times K18: the device chain of merge_masks_single (som_device.merge_masks) on synthetic 2048 x 2048 masks -- a few
thousand discs as cells, a few hundred blobs as objects -- under HIP events, stage by stage and as a whole, and the numpy
statement of the same contract (tests/merge_masks_reference.py) once on the same host at a size where it finishes in
seconds.

    python scripts/merge_masks_bench.py [--size 2048] [--cells 6000] [--objects 400] [--reps 10] [--host-size 256]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ark_analysis_amd import som_device  # noqa: E402
from tests import merge_masks_reference as mmr  # noqa: E402


def masks(rs, size, n_cells, n_objects):
    scale = size / 2048.0
    # (the windowed painter: the same masks as random_masks, without a whole-image pass per disc)
    return mmr.random_masks_windowed(rs, size, size, n_cells, n_objects, cell_r=(6, 12),
                                     object_r=(max(8, int(20 * scale)), max(12, int(45 * scale))))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=6000)
    ap.add_argument("--objects", type=int, default=400)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-size", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda")
    rs = np.random.RandomState(18)
    objects, cells = masks(rs, args.size, args.cells, args.objects)
    ot, ct = torch.from_numpy(objects).to(dev), torch.from_numpy(cells).to(dev)
    print("device: %s; masks %d x %d int32" % (torch.cuda.get_device_name(0), args.size, args.size))
    ol, n_o, _ = som_device.label_regions(ot, 2)
    cl, n_c, _ = som_device.label_regions(ct, 2)
    n_o, n_c = int(n_o.item()), int(n_c.item())
    pairs = som_device.pair_overlaps(ol, cl, n_o, n_c)
    print("regions: %d objects, %d cells, %d overlapping pairs" % (n_o, n_c, pairs.shape[0]))
    winner = torch.zeros(n_c + 1, dtype=torch.int32, device=dev)
    removed = torch.zeros(n_c + 1, dtype=torch.int32, device=dev)
    for name, fn in (("label_regions (cells)", lambda: som_device.label_regions(ct, 2)),
                     ("label_components (cells != 0, K16)", lambda: som_device.label_components((ct != 0), 2)),
                     ("pair_overlaps (two calls, one read-back)", lambda: som_device.pair_overlaps(ol, cl, n_o, n_c)),
                     ("merge_apply", lambda: som_device.merge_apply(ol, cl, winner, removed)),
                     ("merge_masks (whole chain, host choice included)", lambda: som_device.merge_masks(ot, ct, 10, 10))):
        med, best = timed(fn, args.reps)
        print("%-50s median %9.3f ms   min %9.3f ms   (%d reps, HIP events)" % (name, med, best, args.reps))
    merged, remaining = som_device.merge_masks(ot, ct, 10, 10)
    print("merged cells: %d" % (n_c - (torch.unique(remaining).numel() - 1)))

    ho, hc = masks(np.random.RandomState(19), args.host_size, max(args.cells * args.host_size ** 2 // args.size ** 2, 8),
                   max(args.objects * args.host_size ** 2 // args.size ** 2, 2))
    t0 = time.perf_counter()
    want = mmr.merge_masks(ho, hc, 10, 10)
    host_s = time.perf_counter() - t0
    got = som_device.merge_masks(torch.from_numpy(ho).to(dev), torch.from_numpy(hc).to(dev), 10, 10)
    same = np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    med, _ = timed(lambda: som_device.merge_masks(torch.from_numpy(ho).to(dev), torch.from_numpy(hc).to(dev), 10, 10), args.reps)
    print("host statement (numpy + scipy loops) at %d x %d: %.3f s once; device chain on the same masks %.3f ms; equal: %s"
          % (args.host_size, args.host_size, host_s, med, same))


if __name__ == "__main__":
    main()
