#!/usr/bin/env python3
"""Times K21: the two device entries of split_large_nuclei (som_device.nuclear_overlaps, split_nuclei_apply) and the
whole chain (som_device.split_large_nuclei, host choice and read-backs included) on synthetic 2048 x 2048 planes -- Voronoi
cells with shifted, eroded nuclei (tests/split_nuclei_reference.py) -- under HIP events, and the literal numpy loop of the
reference's algorithm (split_loop: two full-image masks per cell) once on the same host at a size where it finishes in
seconds.

    python scripts/split_nuclei_bench.py [--size 2048] [--cells 20000] [--reps 10] [--host-size 512]
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
from tests import split_nuclei_reference as snr  # noqa: E402


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
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-size", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda")
    cell, nuc = snr.voronoi_case(args.size, args.size, args.cells, args.size)
    ct, nt = torch.from_numpy(cell).to(dev), torch.from_numpy(nuc).to(dev)
    print("device: %s; planes %d x %d int32" % (torch.cuda.get_device_name(0), args.size, args.size))
    keys, nuc_keys, best, inside, area = som_device.nuclear_overlaps(ct, nt)
    ids = keys.cpu().numpy()
    tables = som_device.choose_splits(ids, nuc_keys.cpu().numpy(), best.cpu().numpy(), inside.cpu().numpy(),
                                      area.cpu().numpy(), ids)
    chosen, cell_value, nuc_value = (torch.from_numpy(t).to(dev) for t in tables[:3])
    print("%d cells, %d nuclei, %d splits" % (keys.numel(), nuc_keys.numel(), tables[3]))
    for name, fn in (("label_keys (both planes)", lambda: (som_device.label_keys(ct), som_device.label_keys(nt))),
                     ("nuclear_overlaps (two calls, one read-back; keys given)",
                      lambda: som_device.nuclear_overlaps(ct, nt, keys, nuc_keys)),
                     ("nuclear_overlaps, binary search", lambda: som_device.nuclear_overlaps(ct, nt, keys, nuc_keys, True)),
                     ("split_nuclei_apply", lambda: som_device.split_nuclei_apply(ct, nt, keys, nuc_keys, chosen, cell_value,
                                                                                  nuc_value)),
                     ("split_large_nuclei (whole chain, host choice included)",
                      lambda: som_device.split_large_nuclei(ct, nt))):
        med, low = timed(fn, args.reps)
        print("%-58s median %9.3f ms   min %9.3f ms   (%d reps, HIP events)" % (name, med, low, args.reps))

    n_host = max(args.cells * args.host_size ** 2 // args.size ** 2, 8)
    hc, hn = snr.voronoi_case(args.host_size, args.host_size, n_host, args.host_size)
    hids = np.unique(hc)
    hids = hids[hids != 0]
    t0 = time.perf_counter()
    want, n_splits = snr.split_loop(hc, hn, hids)
    host_s = time.perf_counter() - t0
    hct, hnt = torch.from_numpy(hc).to(dev), torch.from_numpy(hn).to(dev)
    same = np.array_equal(som_device.split_large_nuclei(hct, hnt).cpu().numpy(), want)
    med, _ = timed(lambda: som_device.split_large_nuclei(hct, hnt), args.reps)
    print("host loop (the reference's algorithm in numpy) at %d x %d, %d cells, %d splits: %.3f s once; device chain on the "
          "same planes %.3f ms; equal: %s" % (args.host_size, args.host_size, hids.size, n_splits, host_s, med, same))


if __name__ == "__main__":
    main()
