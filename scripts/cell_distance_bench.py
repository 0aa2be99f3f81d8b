#!/usr/bin/env python
"""Times the cell-distance kernel (pxsom_nearest_type_means) on uniform random centroids over a
2048 x 2048 field with 20 phenotypes and k = 5:

  - kernel_us: one pxsom_nearest_type_means launch on rows already sorted by type (HIP events over back-to-back launches
    on one stream), and counts_kernel_us: pxsom_neighbor_counts (distlim 50) on the same rows in the same run, with the
    ratio of the two;
  - call_us: som_device.nearest_type_means as the package calls it -- the checks (one small read-back), the sort by
    (FOV, type), the launch and the scatter back to the caller's order (HIP events over back-to-back calls);
  - numpy_us: the reference's statement per FOV (cdist, astype(float32), then per phenotype where(> 0), sort, the mean of
    the first k) timed in the same run on this host, at the sizes where its N x N float64 matrix fits in memory; the
    outputs must be equal bit for bit, NaN in the same places.

Every case runs in a child process of its own under a time limit; the first case that fails or runs over ends the run.
The run fails unless, at 10 000 cells, the device call is faster than the numpy statement.

    python scripts/cell_distance_bench.py [--cases 1x2000 1x10000 1x50000 20x5000] [--k 5] [--reps 20] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELD, N_TYPES, DISTLIM = 2048.0, 20, 50
NUMPY_MAX_CELLS = 12000        # the statement's float64 matrix: 8 N^2 bytes, 1.2 GB at 12 000


def numpy_statement(xy, types, seg, k):
    from scipy.spatial.distance import cdist
    out = np.full((len(xy), N_TYPES), np.nan, dtype=np.float32)
    for a, b in zip(seg[:-1], seg[1:]):
        dist = cdist(xy[a:b], xy[a:b]).astype(np.float32)
        for t in range(N_TYPES):
            cols = np.flatnonzero(types[a:b] == t)
            if len(cols) < k:
                continue
            d = np.ascontiguousarray(dist[:, cols])
            d = np.sort(np.where(d > 0, d, np.float32(np.nan)), axis=1)
            out[a:b, t] = d[:, :k].mean(axis=1)
    return out


def _events_us(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def run_case(case, k, reps):
    import torch
    from ark_analysis_amd import _capi, som_device
    dev = _capi.require_gpu()
    n_fovs, per_fov = (int(v) for v in case.split("x"))
    n = n_fovs * per_fov
    rs = np.random.RandomState(n_fovs * 1000003 + per_fov)
    xy = rs.uniform(0, FIELD, (n, 2))
    types = rs.randint(0, N_TYPES, n).astype(np.int64)
    seg = (np.arange(n_fovs + 1) * per_fov).astype(np.int64)
    xy_d, ty_d, seg_d = (torch.from_numpy(a).to(dev) for a in (xy, types, seg))

    got = som_device.nearest_type_means(xy_d, ty_d, seg_d, N_TYPES, k)
    call_us = _events_us(lambda: som_device.nearest_type_means(xy_d, ty_d, seg_d, N_TYPES, k), reps)

    order = np.concatenate([a + np.argsort(types[a:b], kind="stable") for a, b in zip(seg[:-1], seg[1:])])
    xy_s = torch.from_numpy(xy[order]).to(dev)
    ty_s = torch.from_numpy(types[order].astype(np.int32)).to(dev)
    out = torch.empty((n, N_TYPES), dtype=torch.float32, device=dev)
    counts = torch.empty((n, N_TYPES), dtype=torch.int32, device=dev)
    s_lim, s_zero = som_device.neighbor_thresholds(DISTLIM)
    lib, st = _capi.lib(), _capi.stream_ptr()

    def launch():
        _capi.check(lib.pxsom_nearest_type_means(xy_s.data_ptr(), ty_s.data_ptr(), seg_d.data_ptr(), n_fovs, n, N_TYPES,
                                                 k, s_zero, out.data_ptr(), st), "pxsom_nearest_type_means")

    def launch_counts():
        _capi.check(lib.pxsom_neighbor_counts(xy_s.data_ptr(), ty_s.data_ptr(), seg_d.data_ptr(), n_fovs, n, N_TYPES,
                                              s_lim, s_zero, 0, counts.data_ptr(), st), "pxsom_neighbor_counts")
    kernel_us = _events_us(launch, reps)
    counts_kernel_us = _events_us(launch_counts, reps)
    kernel_us_again = _events_us(launch, reps)
    same = out.view(torch.int32) == got[torch.from_numpy(order).to(dev)].view(torch.int32)
    assert bool((same | (out != out)).all())

    rec = {"fovs": n_fovs, "cells_per_fov": per_fov, "types": N_TYPES, "k": k,
           "kernel_us": round(min(kernel_us, kernel_us_again), 1), "counts_kernel_us": round(counts_kernel_us, 1),
           "kernel_over_counts_kernel": round(min(kernel_us, kernel_us_again) / counts_kernel_us, 2),
           "call_us": round(call_us, 1),
           "pairs_per_us": round(n_fovs * per_fov * per_fov / min(kernel_us, kernel_us_again), 1)}
    if per_fov <= NUMPY_MAX_CELLS:
        t0 = time.perf_counter()
        want = numpy_statement(xy, types, seg, k)
        rec["numpy_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        host = got.cpu().numpy()
        assert np.array_equal(np.isnan(host), np.isnan(want)), "NaN positions differ from the numpy statement"
        ok = ~np.isnan(want)
        assert np.array_equal(host.view(np.uint32)[ok], want.view(np.uint32)[ok]), "bits differ from the numpy statement"
        rec["numpy_over_call"] = round(rec["numpy_us"] / call_us, 1)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["1x2000", "1x10000", "1x50000", "20x5000"])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds per case")
    ap.add_argument("--case", help=argparse.SUPPRESS)      # the child's one case
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.k, args.reps)
        return 0
    for case in args.cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--k", str(args.k), "--reps", str(args.reps)]
        try:
            res = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print("case %s ran over %d s: stopping" % (case, args.limit), file=sys.stderr)
            return 1
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            print("case %s failed with status %d: stopping" % (case, res.returncode), file=sys.stderr)
            return 1
        if case == "1x10000":
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            if not rec["numpy_us"] > rec["call_us"]:
                print("at 10 000 cells the device call (%.1f us) is not faster than the numpy statement (%.1f us)"
                      % (rec["call_us"], rec["numpy_us"]), file=sys.stderr)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
