#!/usr/bin/env python
"""Times the spatial-LDA neighbourhood sums (pxsom_neighborhood_sums) on uniform random centroids over a
2048 x 2048 field at radius 50:

  - kernel_us: one pxsom_neighborhood_sums launch with P feature columns (HIP events over back-to-back launches on one
    stream), for P = 0 (counts only), 8 (one chunk) and the featurisation's own width;
  - featurize_us: ark_analysis_amd.spLDA.processing.neighborhood_features for the "cluster" featurisation with 20
    clusters as the package calls it -- the frames to arrays, the copy to the device, the launch, the copy back and the
    result frame (wall clock, best of three);
  - numpy_us: the statement per FOV timed in the same run on this host -- the distance matrix with
    sqrt(dx * dx + dy * dy) < radius and one matrix product with the features -- at the sizes where its N x N float64
    matrix fits in memory; the counts must be equal and the sums, which the statement adds in another order, close.

Every case runs in a child process of its own under a time limit; the first case that fails or runs over ends the run.

    python scripts/splda_bench.py [--cases 1x2000 1x10000 1x50000 20x5000] [--reps 20] [--limit 300]
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

FIELD, N_CLUSTERS, RADIUS = 2048.0, 20, 50
NUMPY_MAX_CELLS = 12000        # the statement's float64 matrix: 8 N^2 bytes, 1.2 GB at 12 000


def numpy_statement(xy, feats, seg):
    sums = np.zeros_like(feats)
    counts = np.zeros(len(xy), dtype=np.int32)
    for a, b in zip(seg[:-1], seg[1:]):
        dx = xy[a:b, None, 0] - xy[None, a:b, 0]
        dy = xy[a:b, None, 1] - xy[None, a:b, 1]
        inside = (np.sqrt(dx * dx + dy * dy) < RADIUS).astype(np.float64)
        counts[a:b] = inside.sum(axis=1)
        sums[a:b] = inside.dot(feats[a:b])
    return sums, counts


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


def run_case(case, reps):
    import pandas as pd
    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.spLDA import processing as pros
    dev = _capi.require_gpu()
    n_fovs, per_fov = (int(v) for v in case.split("x"))
    n = n_fovs * per_fov
    rs = np.random.RandomState(n_fovs * 1000003 + per_fov)
    xy = rs.uniform(0, FIELD, (n, 2))
    clusters = rs.randint(0, N_CLUSTERS, n)
    feats = np.zeros((n, N_CLUSTERS))
    feats[np.arange(n), clusters] = 1.0
    seg = (np.arange(n_fovs + 1) * per_fov).astype(np.int64)
    xy_d, feats_d, seg_d = (torch.from_numpy(a).to(dev) for a in (xy, feats, seg))
    s_lim = som_device.radius_threshold(RADIUS)
    lib, st = _capi.lib(), _capi.stream_ptr()
    counts_d = torch.empty((n,), dtype=torch.int32, device=dev)
    rec = {"fovs": n_fovs, "cells_per_fov": per_fov, "radius": RADIUS}
    for p in (0, 8, N_CLUSTERS):
        f_d = feats_d[:, :p].contiguous() if p else None
        sums_d = torch.empty((n, p), dtype=torch.float64, device=dev)

        def launch():
            _capi.check(lib.pxsom_neighborhood_sums(xy_d.data_ptr(), f_d.data_ptr() if p else None, seg_d.data_ptr(),
                                                    n_fovs, n, p, s_lim, sums_d.data_ptr() if p else None,
                                                    counts_d.data_ptr(), st), "pxsom_neighborhood_sums")
        rec["kernel_us_p%d" % p] = round(_events_us(launch, reps), 1)
    got_sums, got_counts = sums_d.cpu().numpy(), counts_d.cpu().numpy()
    rec["mean_neighbors"] = round(float(got_counts.mean()), 1)
    rec["pairs_per_us_p%d" % N_CLUSTERS] = round(n_fovs * per_fov * per_fov / rec["kernel_us_p%d" % N_CLUSTERS], 1)

    table = {}
    for f in range(n_fovs):
        a, b = seg[f], seg[f + 1]
        table["fov%d" % f] = pd.DataFrame({"x": xy[a:b, 0], "y": xy[a:b, 1], "cluster": clusters[a:b], "is_index": True})
    table.update({"fovs": np.array(["fov%d" % f for f in range(n_fovs)]), "markers": None,
                  "clusters": list(range(N_CLUSTERS))})
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        frame = pros.neighborhood_features(table, "cluster", RADIUS)
        dt = (time.perf_counter() - t0) * 1e6
        best = dt if best is None else min(best, dt)
    rec["featurize_us"] = round(best, 1)
    assert np.array_equal(frame.to_numpy(), got_sums.astype(np.int64))

    if per_fov <= NUMPY_MAX_CELLS:
        t0 = time.perf_counter()
        want_sums, want_counts = numpy_statement(xy, feats, seg)
        rec["numpy_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        assert np.array_equal(got_counts, want_counts), "device counts differ from the numpy statement"
        assert np.allclose(got_sums, want_sums, rtol=1e-12, atol=0), "device sums differ from the numpy statement"
        rec["numpy_over_featurize"] = round(rec["numpy_us"] / rec["featurize_us"], 1)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["1x2000", "1x10000", "1x50000", "20x5000"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds per case")
    ap.add_argument("--case", help=argparse.SUPPRESS)      # the child's one case
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.reps)
        return 0
    for case in args.cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps)]
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
