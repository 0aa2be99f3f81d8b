#!/usr/bin/env python
"""Times the fibre object table kernels on one GPU:

  - neighbours: 100 FOVs x 2 000 fibres on a 2048 x 2048 field, k = 4.  kernel_us: one pxsom_nearest_indices launch;
    call_us: som_device.nearest_indices with its checks (one small read-back); alignment_us: calculate_fiber_alignment
    over the whole table, host arithmetic and merge included (wall clock).  On the same host, over the first
    ``--host-fovs`` FOVs and scaled to all of them: loop_us, the reference's loop (cdist, then argsort()[1 : 1 + k] fibre
    by fibre), and numpy_us, the numpy statement (the matrix of s, one stable argsort per row).  The indices must equal
    the statement's.
  - objects: a 2048 x 2048 int32 label plane of 3 000 drawn fibres.  euler_entry_us: one pxsom_region_euler call through
    the C ABI (clearing, the key LUT, the pass over the windows, the division); euler_call_us: som_device.region_euler
    with its checks (one small read-back); moments_call_us: som_device.region_moments likewise; props_us:
    fiber_object_props from the host plane to the frame (wall clock, upload included); numpy_euler_us: the numpy
    statement of the bit quads on the host.  The Euler numbers must equal the statement's.

Device times are HIP events around single calls, the median of ``--reps`` (10); host times are one run.  Indicative
figures: nothing here is a pass mark.

    python scripts/fiber_bench.py [--fovs 100] [--per-fov 2000] [--k 4] [--side 2048] [--fibres 3000] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_us(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(times))


def reference_loop(xy, k):
    """The reference's loop over one FOV: [n, k] neighbour positions."""
    from scipy.spatial.distance import cdist
    dist = cdist(xy, xy)
    return np.stack([dist[i, :].argsort()[1:1 + k] for i in range(len(xy))])


def numpy_statement(xy, k):
    dx = xy[:, None, 0] - xy[None, :, 0]
    dy = xy[:, None, 1] - xy[None, :, 1]
    s = dx * dx + dy * dy
    np.fill_diagonal(s, np.inf)            # excluded by identity: behind every real candidate
    return np.argsort(s, axis=1, kind="stable")[:, :k]


def bench_neighbours(args):
    import pandas as pd
    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    dev = _capi.require_gpu()
    n_fovs, per_fov, k = args.fovs, args.per_fov, args.k
    n = n_fovs * per_fov
    rs = np.random.RandomState(23)
    xy = rs.uniform(0, args.side, (n, 2))
    seg = (np.arange(n_fovs + 1) * per_fov).astype(np.int64)
    xy_d, seg_d = torch.from_numpy(xy).to(dev), torch.from_numpy(seg).to(dev)
    out = torch.empty((n, k), dtype=torch.int32, device=dev)
    lib, st = _capi.lib(), _capi.stream_ptr()

    def launch():
        _capi.check(lib.pxsom_nearest_indices(xy_d.data_ptr(), seg_d.data_ptr(), n_fovs, n, k, out.data_ptr(), st),
                    "pxsom_nearest_indices")
    kernel_us = _median_us(launch, args.reps)
    call_us = _median_us(lambda: som_device.nearest_indices(xy_d, seg_d, k), args.reps)
    got = out.cpu().numpy()

    table = pd.DataFrame({"fov": np.repeat(["fov%03d" % f for f in range(n_fovs)], per_fov),
                          "label": np.tile(np.arange(1, per_fov + 1), n_fovs), "centroid-0": xy[:, 0],
                          "centroid-1": xy[:, 1], "major_axis_length": 30.0, "minor_axis_length": 3.0,
                          "orientation": rs.uniform(-np.pi / 2, np.pi / 2, n)})
    fs.calculate_fiber_alignment(table, k=k)
    t0 = time.perf_counter()
    scored = fs.calculate_fiber_alignment(table, k=k)
    alignment_us = (time.perf_counter() - t0) * 1e6
    assert np.isfinite(scored["alignment_score"].to_numpy()).all()

    host_fovs = min(args.host_fovs, n_fovs)
    t0 = time.perf_counter()
    loop = [reference_loop(xy[a:b], k) + a for a, b in zip(seg[:host_fovs], seg[1:host_fovs + 1])]
    loop_us = (time.perf_counter() - t0) * 1e6 * n_fovs / host_fovs
    t0 = time.perf_counter()
    stmt = [numpy_statement(xy[a:b], k) + a for a, b in zip(seg[:host_fovs], seg[1:host_fovs + 1])]
    numpy_us = (time.perf_counter() - t0) * 1e6 * n_fovs / host_fovs
    assert np.array_equal(got[:host_fovs * per_fov], np.concatenate(stmt)), "indices differ from the numpy statement"
    assert np.array_equal(got[:host_fovs * per_fov], np.concatenate(loop)), "indices differ from the reference's loop"
    print(json.dumps({"what": "neighbours", "fovs": n_fovs, "fibres_per_fov": per_fov, "k": k,
                      "kernel_us": round(kernel_us, 1), "call_us": round(call_us, 1),
                      "alignment_us": round(alignment_us, 1), "host_fovs_timed": host_fovs,
                      "loop_us": round(loop_us, 1), "numpy_us": round(numpy_us, 1),
                      "loop_over_call": round(loop_us / call_us, 1), "numpy_over_call": round(numpy_us / call_us, 1),
                      "pairs_per_us": round(n_fovs * per_fov * per_fov / kernel_us, 1)}), flush=True)


def fibre_plane(side, fibres, seed=23):
    rs = np.random.RandomState(seed)
    seg = np.zeros((side, side), dtype=np.int32)
    for lab in range(1, fibres + 1):
        r, c, angle, length = rs.uniform(0, side), rs.uniform(0, side), rs.uniform(0, np.pi), rs.uniform(30, 300)
        t = np.arange(0, length, 0.5)
        rr = np.round(r + t * np.sin(angle)).astype(np.int64)
        cc = np.round(c + t * np.cos(angle)).astype(np.int64)
        for dr in (0, 1):
            for dc in (0, 1):
                ok = (rr + dr >= 0) & (rr + dr < side) & (cc + dc >= 0) & (cc + dc < side)
                seg[rr[ok] + dr, cc[ok] + dc] = lab
    return seg


def bench_objects(args):
    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    from ark_analysis_amd.segmentation import regionprops_extraction as rpe
    dev = _capi.require_gpu()
    seg = fibre_plane(args.side, args.fibres)
    seg_d = torch.from_numpy(seg).to(dev)
    keys = som_device.label_keys(seg_d)
    euler = torch.empty(keys.numel(), dtype=torch.int64, device=dev)
    euler_us = _median_us(lambda: som_device.region_euler(seg_d, keys=keys, out=euler), args.reps)
    moments_us = _median_us(lambda: som_device.region_moments(seg_d, keys=keys), args.reps)
    lib, st = _capi.lib(), _capi.stream_ptr()
    kmin, kmax = (int(v) for v in keys[[0, -1]].cpu())
    wsb = lib.pxsom_region_euler_workspace_bytes(keys.numel(), kmin, kmax, 0)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)

    def entry():
        _capi.check(lib.pxsom_region_euler(seg_d.data_ptr(), som_device.SEG_DTYPES[seg_d.dtype], args.side, args.side,
                                           args.side, keys.data_ptr(), keys.numel(), kmin, kmax, euler.data_ptr(),
                                           ws.data_ptr(), wsb, 0, st), "pxsom_region_euler")
    entry_us = _median_us(entry, args.reps)
    fs.fiber_object_props(seg, "fov")
    t0 = time.perf_counter()
    table = fs.fiber_object_props(seg, "fov")
    props_us = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    want = rpe.euler_numbers(seg, keys.cpu().numpy())
    numpy_euler_us = (time.perf_counter() - t0) * 1e6
    assert np.array_equal(euler.cpu().numpy(), want), "Euler numbers differ from the numpy statement"
    assert np.array_equal(table["euler_number"].to_numpy(), want)
    print(json.dumps({"what": "objects", "side": args.side, "objects": int(keys.numel()),
                      "longest_major_axis": round(float(table["major_axis_length"].max()), 1),
                      "euler_entry_us": round(entry_us, 1), "euler_call_us": round(euler_us, 1), "moments_call_us": round(moments_us, 1),
                      "props_us": round(props_us, 1), "numpy_euler_us": round(numpy_euler_us, 1),
                      "numpy_euler_over_call": round(numpy_euler_us / euler_us, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fovs", type=int, default=100)
    ap.add_argument("--per-fov", type=int, default=2000)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--fibres", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-fovs", type=int, default=5, help="FOVs the host baselines are timed over")
    args = ap.parse_args()
    bench_neighbours(args)
    bench_objects(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
