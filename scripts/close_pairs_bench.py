#!/usr/bin/env python
"""Times the close-pair counts (pxsom_close_pair_counts) on a cohort of uniform random centroids over
2048 x 2048 fields with distlim 50, every cell in each of S sets with probability 0.3, against the route the package
offered before the kernel: one som_device.neighbor_counts call per set with binary types (is the candidate in set t?),
which gives the [n, S] table of close candidates per set, then per FOV the product of the transposed [n, S] membership
matrix with that table (torch.bmm in float64 on the device: integers far below 2^53).

  - kernel_us: one pxsom_close_pair_counts launch, the clearing of the output included (HIP events over back-to-back
    launches on one stream);
  - call_us: som_device.close_pair_counts as the package calls it (the checks with their one small read-back);
  - composed_us: the S neighbor_counts calls and the product; the two results must be equal.

Every case runs in a child process of its own under a time limit; the first case that fails or runs over ends the run.
The run fails unless, at 20 sets, the device call is no slower than the composed route.

    python scripts/close_pairs_bench.py [--cohort 100x5000] [--sets 2 20 64] [--reps 10] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELD, DISTLIM, DENSITY = 2048.0, 50, 0.3


def _events_us(fn, reps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def run_case(cohort, n_sets, reps):
    import torch
    from ark_analysis_amd import _capi, som_device
    dev = _capi.require_gpu()
    n_fovs, per_fov = (int(v) for v in cohort.split("x"))
    n = n_fovs * per_fov
    rs = np.random.RandomState(n_fovs * 1000003 + per_fov + n_sets)
    xy = rs.uniform(0, FIELD, (n, 2))
    member = rs.rand(n, n_sets) < DENSITY
    mask = np.zeros(n, dtype=np.uint64)
    for s in range(n_sets):
        mask |= member[:, s].astype(np.uint64) << np.uint64(s)
    seg = (np.arange(n_fovs + 1) * per_fov).astype(np.int64)
    xy_d, seg_d = torch.from_numpy(xy).to(dev), torch.from_numpy(seg).to(dev)
    mask_d = torch.from_numpy(mask.view(np.int64)).to(dev)
    member_d = torch.from_numpy(member).to(dev)

    got = som_device.close_pair_counts(xy_d, mask_d, mask_d, seg_d, n_sets, n_sets, DISTLIM)
    call_us = _events_us(lambda: som_device.close_pair_counts(xy_d, mask_d, mask_d, seg_d, n_sets, n_sets, DISTLIM), reps)

    out = torch.empty_like(got)
    s_lim, s_zero = som_device.neighbor_thresholds(DISTLIM)
    lib, st = _capi.lib(), _capi.stream_ptr()

    def launch():
        _capi.check(lib.pxsom_close_pair_counts(xy_d.data_ptr(), mask_d.data_ptr(), mask_d.data_ptr(), seg_d.data_ptr(),
                                                n_fovs, n, n_sets, n_sets, s_lim, s_zero, 0, out.data_ptr(), st),
                    "pxsom_close_pair_counts")
    kernel_us = _events_us(launch, reps)
    assert torch.equal(out, got)

    def composed():
        close = torch.empty((n, n_sets), dtype=torch.float64, device=dev)
        for t in range(n_sets):
            close[:, t] = som_device.neighbor_counts(xy_d, member_d[:, t].to(torch.int64), seg_d, 2, DISTLIM)[:, 1]
        q = member_d.to(torch.float64).view(n_fovs, per_fov, n_sets).transpose(1, 2)
        return torch.bmm(q, close.view(n_fovs, per_fov, n_sets)).to(torch.int64)
    want = composed()
    assert torch.equal(got, want), "the kernel's counts differ from the composed route's"
    composed_us = _events_us(composed, max(reps // 5, 2))

    print(json.dumps({"fovs": n_fovs, "cells_per_fov": per_fov, "sets": n_sets, "distlim": DISTLIM,
                      "close_pairs": int(got.sum().item()), "kernel_us": round(kernel_us, 1), "call_us": round(call_us, 1),
                      "composed_us": round(composed_us, 1), "composed_over_call": round(composed_us / call_us, 1),
                      "pairs_per_us": round(n_fovs * per_fov * per_fov / kernel_us, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cohort", default="100x5000", help="FOVs x cells per FOV")
    ap.add_argument("--sets", nargs="+", type=int, default=[2, 20, 64])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300, help="seconds per case")
    ap.add_argument("--case", type=int, help=argparse.SUPPRESS)      # the child's one set count
    args = ap.parse_args()
    if args.case:
        run_case(args.cohort, args.case, args.reps)
        return 0
    for n_sets in args.sets:
        cmd = [sys.executable, os.path.abspath(__file__), "--cohort", args.cohort, "--case", str(n_sets), "--reps",
               str(args.reps)]
        try:
            res = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print("%d sets ran over %d s: stopping" % (n_sets, args.limit), file=sys.stderr)
            return 1
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            print("%d sets failed with status %d: stopping" % (n_sets, res.returncode), file=sys.stderr)
            return 1
        if n_sets == 20:
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            if rec["call_us"] > rec["composed_us"]:
                print("at 20 sets the device call (%.1f us) is slower than the composed route (%.1f us)"
                      % (rec["call_us"], rec["composed_us"]), file=sys.stderr)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
