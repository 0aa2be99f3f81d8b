#!/usr/bin/env python
"""Times the two k-means routes of the neighbourhood workflow on rows drawn as Poisson counts:

  - sweep: compute_kmeans_inertia, k = 2 .. 10, one fit per k;
  - labelling: generate_cluster_labels at k = 10, ten restarts;

each with kmeans="host" (scikit-learn's KMeans on this host's threads) and kmeans="device" (kmeans_fits_device: the init
draws on the host, the upload, one pxsom_kmeans_lloyd call, the labels back), alternating, after one warm-up call of each;
wall-clock around calls that end with their results on the host.  Medians and the spread (min .. max) are printed.

  - pass: pxsom_kmeans_lloyd alone on the sweep's nine problems with tol = 0 and max_iter = --pass-iters (HIP events
    around the call), divided by the iterations it ran: the time of one iteration -- one assignment pass, the fold and
    the update, the read-back -- beside the bytes an iteration must move (the rows twice, labels read and written, the
    winning distances written).

    python scripts/kmeans_bench.py [--n 200000] [--d 20] [--reps 3] [--pass-iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = list(range(2, 11))


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _summary(times):
    return {"median_s": round(float(np.median(times)), 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pass-iters", type=int, default=20)
    args = ap.parse_args()

    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    dev = _capi.require_gpu()
    rs = np.random.RandomState(args.n)
    arche = rs.choice([0.3, 2.0, 6.0], size=(8, args.d))
    x = rs.poisson(arche[rs.randint(0, 8, args.n)]).astype(np.float64)
    frame = pd.DataFrame(x, columns=["type%d" % t for t in range(args.d)])
    small = frame.iloc[:2000]
    threads = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count()))

    jobs = {"sweep": lambda data, route: sau.compute_kmeans_inertia(data, 2, 10, seed=42, kmeans=route).to_numpy(),
            "labelling": lambda data, route: sau.generate_cluster_labels(data, 10, seed=42, kmeans=route)}
    for name, job in jobs.items():
        for route in ("host", "device"):
            job(small, route)                                        # warm-up: code objects, thread pools
        times, last = {"host": [], "device": []}, {}
        for _ in range(args.reps):
            for route in ("host", "device"):
                t, last[route] = _timed(lambda: job(frame, route))
                times[route].append(t)
        rec = {"job": name, "n": args.n, "d": args.d, "host_threads": threads, "reps": args.reps,
               "host": _summary(times["host"]), "device": _summary(times["device"])}
        rec["host_over_device"] = round(rec["host"]["median_s"] / rec["device"]["median_s"], 2)
        if name == "sweep":
            rec["inertia_device_over_host"] = [round(float(v), 6) for v in last["device"] / last["host"]]
        print(json.dumps(rec), flush=True)

    x_d = torch.from_numpy(x - x.mean(axis=0)).to(dev)
    inits = [np.ascontiguousarray((x - x.mean(axis=0))[rs.choice(args.n, k, replace=False)]) for k in KS]
    som_device.kmeans_lloyd(x_d, inits, 0.0, 2)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    n_iter = som_device.kmeans_lloyd(x_d, inits, 0.0, args.pass_iters)[3]
    e1.record()
    torch.cuda.synchronize()
    passes = int(n_iter.max()) + 1                                   # the closing pass of the problems that ran out
    per_pass_us = e0.elapsed_time(e1) * 1e3 / passes
    moved = args.n * (2 * args.d * 8 + len(KS) * (4 + 4 + 8))
    print(json.dumps({"job": "pass", "n": args.n, "d": args.d, "problems": len(KS), "centres": sum(KS),
                      "groups": som_device.kmeans_group_count(args.d, KS), "iterations": [int(v) for v in n_iter],
                      "per_iteration_us": round(per_pass_us, 1), "bytes_per_iteration": moved,
                      "tb_per_s": round(moved / per_pass_us * 1e-6, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
