#!/usr/bin/env python
"""Times the silhouette sweep (pxsom_silhouette) on rows drawn as Poisson counts, d = 20 columns, under
the nine labelings k = 2 .. 10 of a sweep (Voronoi cells of k of the rows):

  - kernel_us: one pxsom_silhouette call -- its four launches -- on labels already sorted (HIP events over back-to-back
    calls on one stream), with the binary64 rate that the distance loop reaches beside the chip's vector peak: a pair
    costs 3 d + 2 operations (d differences, d fused multiply-adds counted as two, a square root and an addition
    counted as one each), and every pair is visited once per labeling;
  - call_us: som_device.silhouette_scores as the package calls it: the checks (one small read-back), the sort by label
    and the call;
  - sklearn_us: sklearn.metrics.silhouette_score for ONE k on the same rows on this host, only at the sizes of
    --sklearn-cases (it is N^2; nothing is extrapolated), with the device's score for that k beside it and
    sklearn_sweep_over_call = 9 x sklearn_us / call_us, the ratio for the nine k the reference would loop over.

Every case runs in a child process of its own under a time limit; the first case that fails or runs over ends the run.

    python scripts/silhouette_bench.py [--cases 20000 100000 200000] [--sklearn-cases 20000] [--reps 3] [--limit 400]
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

D, KS = 20, list(range(2, 11))
PEAK_F64_TFLOPS = 78.6          # MI355X vector binary64, data sheet


def _events_us(fn, reps, warm=1):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def voronoi_labels(x, k, rs):
    seeds = x[rs.choice(len(x), k, replace=False)]
    d2 = ((x[:, None, :] - seeds[None, :, :]) ** 2).sum(axis=2)
    return d2.argmin(axis=1).astype(np.int32)


def run_case(n, reps, with_sklearn):
    import torch
    from ark_analysis_amd import _capi, som_device
    dev = _capi.require_gpu()
    rs = np.random.RandomState(n)
    x = rs.poisson(rs.choice([0.3, 2.0, 6.0], size=(n, D))).astype(np.float64)
    labelings = np.stack([voronoi_labels(x, k, rs) for k in KS])
    x_d, lab_d = torch.from_numpy(x).to(dev), torch.from_numpy(labelings).to(dev)

    scores = som_device.silhouette_scores(x_d, lab_d, KS)
    call_us = _events_us(lambda: som_device.silhouette_scores(x_d, lab_d, KS), reps, warm=0)

    m, k = len(KS), max(KS)
    order = torch.argsort(lab_d, dim=1, stable=True).to(torch.int32).contiguous()
    counts = torch.empty((m, k), dtype=torch.int32, device=dev)
    sums = torch.empty((m, n, k), dtype=torch.float64, device=dev)
    samples = torch.empty((m, n), dtype=torch.float64, device=dev)
    out = torch.empty((m,), dtype=torch.float64, device=dev)
    lib, st = _capi.lib(), _capi.stream_ptr()

    def launch():
        _capi.check(lib.pxsom_silhouette(x_d.data_ptr(), n, D, lab_d.data_ptr(), order.data_ptr(), m, k, counts.data_ptr(),
                                         sums.data_ptr(), samples.data_ptr(), out.data_ptr(), st), "pxsom_silhouette")
    kernel_us = _events_us(launch, reps, warm=0)
    assert bool((out.view(torch.int64) == scores.view(torch.int64)).all()), "two calls, two answers"

    flop = float(m) * n * n * (3 * D + 2)
    rec = {"n": n, "d": D, "labelings": m, "kernel_us": round(kernel_us, 1), "call_us": round(call_us, 1),
           "pairs_per_us": round(float(m) * n * n / kernel_us, 1), "f64_tflops": round(flop / kernel_us * 1e-6, 2),
           "f64_peak_tflops": PEAK_F64_TFLOPS, "f64_of_peak": round(flop / kernel_us * 1e-6 / PEAK_F64_TFLOPS, 3),
           "scores": [round(float(v), 6) for v in scores.cpu().numpy()]}
    if with_sklearn:
        from sklearn.metrics import silhouette_score
        which = KS.index(5)
        t0 = time.perf_counter()
        want = silhouette_score(x, labelings[which], metric="euclidean")
        rec["sklearn_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        rec["sklearn_k"], rec["sklearn_score"] = KS[which], float(want)
        rec["score_gap"] = abs(float(scores[which]) - float(want))
        assert rec["score_gap"] <= 9 * (n + D) * 2.0 ** -53, "the device score is outside the derived bound of sklearn's"
        rec["sklearn_sweep_over_call"] = round(len(KS) * rec["sklearn_us"] / call_us, 1)
        rec["host_threads"] = os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"])
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", type=int, default=[20000, 100000, 200000])
    ap.add_argument("--sklearn-cases", nargs="*", type=int, default=[20000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds per case")
    ap.add_argument("--case", type=int, help=argparse.SUPPRESS)      # the child's one case
    ap.add_argument("--sklearn", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.reps, args.sklearn)
        return 0
    for n in args.cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(n), "--reps", str(args.reps)]
        if n in args.sklearn_cases:
            cmd.append("--sklearn")
        try:
            res = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print("case %d ran over %d s: stopping" % (n, args.limit), file=sys.stderr)
            return 1
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            print("case %d failed with status %d: stopping" % (n, res.returncode), file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
