"""Timing of the BMU labels for FlowSOM's distances (distf 1, 3, 4), next to Euclidean on the same data.

One JSON line per (shape, metric): labels in ms (HIP events around the BMU kernel, median of --reps), the rows evaluated
in binary64 (every row: the metric kernels have no screen), Euclidean's time and listed rows on the same data, and the
binary64 VALU issue bound of the metric's inner loop (2 instructions per (row, node, channel) term, 4.7 clocks per
wave-instruction per SIMD, 1024 SIMDs at 2.4 GHz -- the issue rates of profiles/r05/valu_issue_rates.txt).

    python scripts/metric_bench.py [--reps 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ark_analysis_amd import _capi, som_device  # noqa: E402

SHAPES = [(10_485_760, 22, 100), (1_000_000, 100, 100)]
NAMES = {1: "manhattan", 2: "euclidean", 3: "chebyshev", 4: "cosine"}


def issue_bound_ms(n, c, k, simds=1024, clk_ghz=2.4, clk_per_instr=4.7, instr_per_term=2):
    wave_instr = n * k * c * instr_per_term / 64.0
    return wave_instr / simds * clk_per_instr / (clk_ghz * 1e6)


def time_labels(xd, wd, metric, reps):
    ws = som_device.AssignWorkspace(xd.shape[0], xd.shape[1], wd.shape[0], xd.device, metric)
    labels = torch.empty(xd.shape[0], dtype=torch.int32, device=xd.device)
    som_device.assign(xd, wd, labels=labels, workspace=ws, metric=metric)   # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        som_device.assign(xd, wd, labels=labels, workspace=ws, metric=metric)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], som_device.last_exact_rows(ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = _capi.require_gpu()
    for n, c, k in SHAPES:
        g = torch.Generator(device=dev)
        g.manual_seed(n + c)
        xd = torch.rand((n, c), generator=g, device=dev, dtype=torch.float32)
        idx = torch.randperm(n, generator=g, device=dev)[:k]
        wd = xd[idx].double().contiguous()
        eu_ms, eu_rows = time_labels(xd, wd, 2, args.reps)
        for metric in (1, 3, 4):
            ms, rows = time_labels(xd, wd, metric, args.reps)
            bound = issue_bound_ms(n, c, k)
            print(json.dumps({"shape": [n, c, k], "dtype": "f32", "metric": NAMES[metric], "distf": metric,
                              "labels_ms": round(ms, 4), "rows_exact": rows, "issue_bound_ms": round(bound, 4),
                              "issue_bound_note": "estimate: 2 binary64 VALU instructions per term at 4.7 clk",
                              "frac_of_bound": round(bound / ms, 3), "euclidean_ms": round(eu_ms, 4),
                              "euclidean_rows_exact": eu_rows}), flush=True)
        del xd, wd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
