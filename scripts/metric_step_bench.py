"""Timing of labels + batch statistics under FlowSOM's distf 1 / 3 / 4 (DESIGN.md "K6m").

Per (shape, metric) one JSON line: the one-pass entry pxsom_assign_sums_metric of this build against the pair it replaces,
pxsom_assign_metric followed by pxsom_cluster_sums, taken from the library --pair-lib names (build the commit to compare with
and pass its libpxsom.so; default: this build's own, marked "pair_build": "same").  The two are timed alternately in one
process (HIP events around each call, after a warm-up of both; median and the spread min..max of --reps), and their labels and
statistics are compared on the timed inputs.  Then, per metric, the time of one 22-step pass of the two-phase schedule
(HipKernels(metric) on --pass-rows x 22 binary32 rows, 10 x 10 map; host clock around steps + finish, ending in a synchronise).
In between: pxsom_assign_metric alone on staged binary64 rows, this build against --pair-lib (its kernels share the search).

    python scripts/metric_step_bench.py [--reps 20] [--pair-lib /path/to/other/libpxsom.so] [--pass-rows 10485760]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ark_analysis_amd import _capi, distributed, flowsom, som_device  # noqa: E402

# (rows, channels, nodes, storage type)
# (the last one is past the LDS limit of the workgroup table: its rows are added to the statistics in global memory)
SHAPES = [(1_048_576, 22, 100, torch.float32), (262_144, 40, 400, torch.float16), (65_536, 64, 1024, torch.float32)]
LABELS_SHAPE = (262_144, 40, 400, torch.float64)     # pxsom_assign_metric alone, staged binary64 rows: this build against --pair-lib
NAMES = {1: "manhattan", 3: "chebyshev", 4: "cosine"}


def _pair_library(path):
    lib = ctypes.CDLL(path)
    for name in ("pxsom_assign_metric_workspace_bytes", "pxsom_assign_metric", "pxsom_cluster_sums"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _capi.SYMBOLS[name]
    return lib


def _timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _summary(times):
    times = sorted(times)
    return {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4)}


def step_lines(args, dev):
    pair = _pair_library(args.pair_lib) if args.pair_lib else _capi.lib()
    for n, c, k, dtype in SHAPES:
        g = torch.Generator(device=dev)
        g.manual_seed(n + c)
        # small integers: the statistics are exact in any order, so the two builds must agree to the bit
        xd = torch.randint(0, 16, (n, c), generator=g, device=dev).to(dtype)
        wd = (xd[torch.randperm(n, generator=g, device=dev)[:k]].double() + torch.rand((k, c), generator=g, device=dev,
                                                                                       dtype=torch.float64)).contiguous()
        dt, st = _capi.dtype_code(xd), _capi.stream_ptr()
        for metric in (1, 3, 4):
            ws = som_device.MetricStepWorkspace(c, k, dev, metric)
            labels = torch.empty(n, dtype=torch.int32, device=dev)
            stats = torch.zeros(k * (c + 1), dtype=torch.float64, device=dev)
            pws = torch.empty(pair.pxsom_assign_metric_workspace_bytes(n, c, k, metric), dtype=torch.uint8, device=dev)
            plabels = torch.empty(n, dtype=torch.int32, device=dev)
            psums = torch.zeros((k, c), dtype=torch.float64, device=dev)
            pcounts = torch.zeros(k, dtype=torch.int64, device=dev)

            mine = _capi.lib()

            # (both sides through bare ctypes calls: a wrapper's host work between the two events would count against its side)
            def entry(labels_ptr):
                rc = mine.pxsom_assign_sums_metric(xd.data_ptr(), n, c, c, dt, wd.data_ptr(), k, 1, 0, 1, labels_ptr, stats.data_ptr(), 0.0,
                                                   ws.buf.data_ptr(), ws.bytes, metric, st)
                if rc:
                    raise RuntimeError("pxsom_assign_sums_metric: status %d" % rc)

            def fused():
                entry(labels.data_ptr())

            def pair_calls():
                rc = pair.pxsom_assign_metric(xd.data_ptr(), n, c, c, dt, wd.data_ptr(), k, plabels.data_ptr(), None, pws.data_ptr(),
                                              pws.numel(), metric, st)
                rc = rc or pair.pxsom_cluster_sums(xd.data_ptr(), n, c, c, dt, plabels.data_ptr(), k, psums.data_ptr(),
                                                   pcounts.data_ptr(), st)
                if rc:
                    raise RuntimeError("pair library: status %d" % rc)

            for _ in range(3):
                fused()
                pair_calls()
            torch.cuda.synchronize()
            stats.zero_(), psums.zero_(), pcounts.zero_()
            tf, tp = [], []
            for _ in range(args.reps):
                tf.append(_timed(fused))
                tp.append(_timed(pair_calls))
            same = bool(torch.equal(labels, plabels) and torch.equal(stats[:k * c].view(k, c), psums)
                        and torch.equal(stats[k * c:], pcounts.double()))
            # without a labels vector the entry is always the one pass (with one, the shapes measured slower take two launches)
            for _ in range(3):
                entry(None)
            torch.cuda.synchronize()
            one_pass = _summary([_timed(lambda: entry(None)) for _ in range(args.reps)])
            f, p = _summary(tf), _summary(tp)
            print(json.dumps({"shape": [n, c, k], "dtype": str(dtype).replace("torch.", ""), "metric": NAMES[metric], "distf": metric,
                              "fused": f, "one_pass_no_labels": one_pass, "pair": p, "fused_over_pair": round(f["median_ms"] / p["median_ms"], 3),
                              "pair_build": args.pair_lib or "same", "same_labels_and_statistics": same, "reps": args.reps}),
                  flush=True)
        del xd, wd
        torch.cuda.empty_cache()


def labels_lines(args, dev):
    n, c, k, dtype = LABELS_SHAPE
    mine, pair = _capi.lib(), (_pair_library(args.pair_lib) if args.pair_lib else _capi.lib())
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    xd = torch.rand((n, c), generator=g, device=dev, dtype=dtype)
    wd = xd[torch.randperm(n, generator=g, device=dev)[:k]].contiguous()
    dt, st = _capi.dtype_code(xd), _capi.stream_ptr()
    for metric in (1, 3, 4):
        ws = torch.empty(mine.pxsom_assign_metric_workspace_bytes(n, c, k, metric), dtype=torch.uint8, device=dev)
        out = {lib: torch.empty(n, dtype=torch.int32, device=dev) for lib in (mine, pair)}

        def call(lib):
            rc = lib.pxsom_assign_metric(xd.data_ptr(), n, c, c, dt, wd.data_ptr(), k, out[lib].data_ptr(), None, ws.data_ptr(), ws.numel(),
                                         metric, st)
            if rc:
                raise RuntimeError("pxsom_assign_metric: status %d" % rc)

        for _ in range(3):
            call(mine), call(pair)
        torch.cuda.synchronize()
        tm, tp = [], []
        for _ in range(args.reps):
            tm.append(_timed(lambda: call(mine)))
            tp.append(_timed(lambda: call(pair)))
        a, b = _summary(tm), _summary(tp)
        print(json.dumps({"entry": "pxsom_assign_metric", "shape": [n, c, k], "dtype": "float64", "metric": NAMES[metric], "distf": metric,
                          "this_build": a, "pair_build_time": b, "this_over_pair": round(a["median_ms"] / b["median_ms"], 3),
                          "pair_build": args.pair_lib or "same", "same_labels": bool(torch.equal(out[mine], out[pair])), "reps": args.reps}),
              flush=True)


def pass_lines(args, dev):
    n, c = args.pass_rows, 22
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    xd = torch.rand((n, c), generator=g, device=dev, dtype=torch.float32)
    w0 = xd[torch.randperm(n, generator=g, device=dev)[:100]].double().contiguous()
    rr = flowsom.default_radius_range(10, 10)
    for metric in (2, 1, 3, 4):
        trainer = distributed.BatchSOMTrainer(10, 10, c, dev, radius_range=rr, kernels=distributed.HipKernels(metric=metric))
        out = torch.empty_like(w0)
        trainer.train(xd, w0, out=out)      # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(args.pass_reps):
            t0 = time.perf_counter()
            trainer.train(xd, w0, out=out)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"pass": "two-phase, %d steps" % trainer.batch_steps, "rows": n, "channels": c, "map": "10x10", "dtype": "float32",
                          "metric": NAMES.get(metric, "euclidean"), "distf": metric, **_summary(times), "reps": args.pass_reps}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--pass-rows", type=int, default=10_485_760)
    ap.add_argument("--pair-lib", default=None)
    args = ap.parse_args()
    dev = _capi.require_gpu()
    step_lines(args, dev)
    labels_lines(args, dev)
    pass_lines(args, dev)


if __name__ == "__main__":
    main()
