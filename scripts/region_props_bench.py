#!/usr/bin/env python
"""Times the morphology kernels (pxsom_region_shape, pxsom_region_hull) on the Voronoi-like int32
segmentation scripts/cell_table_bench.py uses (2048^2, ~18 000 cells), beside one pxsom_cellquant call (K12,
total_intensity) over the same segmentation: µs per call from HIP events over back-to-back calls on one stream, the key
table made once.

    python scripts/region_props_bench.py [--size 2048] [--channels 40] [--cells 20000] [--reps 50]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--channels", type=int, default=40)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    import torch
    from ark_analysis_amd import _capi, som_device
    from tests import cell_table_reference as ctr
    dev = _capi.require_gpu()
    lib = _capi.lib()
    n = args.size
    seg = ctr.voronoi_labels(n, n, args.cells, seed=n)
    seg_t = torch.from_numpy(seg).to(dev)
    keys = som_device.label_keys(seg_t)
    k = keys.numel()
    kmin, kmax = int(keys[0]), int(keys[-1])
    got = som_device.region_props(seg_t, keys=keys)
    left_out = int(got["left_out"].sum())
    wsb = lib.pxsom_region_shape_workspace_bytes(k, kmin, kmax, 0)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    code = som_device.SEG_DTYPES[seg_t.dtype]
    st = _capi.stream_ptr()

    def shape(stats):
        p = [got[x].data_ptr() if stats else None for x in ("count", "sums", "bbox")]
        _capi.check(lib.pxsom_region_shape(seg_t.data_ptr(), code, n, n, n, keys.data_ptr(), k, kmin, kmax,
                                           got["shape"].data_ptr(), p[0], p[1], p[2], ws.data_ptr(), wsb, 0, st), "shape")

    def hull():
        _capi.check(lib.pxsom_region_hull(seg_t.data_ptr(), code, n, n, n, keys.data_ptr(), k, got["count"].data_ptr(),
                                          got["bbox"].data_ptr(), 10.0, 60.0, 150.0, got["hull"].data_ptr(),
                                          got["left_out"].data_ptr(), st), "hull")
    rec = {"size": n, "cells": k, "left_out": left_out,
           "region_shape_us": round(timed(lambda: shape(False), args.reps), 1),
           "region_shape_with_tables_us": round(timed(lambda: shape(True), args.reps), 1),
           "region_hull_us": round(timed(hull, args.reps), 1),
           "region_props_call_us": round(timed(lambda: som_device.region_props(seg_t, keys=keys), args.reps), 1)}
    rs = np.random.RandomState(n)
    img_t = torch.from_numpy((rs.gamma(0.7, 5.0, size=(n, n, args.channels))).astype(np.float32)).to(dev)
    rec["channels"] = args.channels
    rec["cellquant_total_intensity_us"] = round(timed(lambda: som_device.cell_quantify(seg_t, img_t, keys=keys),
                                                      args.reps), 1)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
