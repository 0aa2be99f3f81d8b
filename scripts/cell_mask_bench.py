#!/usr/bin/env python
"""Times the cell cluster masks (pxsom_segmask) on int32 Voronoi-like segmentations of ~20 000 cells:

  - device time per FOV of one pxsom_segmask call (HIP events over back-to-back calls on one stream), erosion on / off,
    int16 output (cluster ids, dense LUT) and float64 output (per-cell values), with the algorithmic bytes (input +
    output) per second against 8 TB/s;
  - FOVs/s end to end of generate_and_save_cell_cluster_masks over a temporary directory of 20 FOVs, beside a host
    restatement (scipy.ndimage erosion + numpy lookup + the same TIFF reader / writer) timed in the same run.

    python scripts/cell_mask_bench.py [--sizes 2048 1024] [--fovs 20] [--reps 200]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def device_us(seg_t, erode, table, out_dtype, reps):
    import torch
    from ark_analysis_amd import som_device
    out = torch.empty(seg_t.shape, dtype=out_dtype, device=seg_t.device)
    kw = dict(erode=erode, connectivity=2, table=table, unassigned=0, out_dtype=out_dtype, out=out)
    for _ in range(10):
        som_device.segmentation_mask(seg_t, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        som_device.segmentation_mask(seg_t, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def host_mask(seg, keys, values, unassigned):
    """The host restatement: find_boundaries(connectivity 2, thick) by scipy.ndimage, zeroing, int32 cast, lookup."""
    import scipy.ndimage as ndi
    fp = ndi.generate_binary_structure(2, 2)
    edge = ndi.grey_dilation(seg, footprint=fp) != ndi.grey_erosion(seg, footprint=fp)
    lab = np.where(edge, 0, seg).astype(np.int32)
    idx = np.minimum(np.searchsorted(keys, lab), keys.size - 1)
    return np.where(keys[idx] == lab, values[idx], unassigned).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 1024])
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--fovs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-end-to-end", action="store_true")
    args = ap.parse_args()

    import pandas as pd
    import torch
    from ark_analysis_amd import _capi, image_io, som_device
    from ark_analysis_amd.utils import data_utils
    from tests import cell_mask_reference as cr
    dev = _capi.require_gpu()
    results = []
    for n in args.sizes:
        seg = cr.voronoi_labels(n, n, args.cells, seed=n)
        labels = np.unique(seg)
        rs = np.random.RandomState(n)
        keys = labels.astype(np.int32)
        ids = rs.randint(1, 30, size=keys.size)
        ids[keys == 0] = 0
        seg_t = torch.from_numpy(seg).to(dev)
        tab_i = som_device.segmask_table(keys, ids, dev)
        tab_f = som_device.segmask_table(keys, rs.rand(keys.size), dev, float_values=True)
        for erode in (None, "thick"):
            for out_dtype, tab in ((torch.int16, tab_i), (torch.float64, tab_f)):
                us = device_us(seg_t, erode, tab, out_dtype, args.reps)
                nbytes = seg.size * (4 + torch.empty(0, dtype=out_dtype).element_size())
                results.append({"size": n, "cells": int(labels.size - 1), "erode": erode or "none",
                                "out": str(out_dtype).replace("torch.", ""), "device_us": round(us, 2),
                                "GB_per_s": round(nbytes / us / 1e3, 1),
                                "frac_of_8TBps": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3)})
                print(json.dumps(results[-1]), flush=True)

        if args.no_end_to_end:
            continue
        # end to end over a directory of FOVs
        with tempfile.TemporaryDirectory() as td:
            seg_dir = os.path.join(td, "seg")
            os.makedirs(seg_dir)
            os.makedirs(os.path.join(td, "out"))
            fovs = ["fov%d" % i for i in range(args.fovs)]
            rows = []
            for f in fovs:
                image_io.write_image(os.path.join(seg_dir, f + "_whole_cell.tiff"), seg)
                rows.append(pd.DataFrame({"fov": f, "label": labels[labels > 0],
                                          "cell_meta_cluster": rs.randint(1, 30, size=labels.size - 1)}))
            table = pd.concat(rows, ignore_index=True)
            pd.DataFrame({"cell_meta_cluster": np.arange(1, 30)}).to_csv(os.path.join(td, "names.csv"), index=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data_utils.generate_and_save_cell_cluster_masks(fovs, os.path.join(td, "out"), seg_dir, table,
                                                            os.path.join(td, "names.csv"), sub_dir="cell_masks")
            t_dev = time.perf_counter() - t0

            cmd = data_utils.ClusterMaskData(table, "fov", "label", "cell_meta_cluster")
            t0 = time.perf_counter()
            for f in fovs:
                rows = cmd.fov_mapping(f)
                k, v = cr.table_from_mapping(dict(zip(rows["label"], rows["cluster_id"])))
                s = image_io.read_image(os.path.join(seg_dir, f + "_whole_cell.tiff"))
                data_utils.save_fov_mask(f, os.path.join(td, "out"), host_mask(s, k, v, int(cmd.unassigned_id)),
                                         sub_dir="host_masks")
            t_host = time.perf_counter() - t0
            for f in fovs[:2]:
                a = image_io.read_image(os.path.join(td, "out", "cell_masks", f + ".tiff"))
                b = image_io.read_image(os.path.join(td, "out", "host_masks", f + ".tiff"))
                assert np.array_equal(a, b), "device and host masks differ"
        results.append({"size": n, "fovs": args.fovs, "end_to_end_fovs_per_s": round(args.fovs / t_dev, 2),
                        "host_restatement_fovs_per_s": round(args.fovs / t_host, 2)})
        print(json.dumps(results[-1]), flush=True)


if __name__ == "__main__":
    main()
