#!/usr/bin/env python
"""Times the cell table (pxsom_cellquant) on Voronoi-like int32 segmentations of ~20 000 cells:

  - device time per FOV of one pxsom_cellquant call (HIP events over back-to-back calls on one stream; the key table
    is made once), total_intensity / center_weighting, with and without a nuclear image, against the algorithmic bytes
    (image once, labels twice) at 8 TB/s; one case with a few fragmented labels (bounding box >> pixel count);
  - FOVs/s end to end of generate_cell_table over a temporary directory of FOVs, beside a host restatement (the
    reference's per-cell numpy: coords, fancy-indexed sum, centroid mean, nucleus argmax) timed in the same run over
    the same TIFF reader.

    python scripts/cell_table_bench.py [--configs 2048:40 1024:22] [--fovs 4] [--reps 50]
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


def device_us(seg_t, img_t, keys, mode, nuc_t, nuc_keys, reps):
    import torch
    from ark_analysis_amd import som_device
    kw = dict(keys=keys, mode=mode, nuc=nuc_t, nuc_keys=nuc_keys)
    for _ in range(3):
        som_device.cell_quantify(seg_t, img_t, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        som_device.cell_quantify(seg_t, img_t, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def host_frames(fov, seg, nuc, img, channels):
    """The host restatement of one FOV (total_intensity with nuclear counts)."""
    from tests import cell_table_reference as ctr
    return ctr.cell_frames(fov, seg, img, channels, "total_intensity", 0, nuc=nuc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["2048:40", "1024:22"])
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--fovs", type=int, default=4)
    ap.add_argument("--host-fovs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-end-to-end", action="store_true")
    args = ap.parse_args()

    import pandas as pd
    import torch
    from ark_analysis_amd import _capi, image_io, som_device
    from ark_analysis_amd.segmentation import marker_quantification as mq
    from tests import cell_table_reference as ctr
    dev = _capi.require_gpu()
    for cfg in args.configs:
        n, c = (int(v) for v in cfg.split(":"))
        rs = np.random.RandomState(n + c)
        seg = ctr.voronoi_labels(n, n, args.cells, seed=n)
        nuc = np.where(seg % 4 != 0, seg, 0).astype(np.int32)
        img = (rs.gamma(0.7, 5.0, size=(n, n, c)) * (rs.rand(n, n, c) < 0.8)).astype(np.float32)
        seg_t, nuc_t, img_t = (torch.from_numpy(a).to(dev) for a in (seg, nuc, img))
        keys, nuc_keys = som_device.label_keys(seg_t), som_device.label_keys(nuc_t)
        nbytes = img.nbytes + 2 * seg.nbytes
        cases = [("total_intensity", False, seg_t, keys), ("total_intensity", True, seg_t, keys),
                 ("center_weighting", False, seg_t, keys)]
        frag = ctr.fragment(seg, rs.choice(keys.cpu().numpy(), 8, replace=False), pieces=16, seed=n)
        frag_t = torch.from_numpy(frag).to(dev)
        cases.append(("total_intensity:fragmented", False, frag_t, som_device.label_keys(frag_t)))
        for mode, with_nuc, s_t, k_t in cases:
            us = device_us(s_t, img_t, k_t, mode.split(":")[0], nuc_t if with_nuc else None,
                           nuc_keys if with_nuc else None, args.reps)
            nb = nbytes + (2 * nuc.nbytes if with_nuc else 0)
            rec = {"size": n, "channels": c, "cells": int(k_t.numel()), "mode": mode, "nuclear": with_nuc,
                   "device_us": round(us, 1), "GB_per_s": round(nb / us / 1e3, 1),
                   "frac_of_8TBps": round(nb / (us * 1e-6) / HBM_BYTES_PER_S, 3)}
            print(json.dumps(rec), flush=True)
        t0 = time.perf_counter()
        for _ in range(5):
            som_device.label_keys(seg_t)
        torch.cuda.synchronize()
        print(json.dumps({"size": n, "label_keys_us": round((time.perf_counter() - t0) / 5 * 1e6, 1)}), flush=True)

        if args.no_end_to_end:
            continue
        with tempfile.TemporaryDirectory() as td:
            tiff_dir, seg_dir = os.path.join(td, "tiffs"), os.path.join(td, "seg")
            channels = ["chan%d" % j for j in range(c)]
            fovs = ["fov%d" % i for i in range(args.fovs)]
            os.makedirs(seg_dir)
            for f in fovs:
                os.makedirs(os.path.join(tiff_dir, f, "TIFs"))
                for j, ch in enumerate(channels):
                    image_io.write_image(os.path.join(tiff_dir, f, "TIFs", ch + ".tiff"), np.ascontiguousarray(img[:, :, j]))
                image_io.write_image(os.path.join(seg_dir, f + "_whole_cell.tiff"), seg)
                image_io.write_image(os.path.join(seg_dir, f + "_nuclear.tiff"), nuc)
            mq.generate_cell_table(seg_dir, tiff_dir, fovs=fovs[:1], fast_extraction=True, nuclear_counts=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            norm, _ = mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=True, nuclear_counts=True)
            t_dev = time.perf_counter() - t0

            t0 = time.perf_counter()
            host = []
            for f in fovs[:args.host_fovs]:
                chans = image_io.channel_names(tiff_dir, f, "TIFs")
                im = image_io.read_channels(tiff_dir, f, chans, "TIFs")
                s = image_io.read_image(os.path.join(seg_dir, f + "_whole_cell.tiff"))
                nu = image_io.read_image(os.path.join(seg_dir, f + "_nuclear.tiff"))
                host.append(host_frames(f, s, nu, np.ascontiguousarray(im), chans)[0])
            t_host = time.perf_counter() - t0
            pd.testing.assert_frame_equal(norm[norm["fov"] == fovs[0]], host[0], check_exact=True)
        print(json.dumps({"size": n, "channels": c, "fovs": args.fovs,
                          "end_to_end_fovs_per_s": round(args.fovs / t_dev, 2),
                          "host_restatement_fovs_per_s": round(args.host_fovs / t_host, 3)}), flush=True)


if __name__ == "__main__":
    main()
