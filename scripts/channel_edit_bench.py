#!/usr/bin/env python
"""Times the channel edits (pxsom_gaussian_blur_plane / smooth_channels):

  - device time per plane of one pxsom_gaussian_blur_plane call (HIP events over back-to-back calls on one stream) for
    uint16 and float32 planes at sigma 2 and 6, with the bytes the two passes must move (each pass reads the plane and
    writes it once: 4 x plane bytes) and the fraction of 8 TB/s that implies;
  - FOVs/s end to end of smooth_channels over a synthetic cohort (--fovs FOVs x --channels chosen channels of --size^2
    uint16), beside a host restatement (the same TIFF reader and writer around scipy.ndimage.gaussian_filter) timed in
    the same run.

    python scripts/channel_edit_bench.py [--size 2048] [--fovs 8] [--channels 4] [--reps 100]
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


def device_us(t, sigma, reps):
    import torch
    from ark_analysis_amd import som_device
    out, tmp = torch.empty_like(t), torch.empty_like(t)
    for _ in range(5):
        som_device.gaussian_blur_plane(t, sigma, out=out, tmp=tmp)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        som_device.gaussian_blur_plane(t, sigma, out=out, tmp=tmp)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def host_smooth(fovs, tiff_dir, channels, sigma):
    """The host restatement: the same reader and writer, scipy's blur in between, one plane at a time."""
    import scipy.ndimage as ndimage
    from ark_analysis_amd import image_io
    for fov in fovs:
        for chan in channels:
            img = image_io.read_channel(tiff_dir, fov, chan, "TIFs")
            image_io.write_image(os.path.join(tiff_dir, fov, "TIFs", chan + "_smoothed.tiff"),
                                 ndimage.gaussian_filter(img, sigma))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--fovs", type=int, default=8)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sigma", type=int, default=6)
    args = ap.parse_args()
    import torch
    from ark_analysis_amd import image_io
    from ark_analysis_amd.phenotyping import pixel_cluster_utils
    rs = np.random.RandomState(0)
    n = args.size
    results = {"size": n, "kernel": []}
    for dtype in (np.uint16, np.float32):
        plane = (rs.gamma(0.5, 300.0, size=(n, n))).astype(dtype)
        t = torch.from_numpy(plane).cuda()
        for sigma in (2, 6):
            us = device_us(t, sigma, args.reps)
            moved = 4 * plane.nbytes
            results["kernel"].append({"dtype": np.dtype(dtype).name, "sigma": sigma, "us": round(us, 1),
                                      "bytes": moved, "hbm_fraction": round(moved / (us * 1e-6) / HBM_BYTES_PER_S, 4)})
    with tempfile.TemporaryDirectory() as td:
        fovs = ["fov%d" % i for i in range(args.fovs)]
        chans = ["chan%d" % j for j in range(args.channels)]
        for fov in fovs:
            os.makedirs(os.path.join(td, fov, "TIFs"))
            for ch in chans:
                image_io.write_image(os.path.join(td, fov, "TIFs", ch + ".tiff"),
                                     rs.gamma(0.5, 300.0, size=(n, n)).astype(np.uint16))
        pixel_cluster_utils.smooth_channels(fovs[:1], td, "TIFs", chans, args.sigma)      # warm-up (library, context)
        t0 = time.perf_counter()
        pixel_cluster_utils.smooth_channels(fovs, td, "TIFs", chans, args.sigma)
        dev_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        host_smooth(fovs, td, chans, args.sigma)
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        for fov in fovs:                                  # the file I/O alone: read and write every plane once
            for ch in chans:
                img = image_io.read_channel(td, fov, ch, "TIFs")
                image_io.write_image(os.path.join(td, fov, "TIFs", ch + "_io.tiff"), img)
        io_s = time.perf_counter() - t0
    results["end_to_end"] = {"fovs": args.fovs, "channels": args.channels, "sigma": args.sigma, "dtype": "uint16",
                             "device_fovs_per_s": round(args.fovs / dev_s, 2), "host_fovs_per_s": round(args.fovs / host_s, 2),
                             "io_only_fovs_per_s": round(args.fovs / io_s, 2)}
    print(json.dumps(results))


if __name__ == "__main__":
    main()
