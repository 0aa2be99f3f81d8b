#!/usr/bin/env python
"""Times ``_create_object_mask`` (K16) on synthetic 2048 x 2048 images against the scipy statement of
tests/object_mask_reference.py on the same host:

    A   sigma = 2,  thresh "auto", hole_size "auto", float32 blobs   (the ez_segmenter notebook's shape)
    B   sigma = 10, thresh None,   hole_size 1000, max area = the image   (create_cell_mask's shape, on a 0 / 1 image of
        scattered discs: the blur reaches 40 pixels, so the discs' neighbourhoods are the objects)

Prints one JSON line: per configuration the device chain as called from the host image (upload, kernels, download), the
chain alone on a resident image under HIP events, and the statement's wall time; the masks are compared exactly.
Per-stage device times come from a profiler run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/object_mask_bench.py --reps 5 --no-host
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def image(size, seed=0):
    import scipy.ndimage as ndi
    rs = np.random.RandomState(seed)
    spikes = (rs.rand(size, size) < 0.002) * rs.gamma(2.0, 200.0, size=(size, size))
    img = ndi.gaussian_filter(spikes, 4.0) + (rs.rand(size, size) < 0.05) * rs.gamma(1.0, 0.2, size=(size, size))
    img[img < 0.05] = 0.0
    return img.astype(np.float32)


def cell_image(size, seed=1):
    """A 0 / 1 int32 image of scattered discs, as np.isin(seg, labels) of a few cell types gives."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:size, :size]
    img = np.zeros((size, size), dtype=np.int32)
    for _ in range(max(4, size * size // 50000)):
        cy, cx, r = rs.randint(0, size), rs.randint(0, size), rs.randint(15, 61)
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, size), max(cx - r, 0), min(cx + r + 1, size)
        img[y0:y1, x0:x1] |= ((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2 <= r * r).astype(np.int32)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy statement (profiler runs)")
    args = ap.parse_args()

    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.segmentation.ez_seg import ez_object_segmentation as ez
    from tests import object_mask_reference as omr
    dev = _capi.require_gpu()
    configs = {"A_sigma2_auto_auto": dict(img=image(args.size), sigma=2, thresh="auto", hole_size="auto", max_area=100000),
               "B_sigma10_none_1000": dict(img=cell_image(args.size), sigma=10, thresh=None, hole_size=1000,
                                           max_area=args.size * args.size)}
    result = {"size": args.size, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name, kw in configs.items():
        img, max_area = kw["img"], kw["max_area"]
        block = ez.get_block_size("local_thresh", 400, args.size) if kw["thresh"] == "auto" else None
        hole = ez.get_block_size("small_holes", 400, args.size) if kw["hole_size"] == "auto" else kw["hole_size"]
        got = ez._create_object_mask(img, "blob", kw["sigma"], kw["thresh"], kw["hole_size"], 400, 10, max_area)   # warm-up
        walls = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ez._create_object_mask(img, "blob", kw["sigma"], kw["thresh"], kw["hole_size"], 400, 10, max_area)
            walls.append(time.perf_counter() - t0)
        t = torch.from_numpy(img).to(dev)
        t = t if t.dtype == torch.float32 else t.to(torch.float64)      # (the mirror's cast, outside the timed chain)
        events = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            som_device.object_mask(t, kw["sigma"], kw["thresh"], hole, 10, max_area, block)
            e1.record()
            torch.cuda.synchronize()
            events.append(e0.elapsed_time(e1))
        row = {"mirror_ms_median": 1e3 * float(np.median(walls)), "mirror_ms_min": 1e3 * min(walls),
               "chain_ms_median": float(np.median(events)), "chain_ms_min": min(events),
               "objects": int(len(np.unique(got)) - 1)}
        if not args.no_host:
            t0 = time.perf_counter()
            want = omr.create_object_mask(img, kw["sigma"], kw["thresh"], kw["hole_size"], 400, 10, max_area)
            row["scipy_ms"] = 1e3 * (time.perf_counter() - t0)
            row["equal"] = bool(np.array_equal(got, want))
        result[name] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
