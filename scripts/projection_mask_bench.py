#!/usr/bin/env python
"""Times the "projection" object masks (K22) on a synthetic 2048 x 2048 plane of discs and lines against the numpy statement
of tests/projection_mask_reference.py on the same host: sigma = 1, thresh None, hole_size "auto", the reference's four
scales (the ez_segmenter notebook's microglia-projections cell).

Prints one JSON line: som_device.ridge_sign alone on a resident uint8 plane under HIP events, the device chain on a resident
image with and without the ridge stage under HIP events, _create_object_mask from a host image (upload, kernels, download),
and the statement's wall time; the masks are compared exactly.  Per-kernel device times come from a profiler run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/projection_mask_bench.py --reps 5 --no-host

``--by-scale`` instead times som_device.ridge_sign alone per scale list (one scale of radius 1, 4, 8, 12, 16; four and eight
scales of radius 1; the reference's four), which separates what a scale costs whatever its radius from what the taps add.
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
    """Discs (somata) with thin straight arms, and loose segments, as float32 intensities on exact zeros."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:size, :size]
    plane = np.zeros((size, size), dtype=bool)

    def window(cy, cx, r):
        return slice(max(cy - r, 0), min(cy + r + 1, size)), slice(max(cx - r, 0), min(cx + r + 1, size))

    for _ in range(max(4, size * size // 20000)):
        cy, cx, r = rs.randint(0, size), rs.randint(0, size), rs.randint(4, 13)
        win = window(cy, cx, r)
        plane[win] |= (yy[win] - cy) ** 2 + (xx[win] - cx) ** 2 <= r * r
        for _ in range(rs.randint(2, 6)):
            ang, length, half = rs.uniform(0, 2 * np.pi), rs.randint(15, 60), rs.randint(1, 4) / 2.0
            win = window(cy, cx, length)
            dy, dx = yy[win] - cy, xx[win] - cx
            along = dy * np.sin(ang) + dx * np.cos(ang)
            plane[win] |= (np.abs(dy * np.cos(ang) - dx * np.sin(ang)) <= half) & (along >= 0) & (along <= length)
    return (plane * rs.gamma(4.0, 10.0, size=plane.shape)).astype(np.float32)


def events_ms(reps, call):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"median": float(np.median(out)), "min": min(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy statement (profiler runs)")
    ap.add_argument("--by-scale", action="store_true", help="time ridge_sign alone per scale list and print that instead")
    args = ap.parse_args()

    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.segmentation.ez_seg import ez_object_segmentation as ez
    from tests import projection_mask_reference as pmr
    dev = _capi.require_gpu()
    ez.PROJECTION_FILTER = "meijering"
    img = image(args.size)
    if args.by_scale:
        fg = (torch.from_numpy(img).to(dev) > 0).to(torch.uint8)
        out = torch.empty_like(fg)
        result = {"size": args.size, "reps": args.reps, "device": torch.cuda.get_device_name(0), "ridge_sign_ms_median": {}}
        for sigmas in ([0.25], [1], [2], [3], [4], [0.25] * 4, [0.25] * 8, [1, 2, 3, 4]):
            som_device.ridge_sign(fg, sigmas, pmr.ALPHA, out=out)      # warm-up
            timed = events_ms(args.reps, lambda: som_device.ridge_sign(fg, sigmas, pmr.ALPHA, out=out))
            result["ridge_sign_ms_median"][" ".join("%g" % s for s in sigmas)] = timed["median"]
        print(json.dumps(result))
        return
    hole = ez.get_block_size("small_holes", 400, args.size)
    ridge = (pmr.SIGMAS, pmr.ALPHA)
    call = (1, None, "auto", 400, 10, 100000)

    got = ez._create_object_mask(img, "projection", *call)      # warm-up
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        ez._create_object_mask(img, "projection", *call)
        walls.append(time.perf_counter() - t0)
    t = torch.from_numpy(img).to(dev)
    fg = (t > 0).to(torch.uint8)
    out = torch.empty_like(fg)
    som_device.ridge_sign(fg, *ridge, out=out)
    result = {"size": args.size, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "foreground": float(fg.float().mean().item()), "objects": int(len(np.unique(got)) - 1),
              "ridge_sign_ms": events_ms(args.reps, lambda: som_device.ridge_sign(fg, *ridge, out=out)),
              "chain_ms": events_ms(args.reps, lambda: som_device.object_mask(t, 1, None, hole, 10, 100000, ridge=ridge)),
              "chain_without_ridge_ms": events_ms(args.reps, lambda: som_device.object_mask(t, 1, None, hole, 10, 100000)),
              "mirror_ms": {"median": 1e3 * float(np.median(walls)), "min": 1e3 * min(walls)}}
    if not args.no_host:
        plane = fg.cpu().numpy()
        t0 = time.perf_counter()
        want_ridge = pmr.ridge_sign(plane)
        result["numpy_ridge_ms"] = 1e3 * (time.perf_counter() - t0)
        result["ridge_equal"] = bool(np.array_equal(out.cpu().numpy(), want_ridge))
        t0 = time.perf_counter()
        want = pmr.create_projection_mask(img, *call)
        result["numpy_chain_ms"] = 1e3 * (time.perf_counter() - t0)
        result["equal"] = bool(np.array_equal(got, want))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
