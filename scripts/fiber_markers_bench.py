#!/usr/bin/env python
"""Times the K25 entries -- from the ridge map to the watershed's inputs -- on a synthetic plane of bars (about 10 %
foreground; default 2048 x 2048) against the scipy / numpy statement of tests/fiber_markers_reference.py on the same host.

Prints a table: every entry alone on resident planes and the chain on a resident ridge plane (HIP events, median and
minimum of ``--reps`` after a warm-up call), fiber_watershed_inputs from a host plane (host clock around the call, which
ends in the downloads), the statement's wall time (one run, the only baseline: the capability is new), whether every
result equals the statement's, and the bounds each kernel is judged against: the HBM bytes per pixel of each stage over
the MI355X's 8 TB/s, and for the second pass of the distance transform the sum of its search windows on this plane.  Also
the distance transform's worst case, a plane with a single background pixel, where every pixel searches its whole row.
Per-kernel device times come from a profiler run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/fiber_markers_bench.py --reps 5 --no-host
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
CUTOFF, SOBEL_BLUR = 0.1, 1


def bar_plane(size, target=0.10, seed=0):
    """Straight bars of width 2 .. 7 across the plane until `target` of it is foreground."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:size, :size].astype(np.float32)
    fg = np.zeros((size, size), bool)
    while fg.mean() < target:
        theta, cy, cx, width = rs.uniform(0, np.pi), rs.uniform(0, size), rs.uniform(0, size), rs.randint(2, 8)
        fg |= np.abs((yy - cy) * np.cos(theta) - (xx - cx) * np.sin(theta)) <= width / 2.0
    return fg.astype(np.uint8)


def events_ms(reps, call):
    import torch
    call()                                                      # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy / numpy statement (profiler runs)")
    args = ap.parse_args()

    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    from tests import fiber_markers_reference as fmr
    dev = _capi.require_gpu()
    n = args.size
    fg_host = bar_plane(n)
    ridges_host = fmr.ridge_plane(fg_host, CUTOFF)
    pixels = n * n

    ridges = torch.from_numpy(ridges_host).to(dev)
    fg = som_device.plane_greater(ridges, CUTOFF)
    edt = som_device.distance_transform_edt(fg)
    sq = som_device.distance_transform_edt(fg, squared=True)
    dist = som_device.gaussian_blur_plane_mode(edt, 1, "reflect")
    lo, hi = som_device.plane_minmax(dist)
    counts, edges = som_device.plane_histogram(dist, 256, (lo, hi))
    t0, t1 = fs.threshold_multiotsu_from_histogram(counts.cpu().numpy(), edges)
    smooth = som_device.gaussian_blur_plane_mode(dist, SOBEL_BLUR, "reflect")
    out_fg, out_edt, out_i32, out_f64 = torch.empty_like(fg), torch.empty_like(edt), torch.empty_like(sq), torch.empty_like(edt)
    noise = torch.from_numpy(np.random.RandomState(1).random_sample((n, n))).to(dev)      # every bin equally likely
    single = torch.ones_like(fg)
    single[n // 3, n // 3] = 0

    # bytes per pixel that must cross HBM, reads + writes
    rows = [
        ("plane_greater", lambda: som_device.plane_greater(ridges, CUTOFF, out=out_fg), 8 + 1),
        ("distance_transform_edt (float64)", lambda: som_device.distance_transform_edt(fg, out=out_edt, check=False), 1 + 4 + 4 + 8),
        ("distance_transform_edt (squared)", lambda: som_device.distance_transform_edt(fg, out=out_i32, squared=True, check=False),
         1 + 4 + 4 + 4),
        ("gaussian_blur_plane_mode sigma 1", lambda: som_device.gaussian_blur_plane_mode(edt, 1, "reflect", out=out_f64), 4 * 8),
        ("plane_minmax (with its read-back)", lambda: som_device.plane_minmax(dist), 8),
        ("plane_histogram (range given)", lambda: som_device.plane_histogram(dist, 256, (lo, hi)), 8),
        ("plane_histogram of uniform noise (range given)", lambda: som_device.plane_histogram(noise, 256, (0.0, 1.0)), 8),
        ("class_markers", lambda: som_device.class_markers(dist, t0, t1, out=out_i32), 8 + 4),
        ("sobel_magnitude (float64)", lambda: som_device.sobel_magnitude(smooth, out=out_f64), 8 + 8),
        ("sobel_magnitude (int32)", lambda: som_device.sobel_magnitude(smooth, out=out_i32, as_int32=True), 8 + 4),
        ("watershed_inputs, resident plane", lambda: som_device.watershed_inputs(ridges, CUTOFF, SOBEL_BLUR), None),
        ("distance_transform_edt, single background pixel", lambda: som_device.distance_transform_edt(single, out=out_edt, check=False),
         1 + 4 + 4 + 8),
    ]
    print("K25 fibre markers: scripts/fiber_markers_bench.py --size %d --reps %d on %s" % (n, args.reps, torch.cuda.get_device_name(0)))
    print("plane: %d x %d bars of width 2 .. 7, %.1f %% foreground; ridge_cutoff %g, sobel_blur %g; thresholds %.4f, %.4f"
          % (n, n, 100.0 * fg_host.mean(), CUTOFF, SOBEL_BLUR, t0, t1))
    print("%-50s %10s %10s %8s %12s" % ("entry (HIP events, after a warm-up call)", "median ms", "min ms", "B/pixel", "HBM bound ms"))
    for name, call, bytes_per_pixel in rows:
        median, least = events_ms(args.reps, call)
        bound = "" if bytes_per_pixel is None else "%.4f" % (1e3 * bytes_per_pixel * pixels / HBM_BYTES_PER_S)
        print("%-50s %10.4f %10.4f %8s %12s" % (name, median, least, "" if bytes_per_pixel is None else bytes_per_pixel, bound))

    # the second pass of the distance transform reads 2 entries of g per step of its outward search; a pixel at distance
    # d stops after at most ceil(d) steps
    steps = np.ceil(edt.cpu().numpy()).sum()
    yy, xx = np.mgrid[:n, :n]
    reach = np.maximum(xx, n - 1 - xx)
    worst = np.minimum(np.ceil(np.hypot(yy - n // 3, xx - n // 3)), reach).sum()
    print("search windows of the second pass on this plane: %.3g steps in all, %.3f per pixel, %.2f per foreground pixel; "
          "single background pixel: %.3g steps" % (steps, steps / pixels, steps / max(1, int(fg_host.sum())), worst))

    fs.fiber_watershed_inputs(ridges_host, CUTOFF, SOBEL_BLUR)                   # warm-up
    walls = []
    for _ in range(args.reps):
        w0 = time.perf_counter()
        got = fs.fiber_watershed_inputs(ridges_host, CUTOFF, SOBEL_BLUR)
        walls.append(time.perf_counter() - w0)
    print("fiber_watershed_inputs from a host plane (upload, kernels, three downloads): %.2f ms median, %.2f ms min (host clock)"
          % (1e3 * float(np.median(walls)), 1e3 * min(walls)))
    print("marker classes 0 / 1 / 2: %s; elevation max %d" % (np.bincount(got.markers.ravel(), minlength=3).tolist(), got.elevation_map.max()))
    if not args.no_host:
        w0 = time.perf_counter()
        want = fmr.stages(ridges_host, CUTOFF, SOBEL_BLUR)
        print("scipy / numpy statement on the same host: %.0f ms (one run)" % (1e3 * (time.perf_counter() - w0)))
        checks = {"fg": np.array_equal(fg.cpu().numpy(), want["fg"]),
                  "edt": np.array_equal(edt.cpu().numpy(), fmr.distance_transform_edt(fg_host)),
                  "dist": np.array_equal(got.distance_transformed, want["dist"]),
                  "counts": np.array_equal(counts.cpu().numpy(), want["counts"]),
                  "thresholds": got.thresholds.tolist() == [want["t0"], want["t1"]],
                  "markers": np.array_equal(got.markers, want["markers"]),
                  "elev": np.array_equal(som_device.sobel_magnitude(smooth).cpu().numpy(), want["elev"]),
                  "elevation": np.array_equal(got.elevation_map, want["elevation"])}
        print("equal to the statement: " + ", ".join("%s %s" % kv for kv in checks.items()))
        if not all(checks.values()):
            sys.exit(1)


if __name__ == "__main__":
    main()
