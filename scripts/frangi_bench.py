#!/usr/bin/env python
"""Times the K26 entries -- the Frangi ridge filter of fibre segmentation -- on a synthetic float64 plane of noisy bright
bars (default 2048 x 2048) at the reference's widths (1, 3, 5, 7, 9) against the numpy / scipy statement of
tests/frangi_reference.py on the same host.

Prints a table: pxsom_frangi_scale alone on a resident blurred plane in its storing and its accumulating form, the plane
blur at each width, frangi over the five scales and ridge_watershed_inputs on a resident plane (HIP events around single
calls, median and minimum of ``--reps`` after a warm-up call; windows this short are indicative), frangi_ridges from a
host plane (host clock around the call, which ends in the download), the statement's wall time (one run, the only
baseline: the capability is new), whether every result equals the statement's, and the bound each kernel is judged
against: the HBM bytes per pixel of the stage over the MI355X's 8 TB/s.  Per-kernel device times come from a profiler run
of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/frangi_bench.py --reps 5 --no-host
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
SIGMAS = (1, 3, 5, 7, 9)
BETA, GAMMA, SCALE = 0.5, 15.0, 10000.0
CUTOFF, SOBEL_BLUR = 0.1, 1


def bar_plane(size, target=0.10, noise=0.05, seed=0):
    """Bright bars of half-width 1 .. 4 across a dark plane until `target` of it is covered, plus even noise."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:size, :size].astype(np.float32)
    fg = np.zeros((size, size), bool)
    while fg.mean() < target:
        theta, cy, cx, half = rs.uniform(0, np.pi), rs.uniform(0, size), rs.uniform(0, size), rs.randint(1, 5)
        fg |= np.abs((yy - cy) * np.cos(theta) - (xx - cx) * np.sin(theta)) <= half
    return fg.astype(np.float64) + noise * rs.random_sample((size, size))


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
    ap.add_argument("--no-host", action="store_true", help="skip the numpy / scipy statement (profiler runs)")
    args = ap.parse_args()

    from tests import fiber_markers_reference as fmr
    from tests import frangi_reference as fr
    n = args.size
    pixels = n * n
    plane_host = bar_plane(n)
    want = chain = None
    if not args.no_host:
        w0 = time.perf_counter()
        want = fr.stages(plane_host, SIGMAS, BETA, GAMMA, SCALE)
        statement_s = time.perf_counter() - w0
        w0 = time.perf_counter()
        chain = fmr.stages(want["ridges"], CUTOFF, SOBEL_BLUR)
        chain_s = time.perf_counter() - w0

    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    dev = _capi.require_gpu()
    plane = torch.from_numpy(plane_host).to(dev)
    g = {s: som_device.gaussian_blur_plane_mode(plane, s, "reflect") for s in SIGMAS}
    out, blurred, tmp = torch.empty_like(plane), torch.empty_like(plane), torch.empty_like(plane)
    bsq, gsq = 2.0 * BETA * BETA, 2.0 * GAMMA * GAMMA

    def scale_call(sigma, first):
        return lambda: _capi.call("pxsom_frangi_scale", g[sigma].data_ptr(), n, n, n, float(sigma) ** 2, bsq, gsq, first, 1.0,
                                  out.data_ptr(), n, _capi.stream_ptr())

    # bytes per pixel that must cross HBM, reads + writes
    rows = [("frangi_scale, first scale (stores)", scale_call(1, 1), 8 + 8),
            ("frangi_scale, later scale (folds)", scale_call(3, 0), 8 + 16)]
    rows += [("gaussian_blur_plane_mode sigma %d" % s,
              (lambda s: lambda: som_device.gaussian_blur_plane_mode(plane, s, "reflect", out=blurred, tmp=tmp))(s), 4 * 8) for s in SIGMAS]
    rows += [("frangi, five scales, resident plane", lambda: som_device.frangi(plane, SIGMAS, BETA, GAMMA, SCALE, out=out),
              5 * 4 * 8 + 16 + 4 * 24),
             ("ridge_watershed_inputs, resident plane", lambda: som_device.ridge_watershed_inputs(plane, SIGMAS, CUTOFF, SOBEL_BLUR), None)]
    print("K26 frangi: scripts/frangi_bench.py --size %d --reps %d on %s" % (n, args.reps, torch.cuda.get_device_name(0)))
    print("plane: %d x %d float64, bright bars of half-width 1 .. 4 plus 5 %% noise; sigmas %s, beta %g, gamma %g, scale %g"
          % (n, n, list(SIGMAS), BETA, GAMMA, SCALE))
    print("%-44s %10s %10s %8s %12s" % ("entry (HIP events, after a warm-up call)", "median ms", "min ms", "B/pixel", "HBM bound ms"))
    for name, call, bytes_per_pixel in rows:
        median, least = events_ms(args.reps, call)
        bound = "" if bytes_per_pixel is None else "%.4f" % (1e3 * bytes_per_pixel * pixels / HBM_BYTES_PER_S)
        print("%-44s %10.4f %10.4f %8s %12s" % (name, median, least, "" if bytes_per_pixel is None else bytes_per_pixel, bound))

    fs.frangi_ridges(plane_host)                                                  # warm-up
    walls = []
    for _ in range(args.reps):
        w0 = time.perf_counter()
        got_host = fs.frangi_ridges(plane_host)
        walls.append(time.perf_counter() - w0)
    print("frangi_ridges from a host plane (upload, kernels, one download): %.2f ms median, %.2f ms min (host clock)"
          % (1e3 * float(np.median(walls)), 1e3 * min(walls)))
    ridges, dist, (t0, t1), markers, elevation = som_device.ridge_watershed_inputs(plane, SIGMAS, CUTOFF, SOBEL_BLUR)
    print("ridges: max %.4f, %.1f %% above the cutoff %g; thresholds %.4f, %.4f; marker classes 0 / 1 / 2: %s"
          % (float(ridges.max()), 100.0 * float((ridges > CUTOFF).double().mean()), CUTOFF, t0, t1,
             torch.bincount(markers.flatten(), minlength=3).tolist()))
    if want is not None:
        print("numpy / scipy statement on the same host, one run: frangi %.0f ms, then the K25 stages %.0f ms"
              % (1e3 * statement_s, 1e3 * chain_s))
        scale_call(1, 1)()
        first = out.cpu().numpy()
        scale_call(3, 0)()
        checks = {"scale 1": np.array_equal(first, want["scales"][0]),
                  "fold of 1 and 3": np.array_equal(out.cpu().numpy(), np.maximum(want["scales"][0], want["scales"][1])),
                  "folded": np.array_equal(som_device.frangi(plane, SIGMAS, BETA, GAMMA).cpu().numpy(), want["folded"]),
                  "ridges": np.array_equal(ridges.cpu().numpy(), want["ridges"]),
                  "frangi_ridges": np.array_equal(got_host, want["ridges"]),
                  "dist": np.array_equal(dist.cpu().numpy(), chain["dist"]),
                  "thresholds": [t0, t1] == [chain["t0"], chain["t1"]],
                  "markers": np.array_equal(markers.cpu().numpy(), chain["markers"]),
                  "elevation": np.array_equal(elevation.cpu().numpy(), chain["elevation"])}
        print("equal to the statement: " + ", ".join("%s %s" % kv for kv in checks.items()))
        if not all(checks.values()):
            sys.exit(1)


if __name__ == "__main__":
    main()
