#!/usr/bin/env python
"""Times the K27 entries -- adaptive histogram equalisation, the front of fibre segmentation -- on synthetic float64 planes
of noisy bright bars: 2048 x 2048 with k = 16 and 1024 x 1024 with k = 8 (the reference's 1024 / 128), against the numpy /
scipy statement of tests/clahe_reference.py on the same host.

Prints a table per plane: pxsom_clahe_quantize alone, pxsom_clahe_equalize alone under the default clip limit and with
clip_limit = 0 (the same three launches with the redistribution loop of clip_histogram never entered: the ablation that
prices the loop), contrast_adjust and channel_watershed_inputs on a resident plane (HIP events around single calls, median
and minimum of ``--reps`` after a warm-up call; windows this short are indicative), contrast_adjusted_channel from a host
plane (host clock around the call, which ends in the download), the statement's wall time (one run, the only baseline: the
capability is new), whether every result equals the statement's (the script fails if one does not), and the bound each
entry is judged against: the HBM bytes per pixel it must move over the MI355X's 8 TB/s.  Per-kernel device times come
from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/clahe_bench.py --reps 5 --no-host --plane 2048
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.frangi_bench import bar_plane, events_ms  # noqa: E402

HBM_BYTES_PER_S = 8e12
BLUR, CLIP_LIMIT = 2.0, 0.01
SIGMAS = (1, 3, 5, 7, 9)
CUTOFF, SOBEL_BLUR = 0.1, 1
PLANES = ((2048, 16), (1024, 8))


def bench(n, k, reps, host):
    from tests import clahe_reference as cr
    from tests import fiber_markers_reference as fmr
    from tests import frangi_reference as fr
    channel_host = bar_plane(n) * 200.0
    want = None
    if host:
        w0 = time.perf_counter()
        front = cr.front(channel_host, BLUR)
        front_s = time.perf_counter() - w0
        w0 = time.perf_counter()
        want = cr.equalize_adapthist(front, k, CLIP_LIMIT)
        statement_s = time.perf_counter() - w0
        want_noclip = cr.equalize_adapthist(front, k, 0.0)
        w0 = time.perf_counter()
        ridges = fr.frangi(want[0], SIGMAS, fr.BETA, fr.GAMMA, fr.SCALE)
        chain = fmr.stages(ridges, CUTOFF, SOBEL_BLUR)
        chain_s = time.perf_counter() - w0

    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    dev = _capi.require_gpu()
    pixels = n * n
    channel = torch.from_numpy(channel_host).to(dev)
    b = som_device.gaussian_blur_plane_mode(channel, BLUR, "reflect")
    lo, hi = som_device.plane_minmax(b)
    _capi.call("pxsom_plane_divide", b.data_ptr(), n, n, n, hi, b.data_ptr(), n, _capi.stream_ptr())
    gray = torch.empty((n, n), dtype=torch.uint16, device=dev)
    out = torch.empty((n, n), dtype=torch.float64, device=dev)
    nt = -(-n // k)
    maps = torch.empty((nt, nt, 256), dtype=torch.uint16, device=dev)
    raw = torch.empty((n, n), dtype=torch.uint16, device=dev)
    wsb = _capi.lib().pxsom_clahe_workspace_bytes(n, n, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def quantize():
        _capi.call("pxsom_clahe_quantize", b.data_ptr(), n, n, n, lo / hi, 1.0, gray.data_ptr(), n, _capi.stream_ptr())

    def equalize(clip_limit, with_stages=False):
        _, clim, map_scale = som_device.clahe_arguments((n, n), k, clip_limit)

        def call():
            _capi.call("pxsom_clahe_equalize", gray.data_ptr(), n, n, n, k, clim, map_scale, out.data_ptr(), n,
                       maps.data_ptr() if with_stages else None, raw.data_ptr() if with_stages else None, n, ws.data_ptr(), wsb,
                       _capi.stream_ptr())
        return call

    quantize()
    m = 512.0 / (k * k)                                         # bytes of tile map per pixel
    rows = [("clahe_quantize", quantize, 8 + 2),
            ("clahe_equalize (maps, interpolate, rescale)", equalize(CLIP_LIMIT), (2 + m) + (2 + m + 2) + (2 + 8)),
            ("clahe_equalize, clip_limit 0: no loop", equalize(0.0), (2 + m) + (2 + m + 2) + (2 + 8)),
            ("plane_divide (in place)", lambda: _capi.call("pxsom_plane_divide", out.data_ptr(), n, n, n, 1.0, out.data_ptr(), n,
                                                           _capi.stream_ptr()), 16),
            ("contrast_adjust, resident channel", lambda: som_device.contrast_adjust(channel, BLUR, k, CLIP_LIMIT, out=out), None),
            ("channel_watershed_inputs, resident channel",
             lambda: som_device.channel_watershed_inputs(channel, BLUR, k, SIGMAS, CUTOFF, SOBEL_BLUR), None)]
    print("plane: %d x %d float64, bright bars of half-width 1 .. 4 plus noise, times 200; blur %g, k = %d (%d tiles), clip_limit %g"
          % (n, n, BLUR, k, nt * nt, CLIP_LIMIT))
    print("%-46s %10s %10s %8s %12s" % ("entry (HIP events, after a warm-up call)", "median ms", "min ms", "B/pixel", "HBM bound ms"))
    for name, call, bytes_per_pixel in rows:
        median, least = events_ms(reps, call)
        bound = "" if bytes_per_pixel is None else "%.4f" % (1e3 * bytes_per_pixel * pixels / HBM_BYTES_PER_S)
        print("%-46s %10.4f %10.4f %8s %12s" % (name, median, least, "" if bytes_per_pixel is None else "%.1f" % bytes_per_pixel, bound))
        sys.stdout.flush()

    divisor = n / (k + 0.5)
    fs.contrast_adjusted_channel(channel_host, BLUR, divisor)                      # warm-up
    walls = []
    for _ in range(reps):
        w0 = time.perf_counter()
        got_host = fs.contrast_adjusted_channel(channel_host, BLUR, divisor)
        walls.append(time.perf_counter() - w0)
    print("contrast_adjusted_channel from a host plane (upload, kernels, one download): %.2f ms median, %.2f ms min (host clock)"
          % (1e3 * float(np.median(walls)), 1e3 * min(walls)))
    if want is None:
        return True
    print("numpy / scipy statement on the same host, one run: blur and division %.0f ms, equalize_adapthist %.0f ms, then "
          "frangi and the K25 stages %.0f ms" % (1e3 * front_s, 1e3 * statement_s, 1e3 * chain_s))
    quantize()
    checks = {"gray": np.array_equal(gray.cpu().numpy(), want[1])}
    equalize(CLIP_LIMIT, True)()
    checks.update(maps=np.array_equal(maps.cpu().numpy(), want[2]), raw=np.array_equal(raw.cpu().numpy(), want[3]),
                  equalize=np.array_equal(out.cpu().numpy(), want[0]))
    equalize(0.0, True)()
    checks["no clip"] = np.array_equal(maps.cpu().numpy(), want_noclip[2]) and np.array_equal(out.cpu().numpy(), want_noclip[0])
    checks["contrast_adjust"] = np.array_equal(som_device.contrast_adjust(channel, BLUR, k, CLIP_LIMIT).cpu().numpy(), want[0])
    checks["contrast_adjusted_channel"] = np.array_equal(got_host, want[0])
    contrast, rid, dist, (t0, t1), markers, elevation = som_device.channel_watershed_inputs(channel, BLUR, k, SIGMAS, CUTOFF, SOBEL_BLUR)
    checks.update(chain_contrast=np.array_equal(contrast.cpu().numpy(), want[0]), ridges=np.array_equal(rid.cpu().numpy(), ridges),
                  dist=np.array_equal(dist.cpu().numpy(), chain["dist"]), thresholds=[t0, t1] == [chain["t0"], chain["t1"]],
                  markers=np.array_equal(markers.cpu().numpy(), chain["markers"]),
                  elevation=np.array_equal(elevation.cpu().numpy(), chain["elevation"]))
    print("equal to the statement: " + ", ".join("%s %s" % kv for kv in checks.items()))
    return all(checks.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy / scipy statement (profiler runs)")
    ap.add_argument("--plane", type=int, default=0, help="only the plane of this side (a profiler run per plane keeps its kernel rows apart)")
    args = ap.parse_args()
    import torch
    print("K27 clahe: scripts/clahe_bench.py --reps %d on %s" % (args.reps, torch.cuda.get_device_name(0)))
    ok = True
    for n, k in PLANES:
        if args.plane and n != args.plane:
            continue
        ok &= bench(n, k, args.reps, not args.no_host)
        print()
        sys.stdout.flush()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
