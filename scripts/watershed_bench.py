#!/usr/bin/env python
"""Times the K28 entries -- the marker watershed and the chain from a raw channel to filtered fibre labels -- on synthetic
planes (default 2048 x 2048) and checks the labels against the heap statement of tests/watershed_reference.py.

Prints: the watershed alone on the elevation and markers that the K25 chain makes from a plane of bars (HIP events around
single calls, median and minimum of ``--reps`` after a warm-up call), with its rounds, levels and basin rounds, the time per
host-driven step (a round or a level start: its launches and its one read-back) and, for scale, the cost of a bare 40-byte
read-back on an idle stream; channel_fiber_labels beside channel_watershed_inputs on a raw channel; the adversarial plane, a
single marker on a flat plane, where the rounds number about H + W; and one plane of random levels, where most rounds take
the basin path.  The capability is new: there is no earlier time to compare with.  Per-kernel device times come from a
profiler run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/watershed_bench.py --reps 3 --no-host
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.fiber_markers_bench import CUTOFF, SOBEL_BLUR, bar_plane, events_ms  # noqa: E402

BLUR, SIGMAS = 2.0, (1, 3, 5, 7, 9)


def row(name, median, least, stats=None):
    steps = "" if stats is None else "  rounds %5d  levels %2d  basin rounds %3d  %.1f us per step" % (
        stats["rounds"], stats["levels"], stats["descents"], 1e3 * median / max(1, stats["rounds"] + stats["levels"]))
    print("%-58s %10.4f %10.4f%s" % (name, median, least, steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the heap statement on the host (profiler runs)")
    args = ap.parse_args()

    import torch
    from ark_analysis_amd import _capi, som_device
    from scripts.frangi_bench import bar_plane as channel_plane
    from tests import fiber_markers_reference as fmr
    from tests import watershed_reference as wr
    dev = _capi.require_gpu()
    n, reps = args.size, args.reps

    fg_host = bar_plane(n)
    ridges = torch.from_numpy(fmr.ridge_plane(fg_host, CUTOFF)).to(dev)
    _, _, markers, elevation = som_device.watershed_inputs(ridges, CUTOFF, SOBEL_BLUR)
    out = torch.empty_like(markers)
    classes = torch.bincount(markers.flatten(), minlength=3).tolist()
    print("K28 watershed: scripts/watershed_bench.py --size %d --reps %d on %s" % (n, reps, torch.cuda.get_device_name(0)))
    print("bars: %d x %d, %.1f %% foreground through the K25 chain; marker classes 0 / 1 / 2: %s (%.1f %% of the plane marked); "
          "elevation values %s" % (n, n, 100.0 * fg_host.mean(), classes, 100.0 * (classes[1] + classes[2]) / (n * n),
                                   torch.unique(elevation).tolist()))
    print("%-58s %10s %10s" % ("entry (HIP events, after a warm-up call)", "median ms", "min ms"))
    _, stats = som_device.watershed(elevation, markers, out=out, return_stats=True)
    row("watershed, bars", *events_ms(reps, lambda: som_device.watershed(elevation, markers, out=out)), stats)

    word = torch.zeros(5, dtype=torch.int64, device=dev)
    row("a 40-byte read-back on an idle stream (tensor.cpu())", *events_ms(max(reps, 50), lambda: word.cpu()))

    k = max(1, n // 128)
    channel = torch.from_numpy(channel_plane(n) * 200.0).to(dev)
    row("channel_watershed_inputs, resident channel (K27 .. K25)",
        *events_ms(reps, lambda: som_device.channel_watershed_inputs(channel, BLUR, k, SIGMAS, CUTOFF, SOBEL_BLUR)))
    row("channel_fiber_labels, resident channel (K27 .. K23)",
        *events_ms(reps, lambda: som_device.channel_fiber_labels(channel, BLUR, k, SIGMAS, CUTOFF, SOBEL_BLUR)))
    chain = som_device.channel_fiber_labels(channel, BLUR, k, SIGMAS, CUTOFF, SOBEL_BLUR)
    _, chain_stats = som_device.watershed(chain[6], chain[5], return_stats=True)
    row("watershed inside that chain",
        *events_ms(reps, lambda: som_device.watershed(chain[6], chain[5], out=out)), chain_stats)
    print("fibres kept by the chain: %d labels" % (torch.unique(chain[0]).numel() - 1))

    flat = torch.zeros((n, n), dtype=torch.int32, device=dev)
    single = torch.zeros_like(flat)
    single[0, 0] = 1
    _, flat_stats = som_device.watershed(flat, single, out=out, return_stats=True)
    row("watershed, one marker in the corner of a flat plane", *events_ms(min(reps, 3), lambda: som_device.watershed(flat, single, out=out)),
        flat_stats)
    assert bool((out == 1).all())

    m = min(n, 512)
    rs = np.random.RandomState(3)
    rough_host = rs.randint(0, 4, (m, m)).astype(np.int32)
    seeds_host = ((rs.random_sample((m, m)) < 0.001) * rs.randint(1, 4, (m, m))).astype(np.int32)
    rough, seeds = torch.from_numpy(rough_host).to(dev), torch.from_numpy(seeds_host).to(dev)
    rough_out, rough_stats = som_device.watershed(rough, seeds, return_stats=True)
    row("watershed, %d x %d of 4 random levels, 0.1 %% marked" % (m, m),
        *events_ms(min(reps, 3), lambda: som_device.watershed(rough, seeds)), rough_stats)

    if not args.no_host:
        w0 = time.perf_counter()
        want = wr.watershed(elevation.cpu().numpy(), markers.cpu().numpy())
        wall = time.perf_counter() - w0
        som_device.watershed(elevation, markers, out=out)
        checks = {"bars": np.array_equal(out.cpu().numpy(), want),
                  "random levels": np.array_equal(rough_out.cpu().numpy(), wr.watershed(rough_host, seeds_host))}
        print("heap statement on the same host, bars: %.0f ms (one run)" % (1e3 * wall))
        print("equal to the statement: " + ", ".join("%s %s" % kv for kv in checks.items()))
        if not all(checks.values()):
            sys.exit(1)


if __name__ == "__main__":
    main()
