#!/usr/bin/env python
"""Times the K29 entries -- the overlay chain of create_overlay on resident tensors and, separately, its compose kernel
pxsom_overlay_rgb -- on synthetic FOVs of 1024 x 1024 and 2048 x 2048 with int16 and float32 planes under a Voronoi-like
segmentation of about 20 000 cells, and writes profiles/k29_overlay_bench.txt (``--out``).

Per case: HIP events around single calls (median and minimum of ``--reps`` after a warm-up call) for the whole chain
(torch maxima, the percentile selects, the compose launch; two channels, as notebook 1 overlays them), for its phases, for
the compose kernel alone with its input + output bytes per second, and for the border plane alone; the numpy statement of
tests/overlay_reference.py on the same machine's host (one run); and whether the device equals it.  The capability is
new: there is no earlier implementation to compare with.  No pass mark is set.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.fiber_markers_bench import events_ms  # noqa: E402

CELLS = 20000


def planes_for(n, dtype, seed):
    """Two channels of a FOV: sparse gamma-distributed signal, zeros elsewhere."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        p = rs.gamma(2.0, 40.0, size=(n, n)) * (rs.random_sample((n, n)) < 0.7)
        out.append(p.astype(dtype))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy statement on the host (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k29_overlay_bench.txt"))
    args = ap.parse_args()

    import torch
    from ark_analysis_amd import _capi, som_device as sd
    from tests import overlay_reference as ovr
    from tests.cell_mask_reference import voronoi_labels
    dev = _capi.require_gpu()
    reps = args.reps
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("K29 overlays: scripts/overlay_bench.py --sizes %s --reps %d on %s (one MI355X, gfx950); HIP events around single"
        % (" ".join(str(s) for s in args.sizes), reps, torch.cuda.get_device_name(0)))
    say("calls, median and minimum after a warm-up call.  Two channels (red stays empty), int32 labels, no alternate")
    say("segmentation; bytes = the planes and labels read once plus the RGB image written.")
    ok = True
    for n in args.sizes:
        seg_host = voronoi_labels(n, n, CELLS, seed=29)
        seg = torch.from_numpy(seg_host).to(dev)
        for dtype in (np.int16, np.float32):
            host_planes = planes_for(n, dtype, seed=n)
            planes = [torch.from_numpy(p).to(dev) for p in host_planes]
            say()
            say("%d x %d, %s planes, %d cells, %.1f %% border pixels" % (n, n, np.dtype(dtype).name, CELLS,
                                                                       100.0 * ovr.inner_boundaries(seg_host).mean()))
            say("%-62s %10s %10s" % ("entry", "median ms", "min ms"))

            def row(name, call, nbytes=None):
                med, least = events_ms(reps, call)
                tail = "" if nbytes is None else "  %7.1f GB/s" % (nbytes / (med * 1e-3) / 1e9)
                say("%-62s %10.4f %10.4f%s" % (name, med, least, tail))
                return med

            chain = row("overlay_rgb: the whole chain, resident planes", lambda: sd.overlay_rgb(planes, seg))
            row("  maxima (torch) and their read-back",
                lambda: torch.stack([p.max().to(torch.float64) for p in planes]).cpu())
            row("  percentiles_positive (5, 95) of both channels and read-back",
                lambda: torch.stack([sd.percentiles_positive(p, (5, 95)) for p in planes]).cpu())
            modes, ranges = sd.overlay_ranges(planes)
            rgb_planes, rgb_modes, rgb_ranges = [None, planes[1], planes[0]], [0, modes[1], modes[0]], [(0.0, 0.0), ranges[1], ranges[0]]
            rgb = torch.empty((n, n, 3), dtype=torch.uint8, device=dev)
            borders = torch.empty((n, n), dtype=torch.uint8, device=dev)
            nbytes = n * n * (2 * np.dtype(dtype).itemsize + 4 + 3)
            row("  pxsom_overlay_rgb: the compose kernel alone",
                lambda: sd.overlay_compose(rgb_planes, rgb_modes, rgb_ranges, seg, rgb=rgb), nbytes)
            row("pxsom_overlay_rgb: the border plane alone",
                lambda: sd.overlay_compose([None] * 3, [0] * 3, [(0.0, 0.0)] * 3, seg, want_rgb=False, want_borders=True,
                                           borders=borders), n * n * 5)
            if not args.no_host:
                tif = np.stack(host_planes, axis=-1)
                t0 = time.perf_counter()
                want = ovr.overlay(tif, seg_host)
                wall = 1e3 * (time.perf_counter() - t0)
                same = np.array_equal(sd.overlay_rgb(planes, seg).cpu().numpy(), want)
                ok = ok and same
                say("numpy statement on the same host (one run): %.0f ms, %.0f x the chain; device equals it: %s"
                    % (wall, wall / chain, same))
        table = torch.from_numpy(ovr.color_table(np.random.RandomState(1).rand(30, 4))).to(dev)
        mask = torch.from_numpy(np.random.RandomState(2).randint(0, 30, size=(n, n)).astype(np.int16)).to(dev)
        out = torch.empty((n, n, 4), dtype=torch.uint8, device=dev)
        med, least = events_ms(reps, lambda: sd.colorize(mask, table, out=out))
        say()
        say("%-62s %10.4f %10.4f  %7.1f GB/s" % ("pxsom_colorize: %d x %d int16 mask, 30 x 4 table (+ status)" % (n, n), med, least,
                                               n * n * 6 / (med * 1e-3) / 1e9))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
