#!/usr/bin/env python
"""Times K30 -- exact t-SNE and PCA of a cell table on the device -- on synthetic tables of ``--sizes`` rows x 30 float32
columns (eight blobs) and writes profiles/k30_tsne_bench.txt (``--out``).

Per size: the squared distances and the affinities (host clock around a synchronise, one run each), milliseconds per descent
iteration without the error terms (HIP events around ``--steps`` iterations after a warm-up, median of ``--reps``), the same
with the error terms, the whole 1000-iteration run of som_device.tsne with its read-backs, and the PCA scores.  Spot checks
at every size (they matter past 2^31 elements): rows 0 and n - 1 of d2 equal the numpy statement, P is symmetric and sums
to 1 (plus at most eps per clamped pair).  Beside it scikit-learn on the same machine's host, exactly as the reference
calls it (``TSNE()``, ``PCA()``), for ``--host-sizes``.  No pass mark is set.

The split of an iteration into its launches comes from a profiler run of its own, per size:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/n<rows> -o t -- python scripts/tsne_bench.py --profile-rows <rows>
(uniform P and a normal embedding: the launches' work does not depend on the values) and is read back with
``--kernel-stats DIR``.  The gradient launch streams P once, 8 n^2 bytes; its rate is set against the 6.29 TB/s measured copy
rate of the MI355X.
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = 30
COPY_RATE = 6.29e12


def table(n, seed=30):
    r = np.random.RandomState(seed)
    centres = r.normal(0, 4.0, size=(8, COLUMNS))
    return (centres[np.arange(n) % 8] + r.normal(0, 1, size=(n, COLUMNS))).astype(np.float32)


def d2_row(x, i):
    """Row i of tests/tsne_reference.py pair_sqdist_f32 without the other rows."""
    x = x.astype(np.float64)
    s = np.zeros(x.shape[0])
    for t in range(x.shape[1]):
        d = x[i, t] - x[:, t]
        s += d * d
    return s.astype(np.float32)


def synced(torch, call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def step_state(torch, sd, n, dev):
    g = torch.Generator(device="cpu").manual_seed(n)
    y = (5.0 * torch.randn((n, 2), dtype=torch.float64, generator=g)).to(dev)
    return {"y": y, "y_next": torch.empty_like(y), "update": torch.zeros_like(y), "gains": torch.ones_like(y),
            "ws": torch.empty(sd.tsne_workspace_bytes(n), dtype=torch.uint8, device=dev),
            "err": torch.empty(2, dtype=torch.float64, device=dev)}


def run_steps(sd, P, s, count, want_error=False):
    lr = sd.tsne_learning_rate(P.shape[0])
    for _ in range(count):
        sd.tsne_step(P, s["y"], s["y_next"], s["update"], s["gains"], 1.0, 0.8, lr, error=s["err"] if want_error else None,
                     workspace=s["ws"])
        s["y"], s["y_next"] = s["y_next"], s["y"]


def iteration_ms(torch, sd, P, s, steps, reps, want_error=False):
    run_steps(sd, P, s, 3, want_error)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run_steps(sd, P, s, steps, want_error)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / steps)
    return float(np.median(times)), float(np.min(times))


def kernel_split(stats_dir, n):
    """Average microseconds per launch of the step's kernels from a rocprofv3 --stats run, or None."""
    files = glob.glob(os.path.join(stats_dir, "n%d" % n, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    out = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            for key in ("tsne_z_rows_kernel", "tsne_gradient_kernel", "fold_kernel"):
                if key in row["Name"]:
                    out[key] = out.get(key, 0.0) + float(row["TotalDurationNs"]) / 1e3
                    out[key + "#"] = out.get(key + "#", 0) + int(row["Calls"])
    return {k: out[k] / out[k + "#"] for k in out if not k.endswith("#")} or None


def profile_run(rows, steps):
    import torch
    from ark_analysis_amd import _capi, som_device as sd
    dev = _capi.require_gpu()
    P = torch.full((rows, rows), 1.0 / (rows * rows), dtype=torch.float64, device=dev)
    s = step_state(torch, sd, rows, dev)
    run_steps(sd, P, s, steps)
    torch.cuda.synchronize()
    print("profile run: %d iterations at %d rows" % (steps, rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 20000, 50000])
    ap.add_argument("--host-sizes", type=int, nargs="*", default=[5000, 20000, 50000])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-stats", default=None, help="directory of the per-size profiler runs")
    ap.add_argument("--profile-rows", type=int, default=None, help="only run --steps iterations at this size (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k30_tsne_bench.txt"))
    args = ap.parse_args()
    if args.profile_rows:
        return profile_run(args.profile_rows, args.steps)

    import torch
    from ark_analysis_amd import _capi, som_device as sd
    from tests import tsne_reference as ts
    dev = _capi.require_gpu()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("K30 t-SNE and PCA: scripts/tsne_bench.py --sizes %s --steps %d --reps %d on %s (one MI355X, gfx950)."
        % (" ".join(str(s) for s in args.sizes), args.steps, args.reps, torch.cuda.get_device_name(0)))
    say("Tables of n x %d float32 (eight blobs), perplexity 30.  ms / iteration: HIP events around %d iterations, median (min)"
        % (COLUMNS, args.steps))
    say("of %d; the other times: a host clock around one call that ends in a synchronise.  P share: 8 n^2 bytes over the"
        % args.reps)
    say("gradient launch's time (profiler run) against the measured 6.29 TB/s copy rate.")
    ok = True
    for n in args.sizes:
        x_host = table(n)
        x = torch.from_numpy(x_host).to(dev)
        sd.pair_sqdist_f32(x[:64].contiguous())                       # (code objects loaded before the first timing)
        d2, t_d2 = synced(torch, lambda: sd.pair_sqdist_f32(x))
        rows_ok = all(np.array_equal(d2[i].cpu().numpy(), d2_row(x_host, i)) for i in (0, n - 1))
        (P, beta, steps), t_aff = synced(torch, lambda: sd.tsne_affinities(d2, 30.0))
        del d2
        pick = torch.from_numpy(np.random.RandomState(1).randint(0, n, size=(2, 4096))).to(dev)
        total = float(P.sum().item()) - n * ts.EPS                    # (the diagonal holds eps)
        # every pair clamped to eps adds up to eps to the sum: at most n^2 eps in all
        p_ok = bool((P[pick[0], pick[1]] == P[pick[1], pick[0]]).all().item()) and -1e-10 < total - 1.0 < n * n * ts.EPS + 1e-10
        ok = ok and rows_ok and p_ok
        say()
        say("n = %d  (P %.2f GB, d2 %.2f GB)" % (n, 8e-9 * n * n, 4e-9 * n * n))
        say("  squared distances %10.1f ms     affinities %10.1f ms  (search steps: median %d, max %d)"
            % (t_d2, t_aff, int(steps.median().item()), int(steps.max().item())))
        say("  spot checks: d2 rows 0 and n - 1 equal the statement: %s; P symmetric and sum(P) - 1 = %.1e: %s"
            % (rows_ok, total - 1.0, p_ok))
        s = step_state(torch, sd, n, dev)
        med, least = iteration_ms(torch, sd, P, s, args.steps, args.reps)
        med_e, least_e = iteration_ms(torch, sd, P, s, args.steps, args.reps, want_error=True)
        say("  iteration               %8.3f ms (%.3f)   with the error terms %8.3f ms (%.3f)" % (med, least, med_e, least_e))
        split = kernel_split(args.kernel_stats, n) if args.kernel_stats else None
        if split and "tsne_gradient_kernel" in split:
            z, g, f = split.get("tsne_z_rows_kernel", float("nan")), split["tsne_gradient_kernel"], split.get("fold_kernel", float("nan"))
            rate = 8.0 * n * n / (g * 1e-6)
            say("  launches (profiler run) Z rows %8.3f ms   fold %8.4f ms   gradient + update %8.3f ms = %.2f TB/s of P, %.0f %% "
                "of the copy rate" % (z / 1e3, f / 1e3, g / 1e3, rate / 1e12, 100 * rate / COPY_RATE))
        else:
            say("  launches: no profiler run given (--kernel-stats); 8 n^2 / the whole iteration = %.2f TB/s"
                % (8.0 * n * n / (med * 1e-3) / 1e12))
        y0 = (1e-4 * torch.randn((n, 2), dtype=torch.float64, generator=torch.Generator().manual_seed(1))).to(dev)
        res, t_run = synced(torch, lambda: sd.tsne(P, y0))
        say("  1000-iteration run      %8.2f s   (n_iter %d, KL %.4f)" % (t_run / 1e3, res.n_iter, res.kl_divergence))
        del P
        sd.pca_scores(x[:64].contiguous())
        _, t_pca = synced(torch, lambda: sd.pca_scores(x))
        say("  PCA scores              %8.2f ms  (moments, eigenvectors on the host, projection)" % t_pca)
        if n in args.host_sizes:
            from sklearn.decomposition import PCA
            from sklearn.manifold import TSNE
            t0 = time.perf_counter()
            PCA().fit_transform(x_host)
            t_host_pca = time.perf_counter() - t0
            t0 = time.perf_counter()
            est = TSNE()
            est.fit_transform(x_host)
            t_host = time.perf_counter() - t0
            say("  host: sklearn PCA() %.1f ms; sklearn TSNE() (Barnes-Hut, %d threads) %.1f s, KL %.4f, n_iter %d"
                % (1e3 * t_host_pca, os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"]),
                   t_host, est.kl_divergence_, est.n_iter_))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
