"""bench.py on one GPU: a plain run does the timed steps and prints the headline (plus what the timed steps themselves measure),
nothing else; `--full` adds the legs that take runs of their own.  One FOV per run, so the lines say nothing about speed.
`-m gpu` only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "batch_train", "online_train", "operating_range", "consensus")


def _bench_line(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--fovs-per-gpu", "1",
           *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert res.returncode == 0 and len(lines) == 1, res.stdout[-2000:] + res.stderr[-4000:]
    return json.loads(lines[0])


def test_plain_bench_line_is_the_headline_only(tmp_path):
    dump = tmp_path / "dump"
    line = _bench_line(tmp_path, "--dump-outputs", str(dump))
    assert all(k in line for k in HEADLINE)
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert not any(k in line for k in FULL_ONLY)
    phases = line["phases_ms"]
    assert "train_batch" not in phases and "assign_and_mean_table" not in phases
    assert phases["assign_filter_kernel"] > 0 and line["roofline"]["launches_timed"] == 2
    rows = line["config"]["rows_per_gpu"]
    labels = np.load(dump / "labels.npy").astype(np.int64)     # 1-based node ids (include/pxsom.h)
    counts = np.load(dump / "cluster_counts.npy")
    assert labels.shape == (rows,) and np.load(dump / "codebook.npy").shape == (100, 22)
    assert labels.min() >= 1 and labels.max() <= 100
    assert counts.sum() == rows and np.array_equal(np.bincount(labels - 1, minlength=100), counts)
    assert np.load(dump / "cluster_means.npy").shape == (100, 22)


def test_full_bench_line_adds_the_phase_run_and_operating_range(tmp_path):
    line = _bench_line(tmp_path, "--full", "--no-pmc", "--no-cpu-baseline", "--no-online")
    assert all(k in line for k in HEADLINE) and line["value"] > 0
    assert line["phases_ms"]["train_batch"] > 0 and line["phases_ms"]["assign_and_mean_table"] > 0
    assert "measured" in line["phases_ms"]
    assert line["operating_range"]["trained codebook"]["assign_ms"] > 0
    assert "cpu_baseline" not in line and "online_train" not in line
