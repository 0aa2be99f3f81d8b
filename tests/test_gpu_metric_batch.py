"""K6m on the device: pxsom_assign_sums_metric against the reference statement, whole training runs under distf 1 / 3 / 4
against the reference loop (tests/metric_batch_reference.py), two shards in one process, the front end and label_table.

Every comparison but one is array_equal: binary64 rows join the sums rounded to the exact quantum, binary32 rows hold small
integers and binary16 values are multiples of 2^-24 below 2^16 (5000 of them sum exactly in binary64), so the statistics do not
depend on the order of the additions."""
import numpy as np
import pytest
import torch

from tests import metric_batch_reference as mbr
from tests import metric_reference as mr
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

METRICS = [1, 3, 4]
# (c, k): small; padded nodes 112; the register / staged boundary (32 | 33); the largest LDS table; past the LDS limit
SHAPES = [(7, 12), (22, 100), (32, 16), (33, 16), (40, 400), (64, 1024)]
NS = (1, 63, 64, 257, 5000)
SENTINEL = -7


def _codebook(c, k, seed):
    rng = np.random.RandomState(seed)
    w = rng.gamma(2.0, 1.0, size=(k, c))
    w[rng.random_sample((k, c)) < 0.3] = 0.0
    w[k // 2] = w[1]          # two equal nodes: the first one wins every tie
    if k > 8:
        w[k - 1] = 0.0        # a zero node (cosine: NaN distance, never chosen)
    return w


def _rows(c, n, seed, kind, w):
    """Rows of one storage type, with planted rows: a NaN entry, all-zero rows, copies of nodes (ties)."""
    x = mbr.test_rows(n, c, seed)
    if kind == "f32":
        x = np.floor(x * 4.0)                 # small integers: exact sums in any order
    planted = [p for p in (3, 40, 41, 200, 4100) if p < n]
    if n > 3:
        x[3, c // 2] = np.nan
    for p in planted[1:3]:
        x[p] = 0.0
    for p in planted[3:]:
        x[p] = w[1] if kind == "f64" else np.floor(w[1])
    dtype = {"f64": np.float64, "f32": np.float32, "f16": np.float16}[kind]
    return np.ascontiguousarray(x.astype(dtype))


def _window_rows(n, window):
    phases, e0, e1 = window
    i = np.arange(n)
    return i[(i % phases >= e0) & (i % phases < e1)]


def _configs(kind, big):
    """(n, window, extra leading dimension): every row count, every window, ldx > c."""
    ns = NS if (kind == "f32" or not big) else NS[:4]     # (the 1024 x 64 reference search at 5000 rows: one storage type)
    out = [(n, (1, 0, 1), 3 if n % 2 else 0) for n in ns]
    out += [(ns[-1], (7, 2, 5), 5), (257, (7, 2, 5), 0), (64, (3, 0, 1), 1), (500, (960, 959, 960), 0), (959, (960, 959, 960), 2)]
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_k%d" % s)
@pytest.mark.parametrize("metric", METRICS)
def test_assign_sums_metric_is_the_reference_statement(gpu, metric, shape):
    from ark_analysis_amd import som_device
    c, k = shape
    big = k * c > 20000
    w = _codebook(c, k, 100 + c)
    wd = torch.from_numpy(w).to(gpu)
    ws = som_device.MetricStepWorkspace(c, k, gpu, metric)
    for kind in ("f64", "f32", "f16"):
        cfgs = _configs(kind, big)
        nmax = max(n for n, _, _ in cfgs)
        x = _rows(c, nmax, 7 + c + k, kind, w)
        x64 = x.astype(np.float64)
        labels_ref, _ = mr.map_data_to_nodes(w, x64, metric)
        zero_share = float((labels_ref == 0).mean())
        print("metric %d c=%d k=%d %s: label-0 share %.4f of %d rows" % (metric, c, k, kind, zero_share, nmax))
        assert zero_share < 0.05
        finite = np.abs(x64[np.isfinite(x64)])
        quantum = som_device.exact_sum_quantum(float(finite.max()), 2 * nmax) if kind == "f64" else 0.0
        for n, window, pad in cfgs:
            xt = torch.full((n, c + pad), 1.0e4, dtype=torch.from_numpy(x).dtype, device=gpu)   # (the padding is never read)
            xt[:, :c] = torch.from_numpy(x[:n]).to(gpu)
            view = xt[:, :c]
            idx = _window_rows(n, window)
            with np.errstate(all="ignore"):
                s, cnt = ob.cluster_sums(ob.quantize(x64[idx], quantum), labels_ref[idx], k)
            want = np.concatenate([s.reshape(-1), cnt.astype(np.float64)])
            labels = torch.full((n,), SENTINEL, dtype=torch.int32, device=gpu)
            stats = torch.zeros(k * (c + 1), dtype=torch.float64, device=gpu)
            som_device.assign_sums_metric(view, wd, metric, labels=labels, stats=stats, quantum=quantum, window=window, workspace=ws)
            got_l, got_s = labels.cpu().numpy(), stats.cpu().numpy()
            what = "%s n=%d window=%s ldx=%d" % (kind, n, window, c + pad)
            expect_l = np.full(n, SENTINEL, dtype=np.int32)
            expect_l[idx] = labels_ref[idx]
            np.testing.assert_array_equal(got_l, expect_l, err_msg=what)                  # labels; the others untouched
            np.testing.assert_array_equal(got_s[k * c:], want[k * c:], err_msg=what)      # counts
            np.testing.assert_array_equal(got_s[:k * c], want[:k * c], err_msg=what)      # sums
            # a second call ADDS (and takes no labels): the statistics double
            som_device.assign_sums_metric(view, wd, metric, labels=None, stats=stats, quantum=quantum, window=window, workspace=ws)
            np.testing.assert_array_equal(stats.cpu().numpy(), 2.0 * want, err_msg=what + " (second call)")


@pytest.mark.parametrize("shape", [(7, 12), (33, 16)], ids=lambda s: "c%d_k%d" % s)
@pytest.mark.parametrize("metric", METRICS)
def test_the_grid_does_not_matter(gpu, metric, shape):
    """More rows than the grid holds at once -- the workgroups resident on the 256 CUs (3 per CU by registers for register rows:
    3 x 256 x 256 = 196 608 rows; never more than 8 per CU) -- so every workgroup loops.  (Cosine with labels asked for takes the
    two launches; the second call below, without labels, is the one pass.)"""
    from ark_analysis_amd import som_device
    c, k = shape
    n = 270001
    w = _codebook(c, k, 5)
    x = _rows(c, n, 11, "f32", w)
    x64 = x.astype(np.float64)
    labels_ref, _ = mr.map_data_to_nodes(w, x64, metric)
    with np.errstate(all="ignore"):
        s, cnt = ob.cluster_sums(x64, labels_ref, k)
    labels, stats = som_device.assign_sums_metric(torch.from_numpy(x).to(gpu), torch.from_numpy(w).to(gpu), metric)
    np.testing.assert_array_equal(labels.cpu().numpy(), labels_ref)
    want = np.concatenate([s.reshape(-1), cnt.astype(np.float64)])
    np.testing.assert_array_equal(stats.cpu().numpy(), want)
    labels.fill_(SENTINEL)
    labels, stats = som_device.assign_sums_metric(torch.from_numpy(x).to(gpu), torch.from_numpy(w).to(gpu), metric, labels=labels,
                                                  stats=stats, window=(2, 0, 2))     # (a window of every row, written the long way)
    np.testing.assert_array_equal(labels.cpu().numpy(), labels_ref)
    _, stats = som_device.assign_sums_metric(torch.from_numpy(x).to(gpu), torch.from_numpy(w).to(gpu), metric, stats=stats.zero_(),
                                             window=(8, 0, 7))                        # 7 phases of 8 (236 251 rows): always the one pass
    idx = _window_rows(n, (8, 0, 7))
    with np.errstate(all="ignore"):
        s, cnt = ob.cluster_sums(x64[idx], labels_ref[idx], k)
    np.testing.assert_array_equal(stats.cpu().numpy(), np.concatenate([s.reshape(-1), cnt.astype(np.float64)]))


@pytest.mark.parametrize("metric", METRICS)
def test_general_binary32_rows_without_a_quantum(gpu, metric):
    """Quantum 0: binary64 additions in unspecified order.  Any order of m binary64 additions is within m 2^-53 sum|x| of the
    exact sum, so two orders differ by at most twice that."""
    from ark_analysis_amd import som_device
    c, k, n = 22, 100, 5000
    w = _codebook(c, k, 9)
    x = mbr.test_rows(n, c, 13, np.float32)
    x64 = x.astype(np.float64)
    labels_ref, _ = mr.map_data_to_nodes(w, x64, metric)
    s, cnt = ob.cluster_sums(x64, labels_ref, k)
    a, _ = ob.cluster_sums(np.abs(x64), labels_ref, k)
    labels, stats = som_device.assign_sums_metric(torch.from_numpy(x).to(gpu), torch.from_numpy(w).to(gpu), metric)
    got = stats.cpu().numpy()
    np.testing.assert_array_equal(labels.cpu().numpy(), labels_ref)
    np.testing.assert_array_equal(got[k * c:], cnt.astype(np.float64))
    bound = 2.0 * cnt[:, None] * 2.0 ** -53 * a
    err = np.abs(got[:k * c].reshape(k, c) - s)
    print("metric %d: largest error / bound %.3g" % (metric, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()


def test_metric_2_and_bad_windows_are_refused_by_the_wrapper(gpu):
    from ark_analysis_amd import _capi, som_device
    x = torch.zeros((8, 3), dtype=torch.float32, device=gpu)
    w = torch.zeros((4, 3), dtype=torch.float64, device=gpu)
    with pytest.raises(_capi.PxsomError):
        som_device.assign_sums_metric(x, w, 2)
    with pytest.raises(ValueError, match="unknown metric"):
        som_device.assign_sums_metric(x, w, 5)
    with pytest.raises(_capi.PxsomError, match="window"):
        som_device.assign_sums_metric(x, w, 1, window=(4, 2, 2))


# ---- whole runs ------------------------------------------------------------------------------------------------------
def _two_phase():
    from ark_analysis_amd.schedule import BatchSchedule
    return BatchSchedule.two_phase()


# (rows, channels, xdim, ydim, schedule, passes)
RUNS = {"3000x7_4x3": (3000, 7, 4, 3, 5, 2), "6000x22_10x10": (6000, 22, 10, 10, _two_phase, 1), "2000x40_20x20": (2000, 40, 20, 20, 4, 1)}
ALPHA = (0.05, 0.01)


def _run_inputs(name):
    from ark_analysis_amd import flowsom
    n, c, xdim, ydim, sched, passes = RUNS[name]
    sched = sched() if callable(sched) else sched
    x = mbr.test_rows(n, c, 31 + c)
    x[5] = 0.0
    x[n // 2] = 0.0                       # all-zero rows: label 0 under cosine
    nodes = x[np.random.RandomState(3).choice(n, xdim * ydim, replace=False)].copy()
    return x, nodes, xdim, ydim, sched, passes, flowsom.default_radius_range(xdim, ydim)


_reference_runs = {}


def _reference_run(name, metric):
    """The reference loop's codebook of a run, computed once and shared (never modified)."""
    if (name, metric) not in _reference_runs:
        x, nodes, xdim, ydim, sched, passes, rr = _run_inputs(name)
        w = mbr.som_batch([x], nodes, xdim, ydim, passes, sched, ALPHA, rr, metric, quantum=mbr.run_quantum([x], sched))
        w.setflags(write=False)
        _reference_runs[(name, metric)] = w
    return _reference_runs[(name, metric)]


def _device_run(gpu, x, nodes, xdim, ydim, sched, passes, rr, metric, quantum, one_step_per_call):
    from ark_analysis_amd import distributed
    from ark_analysis_amd.schedule import resolve
    kern = distributed.HipKernels(metric=metric)
    xd, w = torch.from_numpy(x).to(gpu), torch.from_numpy(nodes).to(gpu)
    kern.begin(xd, w, xdim, ydim, sched, quantum=quantum)
    total = passes * resolve(sched).steps
    if one_step_per_call:
        for g in range(total):
            kern.steps(xd, g, g + 1, total, ALPHA, rr)
    else:
        kern.steps(xd, 0, total, total, ALPHA, rr)
    out = torch.empty_like(w)
    kern.finish(total, total, ALPHA, rr, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(RUNS))
@pytest.mark.parametrize("metric", METRICS)
def test_whole_run_is_the_reference_loop(gpu, metric, name):
    x, nodes, xdim, ydim, sched, passes, rr = _run_inputs(name)
    q = mbr.run_quantum([x], sched)
    want = _reference_run(name, metric)
    got = _device_run(gpu, x, nodes, xdim, ydim, sched, passes, rr, metric, q, False)
    np.testing.assert_array_equal(got, want)
    stepwise = _device_run(gpu, x, nodes, xdim, ydim, sched, passes, rr, metric, q, True)
    np.testing.assert_array_equal(stepwise, got)
    assert np.abs(want - nodes).max() > 1e-2      # (the run trained)


@pytest.mark.parametrize("metric", METRICS)
def test_two_shards_in_one_process(gpu, metric):
    """The multi-rank path without a second process: two kernel sets over the halves of the rows, ring(g) of both summed on
    the device after every step and written to both; each shard deals ITS rows into the phases."""
    from ark_analysis_amd import distributed
    x, nodes, xdim, ydim, sched, passes, rr = _run_inputs("3000x7_4x3")
    shards = [x[:1400], x[1400:]]
    q = mbr.run_quantum(shards, sched)
    want = mbr.som_batch(shards, nodes, xdim, ydim, passes, sched, ALPHA, rr, metric, quantum=q)
    kerns = [distributed.HipKernels(metric=metric) for _ in shards]
    xs = [torch.from_numpy(s).to(gpu) for s in shards]
    w = torch.from_numpy(nodes).to(gpu)
    for kern, xd in zip(kerns, xs):
        kern.begin(xd, w, xdim, ydim, sched, quantum=q)
    total = passes * sched
    for g in range(total):
        for kern, xd in zip(kerns, xs):
            kern.steps(xd, g, g + 1, total, ALPHA, rr)
        both = kerns[0].ring(g) + kerns[1].ring(g)
        for kern in kerns:
            kern.ring(g).copy_(both)
    outs = []
    for kern in kerns:
        out = torch.empty_like(w)
        kern.finish(total, total, ALPHA, rr, out)
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(outs[0], want)
    np.testing.assert_array_equal(outs[1], want)


def test_a_communicator_is_refused_under_a_metric(gpu):
    from ark_analysis_amd import som_device
    x = torch.zeros((64, 3), dtype=torch.float64, device=gpu)
    state = som_device.BatchTrainState(64, 3, 2, 2, 2, gpu, metric=3)
    assert state.metric == 3 and not state.fits(64, 3, 2, 2, 2) and state.fits(64, 3, 2, 2, 2, metric=3)
    with pytest.raises(ValueError, match="exchange"):
        som_device.batch_train_steps(x, state, 0, 2, 2, ALPHA, (1.0, 0.0), comm=object())


# ---- front end and pipeline ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_som_batch_front_end(gpu, metric):
    from ark_analysis_amd import flowsom
    x, nodes, xdim, ydim, sched, passes, rr = _run_inputs("3000x7_4x3")
    got = flowsom.som_batch(x, xdim=xdim, ydim=ydim, rlen=passes, nodes=nodes, batch_steps=sched, distf=metric)
    np.testing.assert_array_equal(got, _reference_run("3000x7_4x3", metric))


def test_label_table_under_cosine(gpu):
    """labels of metric_reference, totals equal to cluster_sums of them (integer rows over power-of-two norms: exact sums)."""
    import pandas as pd
    import pyarrow as pa

    from ark_analysis_amd import arrow_assign
    chans = ["a", "b", "c", "d"]
    rng = np.random.RandomState(2)
    raw = np.floor(mbr.test_rows(3000, 4, 17) * 4.0)
    raw[10] = 0.0
    table = pa.table({**{ch: raw[:, j] for j, ch in enumerate(chans)}, "fov": ["fov0"] * 3000})
    norm = np.array([2.0, 4.0, 0.5, 1.0])

    class Som:
        distf = 4
        weights = pd.DataFrame(rng.gamma(2.0, 1.0, size=(9, 4)), columns=chans)
        norm_data = pd.DataFrame(norm[None, :], columns=chans)
        som_clusters_seen = set()

    som = Som()
    assert arrow_assign.applicable(som, table, True)
    out, release, totals = arrow_assign.label_table(som, table, normalize=True, blocks=arrow_assign.HostBlocks())
    rows = raw / norm
    labels_ref, _ = mr.map_data_to_nodes(som.weights.to_numpy(), rows, 4)
    assert (labels_ref == 0).sum() >= 1 and (labels_ref == 0).mean() < 0.05
    np.testing.assert_array_equal(out.column("pixel_som_cluster").to_numpy(), labels_ref)
    s, cnt = ob.cluster_sums(rows, labels_ref, 9)
    assert totals[0] == tuple(chans)
    np.testing.assert_array_equal(totals[1], s)
    np.testing.assert_array_equal(totals[2], cnt)
    assert totals[2].dtype == np.int64
    assert som.som_clusters_seen == set((np.flatnonzero(cnt) + 1).tolist())
    release()
    som.som_clusters_seen = set()
    plain = arrow_assign.label_table(som, table, normalize=True)
    assert som.som_clusters_seen == set((np.flatnonzero(cnt) + 1).tolist())      # (label 0 is no cluster in either call form)
    np.testing.assert_array_equal(plain.column("pixel_som_cluster").to_numpy(), labels_ref)
