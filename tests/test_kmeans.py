"""K19 on the CPU: the interface (the ``kmeans=`` keyword of the six public functions, the new names, the ABI), the numpy
statement of tests/kmeans_reference.py against scikit-learn's KMeans in quality, the rule's details on hand-built inputs,
and the host logic of ``kmeans="device"`` with the device entry points swapped for the statements.

What is pinned: the device path equals the statement (tests/test_gpu_kmeans.py).  Against scikit-learn only the quality is
compared: kmeans_plusplus carried through one RandomState per k is this project's reading of how KMeans draws its inits,
and scikit-learn forms its distances through a matrix product in another rounding order.

The inertia margin (measured with scikit-learn 1.7.2 on freq_matrix(), k = 2 .. 10, best of 10 restarts, seeds 0, 1, 42): the
statement's inertia over scikit-learn's was 1 + 2.2e-16, 1, 1 + 6.7e-16 at its largest per seed (RATIO_SEEN); scikit-learn
against itself across those seeds moves by up to 1.00852 (k = 8), which is what another draw of the inits does to a
best-of-10 on this input, so the margin for the init-drawing difference is MARGIN = 0.01 and scikit-learn alone stays
inside it."""
import inspect
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

from tests import kmeans_reference as kr
from tests import silhouette_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 42)
RATIO_SEEN = 1.0 + 6.7e-16
MARGIN = 0.01
TOL, MAX_ITER = 1e-4, 300
_CACHE = {}


# ---- inputs (shared with tests/test_gpu_kmeans.py) ------------------------------------------------------------------
BLOB_CENTRES = np.array([[0, 0, 0, 0, 0], [20, 0, 0, 0, 0], [0, 20, 0, 0, 0], [0, 0, 20, 0, 0], [0, 0, 0, 20, 0],
                         [20, 20, 20, 20, 20]], dtype=np.float64)


def blobs():
    """600 integer-valued rows in 5 columns: 6 blobs, centres 20 or more apart, spread at most 2; and the blob of a row."""
    rs = np.random.RandomState(0)
    truth = np.repeat(np.arange(6), 100)
    x = BLOB_CENTRES[truth] + rs.randint(-2, 3, size=(600, 5))
    order = rs.permutation(600)
    return x[order], truth[order]


def freq_matrix():
    """900 rows of counts divided by their sum, 8 columns: five neighbourhood archetypes."""
    rs = np.random.RandomState(5)
    arche = rs.choice([0.3, 2.0, 9.0], size=(5, 8))
    counts = rs.poisson(arche[rs.randint(0, 5, 900)]).astype(np.float64)
    counts[counts.sum(axis=1) == 0, 0] = 1
    return counts / counts.sum(axis=1, keepdims=True)


def counts_matrix(n, d, seed):
    """Integer-valued rows, what a neighbour-count matrix holds."""
    rs = np.random.RandomState(seed)
    arche = rs.choice([0.5, 3.0, 8.0], size=(4, d))
    return rs.poisson(arche[rs.randint(0, 4, n)]).astype(np.float64)


def rows_as_inits(x, k, seed):
    """k rows of x, distinct where x has k distinct rows."""
    rs = np.random.RandomState(seed)
    uniq = np.unique(x, axis=0)
    if len(uniq) >= k:
        return np.ascontiguousarray(uniq[rs.choice(len(uniq), k, replace=False)])
    return np.ascontiguousarray(x[rs.choice(len(x), k, replace=False)])


def tolerance(x):
    return TOL * float(np.mean(np.var(x, axis=0)))


# hand-built inputs: (rows, initial centres)
TIE = (np.array([[-1.0, 0], [1, 0], [-1, 0], [1, 0], [0, 3], [0, -3]]), np.array([[-1.0, 0], [1, 0]]))
ONE_EMPTY = (np.array([[0.0, 0], [0, 0], [0, 0], [10, 0], [10, 0], [4, 0]]), np.array([[0.0, 0], [0, 0], [10, 0]]))
TWO_EMPTY = (ONE_EMPTY[0], np.zeros((3, 2)))


def slow_and_quick():
    """On the centred frequency matrix: an init that needs 15 iterations and one that settles at iteration 2 (the
    converged centres of the first, nudged: the labels of iteration 1 are already the final ones)."""
    if "sq" not in _CACHE:
        from sklearn.cluster import kmeans_plusplus
        f = freq_matrix()
        x = f - f.mean(axis=0)
        slow = kmeans_plusplus(x, 6, random_state=np.random.RandomState(3))[0]
        done = kr.lloyd(x, slow, tolerance(f), MAX_ITER)
        quick = done[1] + 1e-6
        _CACHE["sq"] = (x, slow, quick, tolerance(f))
    return _CACHE["sq"]


def same_partition(a, b, k):
    """Equal up to a renaming of the clusters: the contingency table has one non-zero entry per row and per column."""
    table = np.zeros((k, k), dtype=np.int64)
    np.add.at(table, (np.asarray(a), np.asarray(b)), 1)
    return bool(((table > 0).sum(axis=0) == 1).all() and ((table > 0).sum(axis=1) == 1).all())


def cell_table(n_per_fov=(300, 310, 290), seed=11):
    """(all_data, neighbourhood matrix) of three FOVs, about 900 cells."""
    from tests import test_silhouette as ts
    mat = ts.neighborhood_matrix(n_per_fov, seed)
    rs = np.random.RandomState(seed)
    table = pd.DataFrame({"cell_size": rs.randint(20, 90, len(mat)), "chanA": rs.uniform(0, 1, len(mat)),
                          "chanB": rs.uniform(0, 1, len(mat)), "label": mat["label"].to_numpy(),
                          "fov": mat["fov"].to_numpy(), "cell_meta_cluster": mat["cell_meta_cluster"].to_numpy()})
    return table, mat


@pytest.fixture
def stand_ins(monkeypatch):
    """The two device entry points of spatial_analysis_utils swapped for the numpy statements; the calls are recorded."""
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    calls = {"kmeans": [], "silhouette": []}

    def lloyd(x, inits, tol, max_iter):
        calls["kmeans"].append((np.array(x), [np.array(c) for c in inits], tol, max_iter))
        return kr.host_stand_in(x, inits, tol, max_iter)

    def silhouette(x, labelings, n_clusters):
        calls["silhouette"].append((np.array(x), np.array(labelings), list(n_clusters)))
        return sr.host_stand_in(x, labelings, n_clusters)
    monkeypatch.setattr(sau, "_kmeans_lloyd_device", lloyd)
    monkeypatch.setattr(sau, "_silhouette_device", silhouette)
    return calls


def _six():
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    return [sau.generate_cluster_labels, sau.compute_kmeans_inertia, sau.compute_kmeans_silhouette,
            na.generate_cluster_matrix_results, na.compute_cluster_metrics_inertia, na.compute_cluster_metrics_silhouette]


# ---- interface ------------------------------------------------------------------------------------------------------
def test_new_names_and_keyword_exist():
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    assert callable(som_device.kmeans_lloyd) and callable(sau.kmeans_fits_device)
    assert list(inspect.signature(som_device.kmeans_lloyd).parameters)[:4] == ["rows", "inits", "tol", "max_iter"]
    assert list(inspect.signature(sau.kmeans_fits_device).parameters) == ["values", "ks", "seed", "n_init"]
    for fn in _six():
        par = inspect.signature(fn).parameters["kmeans"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == "host", fn.__name__
    header = open(os.path.join(ROOT, "include", "pxsom.h")).read()
    lib = _capi.lib()
    for name in ("pxsom_kmeans_lloyd", "pxsom_kmeans_workspace_bytes", "pxsom_kmeans_group_count"):
        assert name in _capi.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\(" % name, header), name
    assert lib.pxsom_abi_version() == _capi.ABI_VERSION == 9
    assert som_device.KMEANS_MAX_D == 64 and som_device.KMEANS_MAX_K == 32


def test_bad_kmeans_value_raises(stand_ins):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    table, mat = cell_table((40, 30, 30))
    data = mat.drop(["fov", "label", "cell_meta_cluster"], axis=1)
    for bad in ("gpu", "Device", None, 1):
        for call in (lambda: sau.generate_cluster_labels(data, 3, kmeans=bad),
                     lambda: sau.compute_kmeans_inertia(data, max_k=3, kmeans=bad),
                     lambda: sau.compute_kmeans_silhouette(data, max_k=3, kmeans=bad),
                     lambda: na.generate_cluster_matrix_results(table, mat, 3, kmeans=bad),
                     lambda: na.compute_cluster_metrics_inertia(mat, max_k=3, kmeans=bad),
                     lambda: na.compute_cluster_metrics_silhouette(mat, max_k=3, kmeans=bad)):
            with pytest.raises(ValueError, match="'host' or 'device'"):
                call()
    assert stand_ins == {"kmeans": [], "silhouette": []}
    with pytest.raises(TypeError):
        sau.generate_cluster_labels(data, 3, 42, "device")          # keyword-only


def test_host_is_the_parent_route_with_torch_blocked(stand_ins, monkeypatch):
    """kmeans="host", spelled out or left to the default, with ``import torch`` failing: every fit is the parent's
    KMeans call and every result is read from those fits; the k-means statement is never asked."""
    import sklearn.cluster
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    monkeypatch.setitem(sys.modules, "torch", None)
    with pytest.raises(ImportError):
        import torch  # noqa: F401
    made, real = [], sklearn.cluster.KMeans

    def recorded(*args, **kwargs):
        made.append((real(*args, **kwargs), args, kwargs))
        return made[-1][0]
    monkeypatch.setattr(sklearn.cluster, "KMeans", recorded)
    table, mat = cell_table((70, 60, 50))
    data = mat.drop(["fov", "label", "cell_meta_cluster"], axis=1)
    sweep = [((), dict(n_clusters=k, random_state=9, n_init="auto")) for k in (2, 3, 4)]
    for route in ({}, {"kmeans": "host"}):
        del made[:]
        labels = sau.generate_cluster_labels(data, 4, seed=9, **route)
        assert [(a, kw) for _, a, kw in made] == [((), dict(n_clusters=4, random_state=9, n_init=10))]
        np.testing.assert_array_equal(labels, made[0][0].labels_ + 1)
        assert labels.min() == 1 and labels.max() == 4

        del made[:]
        frames = na.generate_cluster_matrix_results(table, mat, 4, seed=9, **route)
        assert [(a, kw) for _, a, kw in made] == [((), dict(n_clusters=4, random_state=9, n_init=10))]
        merged = frames[0].merge(mat[["fov", "label"]].assign(want=made[0][0].labels_ + 1), on=["fov", "label"])
        np.testing.assert_array_equal(merged["kmeans_neighborhood"], merged["want"])

        for fn, frame in ((sau.compute_kmeans_inertia, data), (na.compute_cluster_metrics_inertia, mat)):
            del made[:]
            series = fn(frame, min_k=2, max_k=4, seed=9, **route)
            assert [(a, kw) for _, a, kw in made] == sweep
            np.testing.assert_array_equal(series.values, [fit.inertia_ for fit, _, _ in made])

        for fn, frame in ((sau.compute_kmeans_silhouette, data), (na.compute_cluster_metrics_silhouette, mat)):
            del made[:]
            del stand_ins["silhouette"][:]
            series = fn(frame, min_k=2, max_k=4, seed=9, **route)
            assert [(a, kw) for _, a, kw in made] == sweep
            (x, labelings, ks), = stand_ins["silhouette"]
            np.testing.assert_array_equal(labelings, np.stack([fit.labels_ for fit, _, _ in made]))
            np.testing.assert_array_equal(series.values, sr.host_stand_in(x, labelings, ks))
    assert stand_ins["kmeans"] == []


def test_limits_are_value_errors_before_any_launch():
    """Host tensors: the size checks come before anything touches a device."""
    import torch
    from ark_analysis_amd import som_device
    x = torch.zeros((10, 5), dtype=torch.float64)
    with pytest.raises(ValueError, match="64"):
        som_device.kmeans_lloyd(torch.zeros((10, 65), dtype=torch.float64), [np.zeros((2, 65))], 0.0, 10)
    with pytest.raises(ValueError, match="32"):
        som_device.kmeans_lloyd(torch.zeros((40, 5), dtype=torch.float64), [np.zeros((33, 5))], 0.0, 10)
    with pytest.raises(ValueError, match="exceeds"):
        som_device.kmeans_lloyd(x, [np.zeros((2, 5)), np.zeros((11, 5))], 0.0, 10)
    with pytest.raises(ValueError, match="float64"):
        som_device.kmeans_lloyd(x.float(), [np.zeros((2, 5))], 0.0, 10)
    with pytest.raises(ValueError, match="inits"):
        som_device.kmeans_lloyd(x, [np.zeros((2, 4))], 0.0, 10)
    with pytest.raises(ValueError, match="max_iter"):
        som_device.kmeans_lloyd(x, [np.zeros((2, 5))], 0.0, 0)
    with pytest.raises(ValueError, match="tol"):
        som_device.kmeans_lloyd(x, [np.zeros((2, 5))], -1.0, 10)
    with pytest.raises(ValueError, match="HBM"):
        som_device.kmeans_lloyd(x, [np.zeros((2, 5))], 0.0, 10)


def test_entry_point_checks_and_the_grouping_rule():
    from ark_analysis_amd import _capi, som_device
    lib = _capi.lib()
    one = 8           # any non-null address: the checks come first and nothing is dereferenced
    ks = np.array([3, 2], dtype=np.int32)
    tol, iters = np.zeros(2), np.array([5, 5], dtype=np.int32)
    inertia, n_iter = np.ones(2), np.ones(2, dtype=np.int32)
    tail = (tol.ctypes.data, iters.ctypes.data, one, inertia.ctypes.data, n_iter.ctypes.data, one, 1 << 30, 0, None)
    for n, d, k0, what in ((10, 65, 3, b"64"), (10, 0, 3, b"64"), (10, 5, 33, b"32"), (10, 5, 0, b"32"), (2, 5, 3, b"exceeds")):
        ks[0] = k0
        assert lib.pxsom_kmeans_lloyd(one, n, d, 2, ks.ctypes.data, one, *tail) == -1
        assert what in lib.pxsom_last_error()
    ks[0] = 3
    assert lib.pxsom_kmeans_lloyd(one, 10, 5, 2, ks.ctypes.data, one, *tail[:5], one, 16, 0, None) == -3     # workspace
    assert lib.pxsom_kmeans_lloyd(one, 0, 5, 2, ks.ctypes.data, one, *tail) == 0             # n = 0 returns at once
    assert (inertia == 0).all() and (n_iter == 0).all()
    assert lib.pxsom_kmeans_workspace_bytes(1000, 5, 2, ks.ctypes.data) >= 2 * 1000 * 8 + 4 * 5 * 6 * 8
    assert lib.pxsom_kmeans_workspace_bytes(1000, 65, 2, ks.ctypes.data) == 0
    # the LDS rule of csrc/pxsom_kmeans.hip: 16864 bytes per problem at k = 32, d = 64, 65536 per group
    assert som_device.kmeans_group_count(64, [32] * 10) == 4
    assert som_device.kmeans_group_count(64, [32] * 3) == 1
    assert som_device.kmeans_group_count(20, range(2, 11)) == 1
    assert som_device.kmeans_group_count(20, [10] * 10) == 1
    assert som_device.kmeans_group_count(1, [1] * 33) == 2              # at most 32 problems share a group


def test_group_count_equals_the_python_rule_on_seeded_draws():
    """pxsom_kmeans_group_count against the rule restated in tests/kmeans_edge_cases.py: lists on both sides of the
    32-problem limit, lists that sit on the byte budget, and 300 seeded (d, k list) draws of up to 70 problems."""
    from ark_analysis_amd import som_device
    from tests import kmeans_edge_cases as ec
    for count in (31, 32, 33, 63, 64, 65, 70):              # the limit alone: 32 of them are 10432 bytes
        assert som_device.kmeans_group_count(1, [1] * count) == len(ec.groups(1, [1] * count)) == -(-count // 32)
    # the bytes alone, one centre either side of the budget (no d and k list fill 65536 to the byte)
    assert ec.group_bytes(124, 4, 64) == 65384 and ec.group_bytes(125, 4, 64) == 65902
    assert som_device.kmeans_group_count(64, [32, 32, 32, 28]) == len(ec.groups(64, [32, 32, 32, 28])) == 1
    assert som_device.kmeans_group_count(64, [32, 32, 32, 29]) == len(ec.groups(64, [32, 32, 32, 29])) == 2
    rs = np.random.RandomState(19)
    seen = set()
    for draw in range(300):
        d = int(rs.choice([1, 3, 4, 5, 17, 32, 33, 60, 61, 64]))
        count = int(rs.randint(1, 71))
        top = int(rs.choice([1, 2, 8, 32]))                 # small k: the problem limit closes; large k: the bytes do
        ks = rs.randint(1, top + 1, size=count).tolist()
        want = ec.groups(d, ks)
        assert som_device.kmeans_group_count(d, ks) == len(want), (d, ks)
        assert sorted(p for g in want for p in g) == list(range(count))
        for g, nxt in zip(want, want[1:]):
            fits = ec.group_bytes(sum(ks[p] for p in g) + ks[nxt[0]], len(g) + 1, d) <= ec.LDS_BUDGET
            assert not fits or len(g) == ec.MAX_GROUP
            seen.add("limit" if fits else "bytes")
        seen.add("one" if len(want) == 1 else "several")
    assert seen == {"limit", "bytes", "one", "several"}    # the draws close groups both ways, and leave some whole


def test_device_entry_point_is_loud_without_gpu():
    import torch
    if torch.cuda.is_available():
        return          # nothing to refuse where a HIP device is visible
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    with pytest.raises(RuntimeError, match="no HIP device"):
        sau._kmeans_lloyd_device(np.zeros((4, 2)), [np.zeros((2, 2))], 0.0, 10)
    with pytest.raises(RuntimeError, match="no HIP device"):
        sau.generate_cluster_labels(pd.DataFrame(counts_matrix(30, 4, 1)), 3, kmeans="device")


# ---- the statement against scikit-learn -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_init", ["auto", 10])
@pytest.mark.parametrize("seed", SEEDS)
def test_statement_finds_sklearns_partition_of_the_blobs(seed, n_init):
    from sklearn.cluster import KMeans
    x, truth = blobs()
    apart = np.sqrt(((BLOB_CENTRES[:, None, :] - BLOB_CENTRES[None, :, :]) ** 2).sum(axis=2))
    assert apart[~np.eye(6, dtype=bool)].min() >= 20 and np.abs(x - BLOB_CENTRES[truth]).max() <= 2
    assert (x == np.round(x)).all() and x.shape == (600, 5)
    labels, inertia, centres = kr.fits(x, [6], seed, n_init)[0]
    fit = KMeans(n_clusters=6, random_state=seed, n_init=n_init).fit(x)
    assert same_partition(labels, fit.labels_, 6) and same_partition(labels, truth, 6)
    np.testing.assert_allclose(inertia, fit.inertia_, rtol=1e-12)
    assert not same_partition(labels, np.roll(labels, 1), 6)            # the comparison can fail


def test_statement_inertia_against_sklearn_on_frequencies():
    from sklearn.cluster import KMeans
    f, ks = freq_matrix(), list(range(2, 11))
    np.testing.assert_allclose(f.sum(axis=1), 1.0, rtol=1e-12)
    theirs = {}
    for seed in SEEDS:
        mine = np.array([inertia for _, inertia, _ in kr.fits(f, ks, seed, 10)])
        theirs[seed] = np.array([KMeans(n_clusters=k, random_state=seed, n_init=10).fit(f).inertia_ for k in ks])
        ratio = mine / theirs[seed]
        print("seed %d: statement / sklearn per k = %s, largest %.17g" % (seed, np.round(ratio, 6), ratio.max()))
        assert ratio.max() < RATIO_SEEN + MARGIN
    table = np.stack([theirs[s] for s in SEEDS])
    spread = (table.max(axis=0) / table.min(axis=0)).max()
    print("sklearn against itself across the seeds: %.6f" % spread)
    assert spread - 1 < MARGIN            # else the input is too ragged for the comparison


# ---- the rule on hand-built inputs ----------------------------------------------------------------------------------
def test_equidistant_row_goes_to_the_lower_index():
    x, init = TIE
    trace = []
    labels, centres, inertia, n_iter, why = kr.lloyd(x, init, 0.0, MAX_ITER, trace)
    assert (kr.sq_dists(x[4:], init) == 10).all()                   # both rows tie in iteration 1
    assert list(trace[0][0]) == [0, 1, 0, 1, 0, 0] and list(labels) == [0, 1, 0, 1, 0, 0]
    assert (n_iter, why) == (2, "labels")
    np.testing.assert_array_equal(centres, [[-0.5, 0], [1, 0]])
    assert inertia == 2 * 0.25 + 2 * (0.25 + 9)


def test_duplicate_rows_leave_a_centre_empty_and_it_is_relocated():
    x, init = ONE_EMPTY
    trace = []
    labels, centres, inertia, n_iter, why = kr.lloyd(x, init, 0.0, MAX_ITER, trace)
    assert list(trace[0][0]) == [0, 0, 0, 2, 2, 0] and trace[0][1] == 1 and trace[0][2] == 16.0
    np.testing.assert_array_equal(centres, [[0, 0], [4, 0], [10, 0]])          # the farthest row, (4, 0), became centre 1
    assert list(labels) == [0, 0, 0, 2, 2, 1] and inertia == 0 and (n_iter, why) == (2, "tol")
    x, init = TWO_EMPTY
    trace = []
    kr.lloyd(x, init, 0.0, 1, trace)
    assert trace[0][1] == 2 and list(kr.farthest_rows(kr.assign(x, init)[1], 2)) == [3, 4]     # a tie: the lower row first
    labels, centres, _, _, _ = kr.lloyd(x, init, 0.0, 1)
    np.testing.assert_array_equal(centres, [[1, 0], [10, 0], [10, 0]])
    assert list(labels) == [0, 0, 0, 1, 1, 0]


def test_the_three_ways_to_stop():
    x, slow, quick, tol = slow_and_quick()
    labels, centres, inertia, n_iter, why = kr.lloyd(x, slow, tol, MAX_ITER)
    assert (n_iter, why) == (15, "labels")
    assert kr.lloyd(x, quick, 0.0, MAX_ITER)[3:] == (2, "labels")
    loose = kr.lloyd(x, slow, 1e9, MAX_ITER)
    assert loose[3:] == (1, "tol")
    for got in (loose, kr.lloyd(x, slow, 0.0, 2)):
        again, best, _ = kr.assign(x, got[1])                     # the closing pass: labels of the returned centres
        np.testing.assert_array_equal(got[0], again)
        assert got[2] == kr.block_inertia(best)
    assert kr.lloyd(x, slow, 0.0, 2)[3:] == (2, "max_iter")
    assert not np.array_equal(kr.lloyd(x, slow, 0.0, 2)[0], kr.assign(x, slow)[0])


# ---- kmeans="device" through the statements -------------------------------------------------------------------------
def test_kmeans_fits_device_host_logic(stand_ins):
    from sklearn.cluster import kmeans_plusplus
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    x = counts_matrix(300, 6, 2)
    fits = sau.kmeans_fits_device(pd.DataFrame(x), [2, 4], seed=7, n_init=3)
    (rows, inits, tol, max_iter), = stand_ins["kmeans"]                  # every (k, restart) in one call
    mean = x.mean(axis=0)
    np.testing.assert_array_equal(rows, x - mean)
    assert tol == tolerance(x) and max_iter == 300 and [len(c) for c in inits] == [2, 2, 2, 4, 4, 4]
    for k, at in ((2, 0), (4, 3)):
        rs = np.random.RandomState(7)
        for r in range(3):                                               # one RandomState per k, carried on
            np.testing.assert_array_equal(inits[at + r], kmeans_plusplus(x - mean, k, random_state=rs)[0])
    for fit, k, at in zip(fits, (2, 4), (0, 3)):
        runs = [kr.lloyd(x - mean, inits[at + r], tol, 300) for r in range(3)]
        best = int(np.argmin([r[2] for r in runs]))
        assert fit.labels_.dtype == np.int32 and fit.inertia_ == runs[best][2]
        np.testing.assert_array_equal(fit.labels_, runs[best][0])
        np.testing.assert_array_equal(fit.cluster_centers_, runs[best][1] + mean)
    assert len(sau.kmeans_fits_device(x, [3], seed=7, n_init="auto")) == 1 and len(stand_ins["kmeans"][-1][1]) == 1
    holed = x.copy()
    for bad in (np.nan, np.inf):
        holed[5, 2] = bad
        before = len(stand_ins["kmeans"])
        with pytest.raises(ValueError, match="NaN or infinite"):
            sau.kmeans_fits_device(holed, [2])
        with pytest.raises(ValueError, match="NaN or infinite"):
            sau.generate_cluster_labels(pd.DataFrame(holed), 2, kmeans="device")
        assert len(stand_ins["kmeans"]) == before                        # on the host, before any launch
    with pytest.raises(ValueError, match="n_clusters"):
        sau.kmeans_fits_device(x[:3], [4])
    assert sau.kmeans_fits_device(np.zeros((0, 6)), [2])[0].labels_.shape == (0,)


def test_ties_between_restarts_keep_the_first(monkeypatch):
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau

    def equal_inertia(x, inits, tol, max_iter):
        labels = np.stack([np.full(len(x), p, dtype=np.int32) for p in range(len(inits))])
        return labels, [np.array(c) for c in inits], np.array([5.0, 3.0, 3.0, 4.0]), np.ones(4, np.int32)
    monkeypatch.setattr(sau, "_kmeans_lloyd_device", equal_inertia)
    fit, = sau.kmeans_fits_device(counts_matrix(50, 3, 1), [2], seed=1, n_init=4)
    assert (fit.labels_ == 1).all() and fit.inertia_ == 3.0


def test_public_functions_on_the_device_route(stand_ins):
    """The six functions with kmeans="device" (the statements in the device's place): one k-means call each, with the
    sweep's 9 fits or the labelling's 10 restarts in it; shapes, labels 1 .. k, and the silhouette of those labels."""
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    from tests import test_silhouette as ts
    table, mat = cell_table((110, 100, 90))
    data = mat.drop(["fov", "label", "cell_meta_cluster"], axis=1)
    labels = sau.generate_cluster_labels(data, 4, seed=3, kmeans="device")
    assert [len(c) for c in stand_ins["kmeans"][-1][1]] == [4] * 10 and len(stand_ins["kmeans"]) == 1
    assert labels.shape == (300,) and set(labels) == {1, 2, 3, 4}
    frames = na.generate_cluster_matrix_results(table, mat, 4, seed=3, kmeans="device")
    assert len(stand_ins["kmeans"]) == 2 and len(frames[0]) == 300
    merged = frames[0].merge(mat[["fov", "label"]].assign(want=labels), on=["fov", "label"])
    np.testing.assert_array_equal(merged["kmeans_neighborhood"], merged["want"])
    assert list(frames[1].index) == list(frames[2].index) == ["Cluster%d" % c for c in (1, 2, 3, 4)]
    assert list(frames[2].columns) == ["chanA", "chanB"]

    inertia = na.compute_cluster_metrics_inertia(mat, seed=3, kmeans="device")
    ts._check_series(inertia, 2, 10)
    assert len(stand_ins["kmeans"]) == 3 and [len(c) for c in stand_ins["kmeans"][-1][1]] == list(range(2, 11))
    want = kr.fits(data, range(2, 11), 3, "auto")
    np.testing.assert_array_equal(inertia.values, [i for _, i, _ in want])
    assert (np.diff(inertia.values) < 0).all()
    np.testing.assert_array_equal(sau.compute_kmeans_inertia(data, seed=3, kmeans="device").values, inertia.values)

    del stand_ins["silhouette"][:]
    scores = na.compute_cluster_metrics_silhouette(mat, max_k=5, seed=3, kmeans="device")
    ts._check_series(scores, 2, 5)
    (x, labelings, ks), = stand_ins["silhouette"]
    np.testing.assert_array_equal(labelings, np.stack([lab for lab, _, _ in want[:4]]))
    assert ks == [2, 3, 4, 5]
    np.testing.assert_array_equal(scores.values, sr.host_stand_in(data.to_numpy(), labelings, ks))
    sub = sau.compute_kmeans_silhouette(data, max_k=3, seed=3, subsample=20, kmeans="device")
    ts._check_series(sub, 2, 3)
    assert len(stand_ins["silhouette"]) == 3                              # one call per k under subsample, as on the host
