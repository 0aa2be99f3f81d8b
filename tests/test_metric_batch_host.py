"""Batch training and the pipeline under FlowSOM's distf 1 / 3 / 4 (K6m): the ABI additions, every refusal of the two new
entries (no device needed: they come before any HIP call), and the host logic on the reference loop's stand-in."""
import ctypes
import os
import pickle
import re

import numpy as np
import pandas as pd
import pytest

from tests import metric_batch_reference as mbr
from tests import metric_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pxsom_metric_step_workspace_bytes", "pxsom_assign_sums_metric", "pxsom_batch_train_sched_metric_workspace_bytes",
       "pxsom_batch_train_sched_metric")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x1000      # a non-null pointer no refusal path dereferences


def test_new_symbols_are_declared_bound_and_exported():
    from ark_analysis_amd import _build, _capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pxsom.h")).read(), flags=re.S)
    lib = _capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS and hasattr(lib, name)
    assert lib.pxsom_abi_version() == 9
    assert "pxsom_metric_step.hip" in _build.SOURCES and "pxsom_metric_bmu.h" in _build.HEADERS


def _assign(lib, n=10, c=4, ldx=4, dtype=0, k=6, window=(1, 0, 1), labels=P, stats=P, q=0.0, ws=P, ws_bytes=None, metric=1, x=P,
            w=P):
    if ws_bytes is None:
        ws_bytes = lib.pxsom_metric_step_workspace_bytes(c, k, metric) or (1 << 20)
    return lib.pxsom_assign_sums_metric(x, n, c, ldx, dtype, w, k, window[0], window[1], window[2], labels, stats, q, ws, ws_bytes,
                                        metric, None)


def test_assign_sums_metric_refusals():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    err = lib.pxsom_last_error
    assert lib.pxsom_metric_step_workspace_bytes(4, 6, 1) == lib.pxsom_assign_metric_workspace_bytes(10, 4, 6, 1) > 0
    for args in ((4, 6, 0), (4, 6, 2), (4, 6, 5), (0, 6, 1), (4, 0, 1), (4, 1025, 3), (1025, 6, 4)):
        assert lib.pxsom_metric_step_workspace_bytes(*args) == 0, args
    # the metric comes first: with every other argument bad as well (nothing else is looked at, no HIP call is made)
    for bad in (0, 5, -1, 77):
        assert lib.pxsom_assign_sums_metric(None, -1, 0, 0, 9, None, 0, 0, 0, 0, None, None, -1.0, None, 0, bad, None) == INVALID
        assert b"unknown metric" in err()
    assert lib.pxsom_assign_sums_metric(None, -1, 0, 0, 9, None, 0, 0, 0, 0, None, None, -1.0, None, 0, 2, None) == UNSUPPORTED
    assert b"pxsom_assign_sums" in err() and b"pxsom_batch_accumulate" in err()
    # then the order and words of pxsom_assign_metric
    assert _assign(lib, n=-1) == INVALID and b"n=-1 outside [0, 2^31)" in err()
    assert _assign(lib, n=1 << 31) == INVALID and b"outside [0, 2^31)" in err()
    assert _assign(lib, c=0, ldx=4) == UNSUPPORTED and b"c=0 outside" in err()
    assert _assign(lib, c=1025, ldx=1025) == UNSUPPORTED and b"c=1025 outside" in err()
    assert _assign(lib, k=0) == UNSUPPORTED and b"k=0 outside" in err()
    assert _assign(lib, k=1025) == UNSUPPORTED and b"k=1025 outside" in err()
    assert _assign(lib, ldx=3) == INVALID and b"ldx=3 < c=4" in err()
    assert _assign(lib, dtype=7) == UNSUPPORTED and b"dtype 7" in err()
    for kw in (dict(w=None), dict(stats=None), dict(x=None)):
        assert _assign(lib, **kw) == INVALID and b"null pointer" in err(), kw
    for window in ((0, 0, 0), (4, -1, 2), (4, 2, 2), (4, 3, 2), (4, 0, 5), (-3, 0, 1)):
        assert _assign(lib, window=window) == INVALID and b"window" in err(), window
    for q in (3.0, -0.5, float("nan"), float("inf"), 0.75):
        assert _assign(lib, q=q) == INVALID and b"power of two" in err(), q
    need = lib.pxsom_metric_step_workspace_bytes(4, 6, 1)
    assert _assign(lib, ws_bytes=need - 1) == WORKSPACE and b"workspace" in err()
    assert _assign(lib, ws=None) == WORKSPACE
    # nothing to do: success before anything is touched (the pointers are not real)
    assert _assign(lib, n=0, x=None, labels=None) == 0
    assert _assign(lib, n=5, window=(960, 959, 960), q=0.25) == 0


def _sched(lib, metric=1, comm=None, n=10, c=4, ldx=4, dtype=1, xdim=2, ydim=3, phases=2, edges=(0, 1, 2), g=(0, 2), passes=1, q=0.0,
           ws=P, ws_bytes=1 << 20, wbuf=P, ring=P):
    e = np.asarray(edges, dtype=np.int32)
    return lib.pxsom_batch_train_sched_metric(P, n, c, ldx, dtype, None, wbuf, ring, xdim, ydim, phases, e.ctypes.data, len(e) - 1, g[0],
                                              g[1], passes, 0.05, 0.01, 2.0, 0.0, q, ws, ws_bytes, 0, comm, metric, None)


def test_batch_train_sched_metric_refusals():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    err = lib.pxsom_last_error
    for bad in (0, 5, -2):
        assert _sched(lib, metric=bad, n=-1, c=0) == INVALID and b"unknown metric" in err()
    assert _sched(lib, metric=2, n=-1) == UNSUPPORTED and b"pxsom_batch_train_sched_from" in err()
    assert _sched(lib, comm=P) == UNSUPPORTED and b"exchange" in err()
    assert _sched(lib, n=-1) == INVALID
    assert _sched(lib, c=0) == UNSUPPORTED
    assert _sched(lib, ldx=3) == INVALID
    assert _sched(lib, dtype=5) == UNSUPPORTED
    assert _sched(lib, q=3.0) == INVALID and b"power of two" in err()
    assert _sched(lib, xdim=40, ydim=40) == UNSUPPORTED and b"grid" in err()
    assert _sched(lib, edges=(0, 2, 1)) == INVALID
    assert _sched(lib, edges=(1, 2)) == INVALID
    assert _sched(lib, g=(0, 3)) == INVALID and b"steps [0, 3)" in err()
    assert _sched(lib, wbuf=None) == INVALID and b"null pointer" in err()
    assert _sched(lib, ws_bytes=8) == WORKSPACE
    assert _sched(lib, g=(1, 1)) == 0      # no step asked for
    e = np.asarray((0, 1, 2), dtype=np.int32)
    # the prepared codebook, then the labels of the largest step (5 of 10 rows)
    step = lib.pxsom_metric_step_workspace_bytes(4, 6, 3)
    assert lib.pxsom_batch_train_sched_metric_workspace_bytes(10, 4, 6, 1, 2, e.ctypes.data, 2, 3) == (step + 255) // 256 * 256 + 5 * 4
    assert lib.pxsom_batch_train_sched_metric_workspace_bytes(10, 4, 6, 1, 2, e.ctypes.data, 2, 2) == 0


def test_trainer_and_kernel_set_carry_the_metric():
    from ark_analysis_amd import distributed
    with pytest.raises(ValueError, match="unknown metric"):
        distributed.HipKernels(metric=5)
    kern = distributed.HipKernels(metric=4)
    assert kern.metric == 4 and kern.exchange(None) is None
    tr = distributed.BatchSOMTrainer(2, 2, 3, "cpu", batch_steps=2, kernels=mbr.MetricOracleKernels(3))
    assert tr.metric == 3
    with pytest.raises(ValueError, match="kernel set runs metric"):
        distributed.BatchSOMTrainer(2, 2, 3, "cpu", batch_steps=2, kernels=mbr.MetricOracleKernels(3), metric=4)
    from tests.oracle_backend import OracleKernels      # (no ``metric`` attribute: a Euclidean kernel set)
    assert distributed.BatchSOMTrainer(2, 2, 3, "cpu", batch_steps=2, kernels=OracleKernels()).metric == 2
    with pytest.raises(ValueError, match="kernel set runs metric 2"):
        distributed.BatchSOMTrainer(2, 2, 3, "cpu", batch_steps=2, kernels=OracleKernels(), metric=4)


@pytest.fixture()
def stand_ins(monkeypatch):
    mbr.install(monkeypatch.setattr)


def test_som_batch_refuses_an_unknown_distf(stand_ins):
    from ark_analysis_amd import flowsom
    x = mbr.test_rows(60, 3, 0)
    for bad in (5, 0, True, 2.0):
        with pytest.raises(NotImplementedError, match="distf"):
            flowsom.som_batch(x, xdim=2, ydim=2, batch_steps=2, seed=1, distf=bad)


@pytest.mark.parametrize("distf", [1, 3, 4])
def test_som_batch_under_a_metric_is_the_reference_loop(stand_ins, distf):
    from ark_analysis_amd import flowsom
    x = mbr.test_rows(600, 5, 3)
    x[17] = 0.0
    nodes = x[np.random.RandomState(7).choice(600, 6, replace=False)]
    rr = flowsom.default_radius_range(3, 2)
    # (on host memory the stand-in trains in the caller's array: hand over copies)
    got = flowsom.som_batch(x, xdim=3, ydim=2, rlen=2, nodes=nodes.copy(), batch_steps=4, distf=distf)
    want = mbr.som_batch([x], nodes, 3, 2, 2, 4, (0.05, 0.01), rr, distf, quantum=mbr.run_quantum([x], 4))
    np.testing.assert_array_equal(got, want)
    euclid = flowsom.som_batch(x, xdim=3, ydim=2, rlen=2, nodes=nodes.copy(), batch_steps=4)
    assert np.abs(got - euclid).max() > 1e-3      # (the distance is not ignored)


def _pixel_dirs(tmp_path, chans, n=400):
    from ark_analysis_amd.fov_tables import write_dataframe
    (tmp_path / "sub").mkdir()
    tables = {}
    for i, fov in enumerate(("fov0", "fov1")):
        df = pd.DataFrame(mbr.test_rows(n, len(chans), 10 + i), columns=chans)
        df["fov"], df["row_index"], df["column_index"] = fov, 0, 0
        write_dataframe(df, str(tmp_path / "sub" / (fov + ".feather")))
        tables[fov] = df
    write_dataframe(pd.DataFrame(np.array([[2.0, 4.0, 0.5]]), columns=chans), str(tmp_path / "norm.feather"))
    return tables


def test_pixel_som_cluster_trains_and_labels_under_cosine(stand_ins, tmp_path):
    from ark_analysis_amd import flowsom
    from ark_analysis_amd.phenotyping import cluster_helpers
    chans = ["a", "b", "c"]
    tables = _pixel_dirs(tmp_path, chans)
    som = cluster_helpers.PixelSOMCluster(str(tmp_path / "sub"), str(tmp_path / "norm.feather"), str(tmp_path / "w.feather"),
                                          ["fov0", "fov1"], chans, xdim=2, ydim=2, num_passes=2, seed=5, train_mode="batch",
                                          batch_steps=3, distf=4)
    assert som.distf == 4
    som.train_som()
    rows = som.train_data[chans].to_numpy(dtype=np.float64)
    nodes = rows[np.random.RandomState(5).choice(len(rows), 4, replace=False)]
    want = mbr.som_batch([rows], nodes, 2, 2, 2, 3, (0.05, 0.01), flowsom.default_radius_range(2, 2), 4,
                         quantum=mbr.run_quantum([rows], 3))
    np.testing.assert_array_equal(som.weights.to_numpy(), want)
    out = som.assign_som_clusters(tables["fov1"])
    normed = tables["fov1"][chans].to_numpy() / np.array([2.0, 4.0, 0.5])
    np.testing.assert_array_equal(out["pixel_som_cluster"].to_numpy(), mr.map_data_to_nodes(want, normed, 4)[0])
    again = pickle.loads(pickle.dumps(som))
    assert again.distf == 4 and again.train_mode == "batch"
    with pytest.raises(NotImplementedError, match="distf"):
        cluster_helpers.PixelSOMCluster(str(tmp_path / "sub"), str(tmp_path / "norm.feather"), str(tmp_path / "w.feather"),
                                        ["fov0"], chans, xdim=2, ydim=2, distf=7)


def test_train_cell_som_under_manhattan(stand_ins, tmp_path, capsys):
    from ark_analysis_amd import flowsom
    from ark_analysis_amd.phenotyping import cell_som_clustering
    cols = ["m1", "m2", "m3", "m4"]
    cell = pd.DataFrame(mbr.test_rows(300, 4, 21), columns=cols)
    cell["fov"] = np.where(np.arange(300) % 2 == 0, "fov0", "fov1")
    cell["segmentation_label"] = np.arange(300)
    (tmp_path / "cell_table.csv").write_text("x\n")
    cobj = cell_som_clustering.train_cell_som(["fov0", "fov1"], str(tmp_path), str(tmp_path / "cell_table.csv"), cols, cell.copy(),
                                              xdim=3, ydim=2, seed=9, normalize=False, train_mode="batch", batch_steps=5, distf=1)
    capsys.readouterr()
    assert cobj.distf == 1 and pickle.loads(pickle.dumps(cobj)).distf == 1
    rows = cell[cols].to_numpy(dtype=np.float64)
    nodes = rows[np.random.RandomState(9).choice(300, 6, replace=False)]
    want = mbr.som_batch([rows], nodes, 3, 2, 1, 5, (0.05, 0.01), flowsom.default_radius_range(3, 2), 1,
                         quantum=mbr.run_quantum([rows], 5))
    np.testing.assert_array_equal(cobj.weights.to_numpy(), want)
    labelled = cobj.assign_som_clusters()
    np.testing.assert_array_equal(labelled["cell_som_cluster"].to_numpy(), mr.map_data_to_nodes(want, rows, 1)[0])
