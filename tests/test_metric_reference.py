"""FlowSOM's other distances (distf 1, 3, 4): the numpy reference, the ABI's argument checks, the front end's refusals.

CPU only.  The reference's Euclidean branch is held against the oracle bit for bit (the loop the other metrics share),
then each metric against hand-checked cases.  The GPU side is tests/test_gpu_metrics.py.
"""
import ctypes

import numpy as np
import pytest

from tests import metric_reference as mr

DBL_MAX = np.finfo(np.float64).max


@pytest.mark.parametrize("n,c,k", [(500, 8, 100), (300, 22, 25), (200, 3, 7)])
def test_reference_euclidean_map_equals_oracle(oracle, n, c, k):
    rs = np.random.RandomState(n + c + k)
    x = rs.rand(n, c)
    w = rs.rand(k, c)
    w[3] = w[1]                       # duplicated node: ties go to the first
    x[:5] = w[rs.randint(0, k, 5)]    # rows equal to a node
    x[7, 2] = np.nan                  # a NaN row: label 0
    want_l, want_d = oracle.map_data_to_nodes(w, x)
    got_l, got_d = mr.map_data_to_nodes(w, x, 2)
    assert np.array_equal(got_l, want_l)
    assert np.array_equal(got_d, want_d)


@pytest.mark.parametrize("xdim,ydim,c,rlen", [(10, 10, 8, 1), (5, 3, 4, 2), (4, 4, 6, 2)])
def test_reference_euclidean_online_equals_oracle(oracle, xdim, ydim, c, rlen):
    from ark_analysis_amd.flowsom import default_radius_range
    rs = np.random.RandomState(xdim * ydim + c)
    n = 300
    x = rs.rand(n, c)
    w0 = x[rs.choice(n, xdim * ydim, replace=False)].copy()
    order = rs.randint(0, n, size=n * rlen).astype(np.int64)
    rr = default_radius_range(xdim, ydim)
    want = oracle.som_online(x, w0, xdim, ydim, rlen, (0.05, 0.01), rr, order)
    got = mr.som_online(x, w0, xdim, ydim, rlen, (0.05, 0.01), rr, order, 2)
    assert np.array_equal(got, want)


def test_manhattan_hand_checked():
    w = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.0]])
    x = np.array([[1.0, 0.0],     # |1|+|0| = 1 to node 0, 0+1 = 1 to node 1, 1+0 = 1 to node 2: first wins
                  [2.0, 1.0],     # 3, 1, 1: node 1
                  [np.nan, 0.0]])  # NaN everywhere: label 0, DBL_MAX
    lab, d = mr.map_data_to_nodes(w, x, 1)
    assert lab.tolist() == [1, 2, 0]
    assert d.tolist() == [1.0, 1.0, DBL_MAX]


def test_chebyshev_hand_checked_nan_channels():
    w = np.array([[0.0, 0.0, 0.0], [5.0, 1.0, 0.0], [5.0, 5.0, 5.0]])
    x = np.array([[np.nan, 1.0, 0.0],        # channel 0 skipped: 1 to node 0, 0 to node 1, 5 to node 2 -> node 1
                  [5.0, np.nan, np.nan],     # 5, 0, 0 -> node 1 (first of the two zeros)
                  [np.nan, np.nan, np.nan],  # all NaN: 0 to every node -> label 1
                  [4.0, 4.0, 4.0]])          # 4, 3, 1 -> node 2
    lab, d = mr.map_data_to_nodes(w, x, 3)
    assert lab.tolist() == [2, 2, 1, 3]
    assert d.tolist() == [0.0, 0.0, 0.0, 1.0]


def test_cosine_hand_checked_zero_row_and_node():
    w = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [0.0, 1.0]])
    x = np.array([[3.0, 0.0],    # NaN (zero node), 0, 0, 1 -> node 1: the first of the equal directions
                  [0.0, 0.0],    # zero row: NaN to every node -> label 0
                  [1.0, 1.0]])   # 1 - 1/sqrt(2) to nodes 1, 2 and 3 -> node 1
    lab, d = mr.map_data_to_nodes(w, x, 4)
    assert lab.tolist() == [2, 0, 2]
    assert d[0] == 0.0 and d[1] == DBL_MAX
    assert d[2] == (-1.0 / (np.sqrt(2.0) * 1.0)) + 1.0
    dd = mr.distances(x, w, 4)
    assert np.isnan(dd[0, 0]) and np.isnan(dd[1]).all()


def test_online_nearest_rules():
    assert mr.online_nearest([np.nan, 0.0, 1.0]) == 0            # node 0's NaN is never replaced
    assert mr.online_nearest([2.0, np.nan, 1.0, 1.0]) == 2       # later NaNs are skipped; first minimum
    assert mr.online_nearest([np.inf, np.nan, np.inf]) == 0


def test_online_reference_metrics_move_the_bmu(oracle):
    """One step with the radius pinned: only the BMU moves, by alpha * (x - w)."""
    w0 = np.array([[0.0, 0.0], [1.0, 1.0], [3.0, 0.0], [0.0, 3.0]])
    x = np.array([[2.0, 0.0]])
    # L1: 2, 2, 1, 5 -> node 2; Linf: 2, 1, 1, 3 -> node 1 (the first); cosine: NaN, 1 - 1/sqrt2, 0, 1 -> node 0, whose
    # NaN no later distance compares smaller than
    for distf, bmu in ((1, 2), (3, 1), (4, 0)):
        got = mr.som_online(x, w0, 2, 2, 1, (0.5, 0.5), (0.0, 0.0), np.array([0]), distf)
        want = w0.copy()
        want[bmu] = want[bmu] + (x[0] - want[bmu]) * 0.5
        assert np.array_equal(got, want), distf


def test_new_symbols_exported_and_unknown_metric_rejected_without_gpu():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    for name in ("pxsom_assign_metric", "pxsom_train_online_metric", "pxsom_assign_metric_workspace_bytes"):
        assert hasattr(lib, name)
    assert lib.pxsom_abi_version() == 9
    for metric in (0, 5, -1):
        rc = lib.pxsom_assign_metric(None, 0, 4, 4, 0, None, 1, None, None, None, 0, metric, None)
        assert rc == -1
        assert b"unknown metric %d" % metric in lib.pxsom_last_error()
        rc = lib.pxsom_train_online_metric(None, 0, 4, 4, 0, None, 2, 2, 1, 0.05, 0.01, 1.0, 0.0, None, metric, 0, None)
        assert rc == -1
        assert b"unknown metric %d" % metric in lib.pxsom_last_error()
        assert lib.pxsom_assign_metric_workspace_bytes(100, 4, 10, metric) == 0
    assert lib.pxsom_assign_metric_workspace_bytes(100, 4, 10, 2) == lib.pxsom_assign_workspace_bytes(100, 4, 10)
    assert lib.pxsom_assign_metric_workspace_bytes(100, 4, 10, 1) >= 4 * 16 * 8
    # a known metric with a bad shape is refused before any HIP call as well
    assert lib.pxsom_assign_metric(None, 10, 0, 4, 0, None, 1, None, None, None, 0, 1, None) == -2
    assert lib.pxsom_assign_metric(None, -1, 4, 4, 0, None, 1, None, None, None, 0, 3, None) == -1
    ws = ctypes.create_string_buffer(8)
    assert lib.pxsom_assign_metric(ctypes.addressof(ws), 10, 4, 4, 0, ctypes.addressof(ws), 1, ctypes.addressof(ws),
                                   None, ctypes.addressof(ws), 8, 4, None) == -3
    assert lib.pxsom_train_online_metric(None, 10, 4, 4, 0, None, 2, 2, 1, 0.05, 0.01, 1.0, 0.0, None, 1, 0, None) == -1


def test_front_end_refuses_unknown_distf_before_any_device():
    from ark_analysis_amd import flowsom
    x = np.zeros((200, 3))
    with pytest.raises(NotImplementedError, match="distf=5.*1 \\(Manhattan\\)"):
        flowsom.map_data_to_nodes(np.zeros((4, 3)), x, distf=5)
    with pytest.raises(NotImplementedError, match="distf=0"):
        flowsom.som(x, 2, 2, distf=0)
    with pytest.raises(NotImplementedError):
        flowsom.som_with_inputs(x, np.zeros((4, 3)), np.zeros(200, dtype=np.int64), 2, 2, 1, distf=7)
    for bad in (True, False, 2.0, "2", None):
        with pytest.raises(NotImplementedError):
            flowsom.map_data_to_nodes(np.zeros((4, 3)), x, distf=bad)
    assert flowsom._check_distf(np.int64(3)) == 3
    assert flowsom.DISTF_CODES == (1, 2, 3, 4)
    assert set(flowsom.RECALLED["distances"][0]) == {1, 2, 3, 4}
    assert "unpinned" in flowsom.RECALLED["distances"][1]


def test_device_wrappers_reject_unknown_metric():
    from ark_analysis_amd import som_device
    for bad in (6, True, 1.0):
        with pytest.raises(ValueError, match="unknown metric"):
            som_device._check_metric(bad)
    with pytest.raises(ValueError, match="Euclidean route only"):
        som_device.assign(None, None, screen_all_lists=True, metric=1)
