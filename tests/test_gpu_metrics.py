"""FlowSOM's other distances on the GPU (distf 1 Manhattan, 3 Chebyshev, 4 cosine): BMU labels / distances and online
training, bit for bit against the numpy reference of tests/metric_reference.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import metric_reference as mr

pytestmark = pytest.mark.gpu

METRICS = (1, 3, 4)
DTYPES = {"f16": (np.float16, torch.float16), "f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}


def _assign(gpu, x_host, w, metric, dtype="f64", pad=0):
    """labels, dists of the device path; x_host [n, c] is cast to `dtype` first, `pad` extra columns make ldx > c."""
    from ark_analysis_amd import som_device
    npdt, tdt = DTYPES[dtype]
    with np.errstate(over="ignore"):   # 1e150 rows are +-inf in binary32 / binary16, on both sides
        x = np.ascontiguousarray(x_host, dtype=npdt)
    n, c = x.shape
    if pad:
        wide = torch.zeros((n, c + pad), dtype=tdt, device=gpu)
        wide[:, :c] = torch.from_numpy(x).to(gpu)
        xd = wide[:, :c]
    else:
        xd = torch.from_numpy(x).to(gpu)
    wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(gpu)
    lab, dist = som_device.assign(xd, wd, want_dists=True, metric=metric)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), dist.cpu().numpy(), x


def _check_assign(gpu, x_host, w, metric, dtype="f64", pad=0):
    lab, dist, xc = _assign(gpu, x_host, w, metric, dtype, pad)
    want_l, want_d = mr.map_data_to_nodes(w, xc, metric)
    assert np.array_equal(lab, want_l), (metric, dtype, int((lab != want_l).sum()))
    assert np.array_equal(dist.view(np.int64), want_d.view(np.int64)), (metric, dtype)


SHAPES = [(20000, 8, 100), (20000, 22, 100), (20000, 40, 400), (20000, 100, 100), (3000, 1, 10), (2000, 1024, 16),
          (5000, 12, 1)]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("metric", METRICS)
def test_assign_metric_shapes(gpu, metric, dtype):
    for n, c, k in SHAPES:
        rs = np.random.RandomState(n + c + k)
        x = rs.rand(n, c) * 4.0 - 1.0
        w = x[rs.choice(n, k, replace=False)].astype(DTYPES[dtype][0]).astype(np.float64)
        w[-1] += 0.01
        _check_assign(gpu, x, w, metric, dtype)


@pytest.mark.parametrize("metric", METRICS)
def test_assign_metric_strided_rows_and_empty(gpu, metric):
    rs = np.random.RandomState(7)
    x = rs.rand(4000, 22)
    w = rs.rand(100, 22)
    for dtype in DTYPES:
        _check_assign(gpu, x, w, metric, dtype, pad=5)
    _check_assign(gpu, np.zeros((0, 22)), w, metric, "f32")
    # rows wider than the register route (staged in LDS per chunk of channels), padded: ldx > c, tail chunks
    for c, pad in ((40, 3), (100, 7), (37, 1)):
        x = rs.rand(3000, c)
        w = rs.rand(70, c)
        for dtype in DTYPES:
            _check_assign(gpu, x, w, metric, dtype, pad=pad)


def _adversarial(rs, n=6000, c=10, k=60):
    w = rs.randint(0, 4, size=(k, c)).astype(np.float64)
    w[5] = w[2]                    # duplicated codebook rows
    w[9] = w[2]
    w[11] = 0.0                    # a zero node (cosine: NaN)
    x = rs.randint(0, 4, size=(n, c)).astype(np.float64)      # integer-valued rows: ties everywhere
    x[:200] = w[rs.randint(0, k, 200)]                       # rows equal to a node
    x[200:260] = 0.0                                          # zero rows
    x[300:340] = np.nan                                       # all-NaN rows
    x[340:400, ::3] = np.nan                                  # partial NaN rows
    x[400:600] = rs.rand(200, c) * 1e150                      # huge magnitudes
    x[600:800] = rs.rand(200, c) * 1e-150                     # tiny magnitudes
    x[800:900, 0] = np.inf
    return x, w


@pytest.mark.parametrize("metric", METRICS)
def test_assign_metric_adversarial(gpu, metric):
    rs = np.random.RandomState(11)
    x, w = _adversarial(rs)
    wbig = w.copy()
    wbig[20:30] *= 1e150
    wbig[30:40] *= 1e-150
    for dtype in ("f64", "f32", "f16"):
        _check_assign(gpu, x, w, metric, dtype)
    _check_assign(gpu, x, wbig, metric, "f64")


@pytest.mark.parametrize("metric", METRICS)
def test_assign_metric_config2_size(gpu, metric):
    """10.5 M x 22 fp32, K = 100: the reference on 100 000 sampled rows."""
    from ark_analysis_amd import som_device
    n, c, k = 10_485_760, 22, 100
    g = torch.Generator(device=gpu)
    g.manual_seed(metric)
    xd = torch.rand((n, c), generator=g, device=gpu, dtype=torch.float32)
    rs = np.random.RandomState(metric)
    w = xd[torch.from_numpy(rs.choice(n, k, replace=False)).to(gpu)].double().cpu().numpy()
    wd = torch.from_numpy(w).to(gpu)
    lab, dist = som_device.assign(xd, wd, want_dists=True, metric=metric)
    sample = np.sort(rs.choice(n, 100_000, replace=False))
    sd = torch.from_numpy(sample).to(gpu)
    xs = xd[sd].cpu().numpy()
    got_l, got_d = lab[sd].cpu().numpy(), dist[sd].cpu().numpy()
    want_l, want_d = mr.map_data_to_nodes(w, xs, metric)
    assert np.array_equal(got_l, want_l)
    assert np.array_equal(got_d, want_d)
    del xd


def test_assign_metric_2_is_pxsom_assign(gpu):
    from ark_analysis_amd import _capi, som_device
    L = _capi.lib()
    rs = np.random.RandomState(3)
    n, c, k = 30000, 22, 100
    xd = torch.from_numpy(rs.rand(n, c).astype(np.float32)).to(gpu)
    wd = torch.from_numpy(rs.rand(k, c)).to(gpu)
    want_l, want_d = som_device.assign(xd, wd, want_dists=True)
    nb = L.pxsom_assign_metric_workspace_bytes(n, c, k, 2)
    assert nb == L.pxsom_assign_workspace_bytes(n, c, k)
    ws = torch.empty(nb, dtype=torch.uint8, device=gpu)
    lab = torch.empty(n, dtype=torch.int32, device=gpu)
    dist = torch.empty(n, dtype=torch.float64, device=gpu)
    _capi.check(L.pxsom_assign_metric(xd.data_ptr(), n, c, c, _capi.PXSOM_F32, wd.data_ptr(), k, lab.data_ptr(),
                                      dist.data_ptr(), ws.data_ptr(), nb, 2, _capi.stream_ptr()), "pxsom_assign_metric")
    assert torch.equal(lab, want_l) and torch.equal(dist, want_d)


def test_assign_metric_exact_rows_reported(gpu):
    from ark_analysis_amd import som_device
    rs = np.random.RandomState(5)
    xd = torch.from_numpy(rs.rand(1234, 6)).to(gpu)
    wd = torch.from_numpy(rs.rand(9, 6)).to(gpu)
    som_device.assign(xd, wd, metric=3)
    assert som_device.last_exact_rows(som_device.assign.last_workspace) == 1234


# (xdim, ydim, c, n, rlen, int_abs, dtype): the register route (c = 8, K = 100; c = 40, K = 400), the codebook in LDS
# (c = 150, K = 100; c = 20, K = 600) and trained where it lies (c = 128, K = 264), small grids, two passes
ONLINE_CASES = [
    (10, 10, 8, 1500, 1, False, "f32"),
    (5, 3, 6, 700, 2, False, "f64"),
    (5, 3, 6, 700, 2, True, "f64"),
    (20, 20, 40, 700, 1, False, "f32"),
    (10, 10, 150, 400, 1, False, "f64"),
    (20, 30, 20, 900, 1, False, "f16"),
    (12, 22, 128, 350, 1, False, "f32"),
    (10, 10, 22, 400, 2, True, "f32"),
    (10, 10, 22, 400, 2, False, "f32"),
]


def _online(gpu, x, w0, xdim, ydim, rlen, order, metric, int_abs):
    from ark_analysis_amd import som_device
    from ark_analysis_amd.flowsom import default_radius_range
    rr = default_radius_range(xdim, ydim)
    wd = torch.from_numpy(w0.copy()).to(gpu)
    som_device.train_online(torch.from_numpy(x).to(gpu), wd, xdim, ydim, rlen, (0.05, 0.01), rr,
                            torch.from_numpy(order).to(gpu), int_abs=int_abs, metric=metric)
    got = wd.cpu().numpy()
    want = mr.som_online(x, w0, xdim, ydim, rlen, (0.05, 0.01), rr, order, metric, int_abs=int_abs)
    return got, want


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", ONLINE_CASES, ids=lambda t: "%dx%d_c%d_r%d%s_%s" % (t[0], t[1], t[2], t[4],
                                                                                        "_int" if t[5] else "", t[6]))
def test_train_online_metric_equals_reference(gpu, metric, case):
    xdim, ydim, c, n, rlen, int_abs, dtype = case
    rs = np.random.RandomState(c * 31 + n)
    x = (rs.rand(n, c) * (3.0 if int_abs else 1.0)).astype(DTYPES[dtype][0])
    w0 = x[rs.choice(n, xdim * ydim, replace=False)].astype(np.float64)
    order = rs.randint(0, n, size=n * rlen).astype(np.int64)
    got, want = _online(gpu, x, w0, xdim, ydim, rlen, order, metric, int_abs)
    assert np.array_equal(got, want), (metric, case, float(np.nanmax(np.abs(got - want))))


@pytest.mark.parametrize("metric", METRICS)
def test_train_online_metric_ties_and_nan(gpu, metric):
    """Integer rows (ties), a zero node 0 and zero rows (cosine: NaN distances), NaN channels (Chebyshev skips them)."""
    rs = np.random.RandomState(17)
    n, c = 600, 7
    x = rs.randint(0, 3, size=(n, c)).astype(np.float64)
    x[10:20] = 0.0
    x[30:40, 2] = np.nan
    w0 = rs.randint(0, 3, size=(25, c)).astype(np.float64)
    w0[0] = 0.0
    w0[7] = w0[3]
    order = rs.randint(0, n, size=n).astype(np.int64)
    got, want = _online(gpu, x, w0, 5, 5, 1, order, metric, False)
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("metric", METRICS)
def test_flowsom_som_and_map_with_distf(gpu, metric):
    from ark_analysis_amd import flowsom
    rs = np.random.RandomState(23)
    n, c, xdim, ydim, rlen, seed = 1500, 5, 6, 6, 1, 42
    x = rs.rand(n, c)
    got = flowsom.som(x, xdim, ydim, rlen, distf=metric, seed=seed)
    init_idx, order = flowsom.som_init_and_order(n, xdim * ydim, rlen, seed)
    want = mr.som_online(x, x[init_idx], xdim, ydim, rlen, (0.05, 0.01), flowsom.default_radius_range(xdim, ydim),
                         order, metric)
    assert np.array_equal(got, want)
    lab, dist = flowsom.map_data_to_nodes(got, x, distf=metric)
    want_l, want_d = mr.map_data_to_nodes(got, x, metric)
    assert np.array_equal(lab, want_l) and np.array_equal(dist, want_d)


def test_metric_entry_point_rejects_unknown_metric_on_device(gpu):
    from ark_analysis_amd import _capi
    L = _capi.lib()
    xd = torch.zeros((10, 4), dtype=torch.float32, device=gpu)
    wd = torch.zeros((2, 4), dtype=torch.float64, device=gpu)
    lab = torch.empty(10, dtype=torch.int32, device=gpu)
    ws = torch.empty(L.pxsom_assign_metric_workspace_bytes(10, 4, 2, 1), dtype=torch.uint8, device=gpu)
    rc = L.pxsom_assign_metric(xd.data_ptr(), 10, 4, 4, _capi.PXSOM_F32, wd.data_ptr(), 2, lab.data_ptr(), None,
                               ws.data_ptr(), ws.numel(), 9, ctypes.c_void_p(_capi.stream_ptr()))
    assert rc == -1 and b"unknown metric 9" in L.pxsom_last_error()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("grid", [(10, 10), (20, 20)])
def test_train_online_metric_ties_across_waves(gpu, metric, grid):
    """More than one wave of nodes: duplicated nodes in different waves (3, 70 and, on 20 x 20, 130 and 300), integer rows
    that equal node 3, zero rows and -- for cosine -- a zero node 0 (NaN at node 0 keeps node 0)."""
    xdim, ydim = grid
    k = xdim * ydim
    rs = np.random.RandomState(29 + k)
    n, c = 900, 6
    w0 = rs.randint(0, 3, size=(k, c)).astype(np.float64)
    for dup in (70, 130, 300):
        if dup < k:
            w0[dup] = w0[3]
    if metric == 4:
        w0[0] = 0.0
    x = rs.randint(0, 3, size=(n, c)).astype(np.float64)
    x[:300] = w0[3]                 # rows equal to node 3 (and its duplicates in later waves)
    x[300:330] = 0.0
    order = rs.randint(0, n, size=n).astype(np.int64)
    order[:40] = np.arange(40)      # the first steps present those rows while the duplicates are still equal
    got, want = _online(gpu, x, w0, xdim, ydim, 1, order, metric, False)
    assert np.array_equal(got, want, equal_nan=True)
