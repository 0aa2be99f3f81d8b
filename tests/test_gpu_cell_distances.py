"""pxsom_nearest_type_means on the GPU against the numpy statement of tests/cell_distance_reference.py (float32 bit
patterns equal, NaN in the same places: no tolerance), the device's float32(sqrt(s)) against numpy's on more than 10^6
pairs, and generate_cell_distance_analysis on the HIP path against the g19 fixture of the reference."""
import numpy as np
import pytest
import torch

from tests import cell_distance_reference as cr
from tests import test_cell_distances as tc

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 257, 1000, 5000]
TYPE_COUNTS = [1, 2, 7, 33]
KS = [1, 5, 8, 13, 32]


def _cohort(rs, sizes, n_types):
    """FOVs of the given sizes on square fields of about one cell per 30 x 30; a few cells sit on another cell's
    centroid, and every type is drawn (so some are absent from, or short of k cells in, small FOVs)."""
    xy, types = [], []
    for m in sizes:
        pts = rs.uniform(0, max(30.0 * np.sqrt(m), 1.0), (m, 2))
        if m >= 2:
            dup = rs.randint(0, m, size=max(1, m // 50))
            pts[dup] = pts[rs.randint(0, m, size=dup.size)]
        xy.append(pts)
        types.append(rs.randint(0, n_types, m))
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(xy).reshape(-1, 2), np.concatenate(types).astype(np.int64), seg


def _device(gpu, xy, types, seg, n_types, k, type_dtype=torch.int64):
    from ark_analysis_amd import som_device
    got = som_device.nearest_type_means(torch.from_numpy(np.ascontiguousarray(xy)).to(gpu),
                                        torch.from_numpy(types).to(gpu).to(type_dtype), torch.from_numpy(seg).to(gpu),
                                        n_types, k)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(xy), n_types)
    return got.cpu().numpy()


@pytest.mark.parametrize("n_types", TYPE_COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_statement(gpu, n, n_types):
    """Several FOVs in one call -- n cells, an empty one, a small one, n again (one FOV of 5 000 plus a small one at the
    largest size) -- for every k of KS, rows in random type order."""
    rs = np.random.RandomState(1000 * n + n_types)
    sizes = [n, 0, 300] if n >= 5000 else [n, 0, min(n, 37) + 3, n]
    xy, types, seg = _cohort(rs, sizes, n_types)
    want = cr.nearest_type_means_for(xy, types, seg, n_types, KS)
    for k in KS:
        got = _device(gpu, xy, types, seg, n_types, k, torch.int32 if n_types % 2 else torch.int64)
        tc.assert_same_float32(got, want[k], "n=%d T=%d k=%d" % (n, n_types, k))


def test_only_empty_fovs_and_no_cells(gpu):
    xy, types = np.zeros((0, 2)), np.zeros(0, dtype=np.int64)
    for seg in (np.array([0]), np.array([0, 0, 0])):
        assert _device(gpu, xy, types, seg.astype(np.int64), 4, 5).shape == (0, 4)


def test_tie_grid(gpu):
    """A 20 x 20 integer grid: every distance is tied many times over, and the k-th smallest sits inside a tie."""
    gy, gx = np.mgrid[0:20, 0:20]
    xy = np.stack([gy.ravel(), gx.ravel()], 1).astype(np.float64) * 10
    rs = np.random.RandomState(3)
    types = rs.randint(0, 3, len(xy)).astype(np.int64)
    seg = np.array([0, len(xy)], dtype=np.int64)
    want = cr.nearest_type_means_for(xy, types, seg, 3, KS)
    for k in KS:
        tc.assert_same_float32(_device(gpu, xy, types, seg, 3, k), want[k], "k=%d" % k)
    one = np.zeros(len(xy), dtype=np.int64)
    got = _device(gpu, xy, one, seg, 1, 4)
    assert (got[np.ix_([21 * 5])] == 10).all()            # an interior cell: its four nearest are at exactly 10


def test_coincident_cells(gpu):
    """130 cells on one point, 70 on another 10 away: the cells at float32 distance 0 do not count, so a cell of the
    first group sees only the 70 (mean exactly 10, or NaN when its type has fewer than k among them)."""
    rs = np.random.RandomState(4)
    xy = np.concatenate([np.tile([[1 / 3, 2 / 7]], (130, 1)), np.tile([[1 / 3, 2 / 7 + 10]], (70, 1))])
    types = rs.randint(0, 5, 200).astype(np.int64)
    seg = np.array([0, 200], dtype=np.int64)
    want = cr.nearest_type_means_for(xy, types, seg, 5, KS)
    for k in KS:
        got = _device(gpu, xy, types, seg, 5, k)
        tc.assert_same_float32(got, want[k], "k=%d" % k)
        far = np.bincount(types[130:], minlength=5)
        assert (np.isnan(got[:130]) == (far < k)[None, :]).all()
        assert (got[:130][:, far >= k] == 10).all()


@pytest.mark.parametrize("k", KS)
def test_exactly_k_and_k_minus_one_members(gpu, k):
    """Type 0 has k - 1 cells (NaN for everyone), type 1 exactly k (a cell of it has k - 1 others: NaN for its own
    type, a number for every other cell), type 2 has k + 1."""
    rs = np.random.RandomState(k)
    types = np.concatenate([np.full(k - 1, 0), np.full(k, 1), np.full(k + 1, 2), np.full(40, 3)]).astype(np.int64)
    types = types[rs.permutation(len(types))]
    xy = rs.uniform(0, 200, (len(types), 2))
    seg = np.array([0, len(types)], dtype=np.int64)
    got = _device(gpu, xy, types, seg, 4, k)
    tc.assert_same_float32(got, cr.nearest_type_means(xy, types, seg, 4, k))
    assert np.isnan(got[:, 0]).all()
    assert (np.isnan(got[:, 1]) == (types == 1)).all()
    assert not np.isnan(got[:, 2:]).any()


def test_rows_keep_the_callers_order(gpu):
    """Permuting the cells inside each FOV permutes the rows of the result and nothing else."""
    rs = np.random.RandomState(5)
    xy, types, seg = _cohort(rs, [700, 0, 129, 300], 11)
    base = _device(gpu, xy, types, seg, 11, 5)
    perm = np.concatenate([a + rs.permutation(b - a) for a, b in zip(seg[:-1], seg[1:])]).astype(np.int64)
    tc.assert_same_float32(_device(gpu, xy[perm], types[perm], seg, 11, 5), base[perm])
    by_type = np.concatenate([a + np.argsort(types[a:b], kind="stable") for a, b in zip(seg[:-1], seg[1:])]).astype(np.int64)
    tc.assert_same_float32(_device(gpu, xy[by_type], types[by_type], seg, 11, 5), base[by_type])


def _sqrt_pairs():
    """(a [m, 2], b [m, 2]): pairs of points whose squared distances stress the square root and the cast."""
    rs = np.random.RandomState(14)
    a, b = [], []
    for scale in (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6):          # uniform centroids, ten scales
        a.append(rs.uniform(0, 2048, (80000, 2)) * scale)
        b.append(rs.uniform(0, 2048, (80000, 2)) * scale)
    g = rs.randint(0, 4096, (200000, 4)).astype(np.float64)                       # integer grids: exact s, many squares
    a.append(g[:, :2])
    b.append(g[:, 2:])
    # float32 rounding midpoints m and their binary64 neighbours as the distance itself: float32(sqrt(m * m)) is a tie
    f = np.abs(rs.standard_normal(40000) * 10.0 ** rs.randint(-3, 7, 40000)).astype(np.float32)
    mid = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    for dx in (mid, np.nextafter(mid, 0), np.nextafter(mid, np.inf), f.astype(np.float64)):
        a.append(np.zeros((len(dx), 2)))
        b.append(np.stack([dx, np.zeros(len(dx))], 1))
    return np.concatenate(a), np.concatenate(b)


def test_square_root_and_cast_are_numpys(gpu):
    """More than 10^6 FOVs of two cells at k = 1: the output is float32(sqrt(s)) itself."""
    a, b = _sqrt_pairs()
    m = len(a)
    assert m >= 1000000
    xy = np.stack([a, b], 1).reshape(2 * m, 2)
    seg = np.arange(0, 2 * m + 1, 2, dtype=np.int64)
    got = _device(gpu, xy, np.zeros(2 * m, dtype=np.int64), seg, 1, 1)
    dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    want = np.sqrt(dx * dx + dy * dy).astype(np.float32)
    want = np.where(want > 0, want, np.float32(np.nan))
    tc.assert_same_float32(got[0::2, 0], want)
    tc.assert_same_float32(got[1::2, 0], want)
    assert np.isfinite(want).sum() > 1000000 and len(np.unique(np.frexp(want[np.isfinite(want)])[1])) > 25
    sub = np.random.RandomState(1).choice(m, 400, replace=False)
    for i in sub:            # and the statement itself (cdist) on a sample
        w = cr.nearest_type_means(xy[2 * i:2 * i + 2], np.zeros(2, dtype=np.int64), [0, 2], 1, 1)
        tc.assert_same_float32(got[2 * i:2 * i + 2], w)


def test_raw_call_writes_every_entry_and_nothing_else(gpu):
    """The C entry on rows already sorted by type, into a slice of a buffer filled with a sentinel: every entry of the
    slice is written (absent types and rows of no FOV as NaN), nothing outside it."""
    from ark_analysis_amd import _capi, som_device
    rs = np.random.RandomState(6)
    n_types = 9
    xy, types, seg = _cohort(rs, [300, 0, 70, 515], n_types)
    types[types == 4] = 5                       # a type no cell has
    types[seg[2]:seg[3]] = 7                    # a FOV of one type
    order = np.concatenate([a + np.argsort(types[a:b], kind="stable") for a, b in zip(seg[:-1], seg[1:])])
    xy, types = xy[order], types[order]
    n = len(xy)
    _, s_zero = som_device.neighbor_thresholds(1)
    guard = 1024
    sentinel = 0x5A5A5A5A
    for k in (3, 13, 32):
        buf = torch.full((guard + n * n_types + guard,), sentinel, dtype=torch.int32, device=gpu)
        xy_d, ty_d = torch.from_numpy(xy).to(gpu), torch.from_numpy(types.astype(np.int32)).to(gpu)
        seg_d = torch.from_numpy(seg).to(gpu)
        rc = _capi.lib().pxsom_nearest_type_means(xy_d.data_ptr(), ty_d.data_ptr(), seg_d.data_ptr(), len(seg) - 1, n,
                                                  n_types, k, s_zero, buf.data_ptr() + guard * 4, _capi.stream_ptr())
        _capi.check(rc, "pxsom_nearest_type_means")
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:guard] == sentinel).all() and (host[guard + n * n_types:] == sentinel).all()
        inner = host[guard:guard + n * n_types]
        assert not (inner == sentinel).any()
        got = inner.view(np.float32).reshape(n, n_types)
        tc.assert_same_float32(got, cr.nearest_type_means(xy, types, seg, n_types, k))
        assert np.isnan(got[:, 4]).all()
    # rows that no FOV holds come back as NaN
    buf = torch.full((n * n_types,), sentinel, dtype=torch.int32, device=gpu)
    short = torch.from_numpy(np.array([0, 100], dtype=np.int64)).to(gpu)
    rc = _capi.lib().pxsom_nearest_type_means(xy_d.data_ptr(), ty_d.data_ptr(), short.data_ptr(), 1, n, n_types, 3, s_zero,
                                              buf.data_ptr(), _capi.stream_ptr())
    _capi.check(rc, "pxsom_nearest_type_means")
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.float32).reshape(n, n_types)
    assert np.isnan(got[100:]).all()
    tc.assert_same_float32(got[:100], cr.nearest_type_means(xy[:100], types[:100], [0, 100], n_types, 3))


def test_wrapper_argument_errors(gpu):
    from ark_analysis_amd import som_device
    xy = torch.zeros((4, 2), dtype=torch.float64, device=gpu)
    ty = torch.zeros(4, dtype=torch.int64, device=gpu)
    seg = torch.tensor([0, 4], device=gpu)
    with pytest.raises(ValueError, match="float64"):
        som_device.nearest_type_means(xy.float(), ty, seg, 2, 5)
    with pytest.raises(ValueError, match="n_types"):
        som_device.nearest_type_means(xy, ty + 2, seg, 2, 5)
    with pytest.raises(ValueError, match="offsets"):
        som_device.nearest_type_means(xy, ty, torch.tensor([0, 3], device=gpu), 2, 5)
    for k in (0, 33):
        with pytest.raises(ValueError, match="32"):
            som_device.nearest_type_means(xy, ty, seg, 2, k)
    from ark_analysis_amd import _capi
    out = torch.zeros((4, 2), dtype=torch.float32, device=gpu)
    rc = _capi.lib().pxsom_nearest_type_means(xy.data_ptr(), ty.int().data_ptr(), seg.data_ptr(), 1, 4, 2, 33, 0.0,
                                              out.data_ptr(), _capi.stream_ptr())
    assert rc == -1 and b"32" in _capi.lib().pxsom_last_error()


def test_generate_cell_distance_analysis_hip_equals_fixture(gpu, tmp_path):
    tc.check_fixture_cases(tmp_path)


def test_per_fov_functions_hip(gpu):
    tc.check_per_fov_functions()
