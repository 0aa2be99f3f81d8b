"""pxsom_close_pair_counts on the GPU against the numpy statement of tests/close_pairs_reference.py (exact integer
equality: no tolerance), and compute_close_cell_num / compute_mixing_scores / compute_mixing_score on the HIP path
against the g23 fixture of the reference."""
import numpy as np
import pytest
import torch

from tests import close_pairs_reference as cpr
from tests import test_mixing as tm

pytestmark = pytest.mark.gpu

FOV_SIZES = [1, 63, 64, 65, 255, 256, 257, 513]
SET_COUNTS = [(1, 2), (2, 1), (31, 32), (32, 33), (33, 63), (63, 64), (64, 31), (64, 64)]


def _points(rs, sizes, density=12.0, distlim=50.0):
    """FOVs of the given sizes on square fields sized for about ``density`` neighbours within distlim; a few cells sit on
    another cell's centroid."""
    xy = []
    for m in sizes:
        side = max(np.sqrt(m * np.pi * distlim ** 2 / density), 1.0)
        pts = rs.uniform(0, side, (m, 2))
        if m >= 2:
            dup = rs.randint(0, m, size=max(1, m // 50))
            pts[dup] = pts[rs.randint(0, m, size=dup.size)]
        xy.append(pts)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(xy).reshape(-1, 2), seg


def _masks(rs, n, n_sets, density=0.4):
    """[n] uint64 with bits below n_sets drawn at ``density``; a tenth of the cells in no set, a tenth in every set."""
    bits = np.zeros((n, 64), dtype=bool)
    bits[:, :n_sets] = rs.rand(n, n_sets) < density
    bits[rs.rand(n) < 0.1] = False
    bits[rs.rand(n) < 0.1, :n_sets] = True
    return cpr.pack(bits)


def _to(gpu, mask):
    return torch.from_numpy(np.ascontiguousarray(mask).view(np.int64)).to(gpu)


def _device(gpu, xy, member_q, member_c, seg, n_sets_q, n_sets_c, distlim, self_neighbor):
    from ark_analysis_amd import som_device
    mq = _to(gpu, member_q)
    mc = mq if member_c is member_q else _to(gpu, member_c)
    got = som_device.close_pair_counts(torch.from_numpy(np.ascontiguousarray(xy)).to(gpu), mq, mc,
                                       torch.from_numpy(seg).to(gpu), n_sets_q, n_sets_c, distlim, self_neighbor)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(seg) - 1, n_sets_q, n_sets_c)
    return got.cpu().numpy()


def _same(got, want):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def _check(gpu, xy, member_q, member_c, seg, n_sets_q, n_sets_c, distlim=50):
    for self_neighbor in (False, True):
        got = _device(gpu, xy, member_q, member_c, seg, n_sets_q, n_sets_c, distlim, self_neighbor)
        _same(got, cpr.close_pair_counts(xy, member_q, member_c, seg, n_sets_q, n_sets_c, distlim, self_neighbor))
    return got


@pytest.mark.parametrize("m", FOV_SIZES)
def test_kernel_equals_statement_on_fov_sizes(gpu, m):
    """Several FOVs in one call -- m cells, an empty one, a small one, m again -- with both self_neighbor values, the
    two masks as one tensor and as two."""
    rs = np.random.RandomState(100 + m)
    xy, seg = _points(rs, [m, 0, min(m, 37) + 3, m])
    mq, mc = _masks(rs, len(xy), 3), _masks(rs, len(xy), 5)
    got = _check(gpu, xy, mq, mc, seg, 3, 5)
    assert m < 63 or got.sum() > 0
    _check(gpu, xy, mq, mq, seg, 3, 3)


def test_many_small_fovs_inside_one_workgroup(gpu):
    rs = np.random.RandomState(1)
    xy, seg = _points(rs, [30] * 10, density=8.0)
    mq, mc = _masks(rs, len(xy), 4), _masks(rs, len(xy), 9)
    got = _check(gpu, xy, mq, mc, seg, 4, 9)
    assert (got.reshape(10, -1).sum(axis=1) > 0).all()


def test_fov_spanning_three_workgroups_with_ends_inside_blocks(gpu):
    """Rows 100 .. 700 are one FOV: it begins inside block 0, fills block 1 and ends inside block 2."""
    rs = np.random.RandomState(2)
    xy, seg = _points(rs, [100, 600, 50])
    mq, mc = _masks(rs, len(xy), 20), _masks(rs, len(xy), 33)
    _check(gpu, xy, mq, mc, seg, 20, 33, 37.5)


def test_empty_fovs_first_last_and_between(gpu):
    rs = np.random.RandomState(3)
    xy, seg = _points(rs, [0, 0, 70, 0, 300, 0, 0, 5, 0])
    mq = _masks(rs, len(xy), 6)
    got = _check(gpu, xy, mq, mq, seg, 6, 6)
    assert (got[[0, 1, 3, 5, 6, 8]] == 0).all() and got[2].sum() > 0 and got[4].sum() > 0


def test_no_cells(gpu):
    xy, mask = np.zeros((0, 2)), np.zeros(0, dtype=np.uint64)
    assert _device(gpu, xy, mask, mask, np.array([0], dtype=np.int64), 2, 3, 50, False).shape == (0, 2, 3)
    got = _device(gpu, xy, mask, mask, np.array([0, 0, 0], dtype=np.int64), 2, 3, 50, False)
    assert got.shape == (2, 2, 3) and (got == 0).all()


@pytest.mark.parametrize("n_sets_q,n_sets_c", SET_COUNTS)
def test_kernel_equals_statement_on_set_counts(gpu, n_sets_q, n_sets_c):
    """Cells in no set, cells in every set, the highest bit of each mask, one tensor for both masks where the counts
    allow; three FOVs of which one spans two workgroups."""
    rs = np.random.RandomState(64 * n_sets_q + n_sets_c)
    xy, seg = _points(rs, [130, 290, 64])
    mq, mc = _masks(rs, len(xy), n_sets_q), _masks(rs, len(xy), n_sets_c, density=0.15)
    assert (mq == 0).any() and (mq >> np.uint64(n_sets_q - 1)).any() and (mc >> np.uint64(n_sets_c - 1)).any()
    got = _check(gpu, xy, mq, mc, seg, n_sets_q, n_sets_c)
    assert (got[:, n_sets_q - 1, n_sets_c - 1] > 0).all()
    if n_sets_q == n_sets_c:
        _check(gpu, xy, mq, mq, seg, n_sets_q, n_sets_c)


def test_bit_63(gpu):
    """Only bit 63 set (the sign bit of the int64 the mask travels in) and only bit 0 set."""
    rs = np.random.RandomState(63)
    xy, seg = _points(rs, [300])
    top = np.where(rs.rand(300) < 0.5, np.uint64(1) << np.uint64(63), np.uint64(0)).astype(np.uint64)
    low = np.where(rs.rand(300) < 0.5, np.uint64(1), np.uint64(0)).astype(np.uint64)
    got = _check(gpu, xy, top | low, top, seg, 64, 64)
    assert got[0, 63, 63] > 0 and got[0, 0, 63] > 0 and got[0, 1:63].sum() == 0 and got[0, :, :63].sum() == 0


def test_exact_tie_grid_and_coincident_cells(gpu):
    """The 20 x 20 grid of pitch 10: the 3 376 ordered pairs at exactly 50 are excluded at distlim 50 and included one
    float32 above it.  130 cells on one point and 70 on another 10 away: coincident cells pair only with self_neighbor."""
    gy, gx = np.mgrid[0:20, 0:20]
    xy = np.stack([gy.ravel(), gx.ravel()], 1).astype(np.float64) * 10
    rs = np.random.RandomState(4)
    mq = _masks(rs, len(xy), 3) | np.uint64(4)             # set 2 holds every cell
    seg = np.array([0, len(xy)], dtype=np.int64)
    above = float(np.nextafter(np.float32(50), np.float32(60)))
    totals = {}
    for distlim in (50, above, np.float64(50), 50.0):
        totals[distlim] = int(_check(gpu, xy, mq, mq, seg, 3, 3, distlim)[0, 2, 2])     # self_neighbor: + 400 both times
    assert totals[above] - totals[50] == 3376
    xy = np.concatenate([np.tile([[1 / 3, 2 / 7]], (130, 1)), np.tile([[1 / 3, 2 / 7 + 10]], (70, 1))])
    ones = np.ones(200, dtype=np.uint64)
    seg = np.array([0, 200], dtype=np.int64)
    assert _device(gpu, xy, ones, ones, seg, 1, 1, 50, False)[0, 0, 0] == 2 * 130 * 70
    assert _device(gpu, xy, ones, ones, seg, 1, 1, 50, True)[0, 0, 0] == 200 * 200


def test_stray_bits_change_nothing_and_the_raw_call_writes_only_out(gpu):
    """The C entry into a slice of a buffer filled with a sentinel: the slice is cleared and written by the entry itself,
    nothing outside it is touched, and mask bits at or above the set counts change nothing."""
    from ark_analysis_amd import _capi, som_device
    rs = np.random.RandomState(6)
    n_sets_q, n_sets_c = 5, 12
    xy, seg = _points(rs, [300, 0, 70, 515])
    n, n_fovs = len(xy), len(seg) - 1
    clean_q, clean_c = _masks(rs, n, n_sets_q), _masks(rs, n, n_sets_c)
    stray = cpr.pack(rs.rand(n, 64) < 0.5)
    dirty_q = clean_q | (stray & ~np.uint64((1 << n_sets_q) - 1))
    dirty_c = clean_c | (stray & ~np.uint64((1 << n_sets_c) - 1))
    assert (dirty_q != clean_q).any() and (dirty_c >> np.uint64(63)).any()
    s_lim, s_zero = som_device.neighbor_thresholds(50)
    guard, size = 1024, n_fovs * n_sets_q * n_sets_c
    sentinel = 0x5A5A5A5A5A5A5A5A
    xy_d, seg_d = torch.from_numpy(xy).to(gpu), torch.from_numpy(seg).to(gpu)
    results = []
    for mq, mc in ((clean_q, clean_c), (dirty_q, dirty_c)):
        for self_neighbor in (0, 1):
            buf = torch.full((guard + size + guard,), sentinel, dtype=torch.int64, device=gpu)
            mq_d, mc_d = _to(gpu, mq), _to(gpu, mc)
            rc = _capi.lib().pxsom_close_pair_counts(xy_d.data_ptr(), mq_d.data_ptr(), mc_d.data_ptr(), seg_d.data_ptr(),
                                                     n_fovs, n, n_sets_q, n_sets_c, s_lim, s_zero, self_neighbor,
                                                     buf.data_ptr() + guard * 8, _capi.stream_ptr())
            _capi.check(rc, "pxsom_close_pair_counts")
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert (host[:guard] == sentinel).all() and (host[guard + size:] == sentinel).all()
            got = host[guard:guard + size].reshape(n_fovs, n_sets_q, n_sets_c)
            _same(got, cpr.close_pair_counts(xy, clean_q, clean_c, seg, n_sets_q, n_sets_c, 50, bool(self_neighbor)))
            results.append(got)
    _same(results[0], results[2])
    _same(results[1], results[3])
    assert (results[0][1] == 0).all()


def test_counts_beyond_32_bits_in_closed_form(gpu):
    """50 000 distinct cells of one FOV inside a disc of radius < distlim / 2: every pair of distinct cells counts, so
    out[s, t] = |S_s| |S_t| - |S_s and S_t| (with self_neighbor |S_s| |S_t|).  Set 2 holds every cell: 50 000 * 49 999
    is above 2^31."""
    rs = np.random.RandomState(7)
    n = 50000
    cells = rs.permutation(1001 * 1001)[:n]                      # distinct points of a fine grid inside the disc's box
    xy = np.stack([cells // 1001, cells % 1001], 1).astype(np.float64) * (30.0 / 1000) + 100.0
    assert np.hypot(30.0, 30.0) < 50 and len(np.unique(cells)) == n
    member = np.stack([rs.rand(n) < 0.5, rs.rand(n) < 0.1, np.ones(n, dtype=bool)], 1)
    mask = cpr.pack(member)
    seg = np.array([0, n], dtype=np.int64)
    sizes = member.sum(axis=0).astype(np.int64)
    both = member.astype(np.int64).T.dot(member.astype(np.int64))
    for self_neighbor in (False, True):
        got = _device(gpu, xy, mask, mask, seg, 3, 3, 50, self_neighbor)[0]
        _same(got, np.outer(sizes, sizes) - (0 if self_neighbor else both))
    assert n * (n - 1) > 2 ** 31


def test_wrapper_argument_errors(gpu):
    from ark_analysis_amd import som_device
    xy = torch.zeros((4, 2), dtype=torch.float64, device=gpu)
    m = torch.zeros(4, dtype=torch.int64, device=gpu)
    seg = torch.tensor([0, 4], device=gpu)
    with pytest.raises(ValueError, match="float64"):
        som_device.close_pair_counts(xy.float(), m, m, seg, 2, 2, 50)
    with pytest.raises(ValueError, match="member_c"):
        som_device.close_pair_counts(xy, m, m.to(torch.int32), seg, 2, 2, 50)
    with pytest.raises(ValueError, match="member_q"):
        som_device.close_pair_counts(xy, m[:3], m, seg, 2, 2, 50)
    with pytest.raises(ValueError, match="1 .. 64"):
        som_device.close_pair_counts(xy, m, m, seg, 65, 2, 50)
    with pytest.raises(ValueError, match="1 .. 64"):
        som_device.close_pair_counts(xy, m, m, seg, 2, 0, 50)
    with pytest.raises(ValueError, match="offsets"):
        som_device.close_pair_counts(xy, m, m, torch.tensor([0, 3], device=gpu), 2, 2, 50)
    with pytest.raises(ValueError, match="offsets"):
        som_device.close_pair_counts(xy, m, m, torch.tensor([0, 5, 4], device=gpu), 2, 2, 50)


def test_compute_close_cell_num_hip_equals_fixture(gpu):
    tm.check_close_cell_num_cases()


def test_mixing_functions_hip_equal_fixture(gpu):
    tm.check_mixing_cases()


def test_mixing_scores_hip_equal_the_loop(gpu):
    tm.check_mixing_scores_equal_loop()
