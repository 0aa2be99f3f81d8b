"""pxsom_silhouette on the GPU (som_device.silhouette_samples / silhouette_scores) against the numpy statement of
tests/silhouette_reference.py within the derived bound of tests/test_silhouette.py (|delta s_i| <= 8 (n + d) 2^-53,
|delta score| <= 9 (n + d) 2^-53), against sklearn's recorded samples, and compute_cluster_metrics_silhouette end to end."""
import numpy as np
import pytest
import torch

from tests import silhouette_reference as sr
from tests import test_silhouette as ts

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 255, 256, 257, 513, 1000]
DIMS = [1, 2, 7, 8, 9, 33, 64]
KS = [2, 3, 10, 32]


def _device(gpu, x, labelings, n_clusters, label_dtype=torch.int64):
    """(samples [M, n], scores [M]) of one call with every labeling."""
    from ark_analysis_amd import som_device
    x_d = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(gpu)
    lab_d = torch.from_numpy(np.ascontiguousarray(labelings)).to(gpu).to(label_dtype)
    samples = som_device.silhouette_samples(x_d, lab_d, n_clusters)
    scores = som_device.silhouette_scores(x_d, lab_d, n_clusters)
    torch.cuda.synchronize()
    assert samples.dtype == torch.float64 and tuple(samples.shape) == tuple(lab_d.shape)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (1 if lab_d.dim() == 1 else len(lab_d),)
    return samples.cpu().numpy(), scores.cpu().numpy()


def _check(got, x, labelings, n_clusters, what=""):
    samples, scores = got
    n, d = x.shape
    want = sr.silhouette_samples_for(x, labelings, n_clusters)
    gap = np.abs(samples - want).max()
    score_gap = max(abs(s - sr.score(w)) for s, w in zip(scores, want))
    print("%s n=%d d=%d: max |delta s| = %.3g (bound %.3g), max |delta score| = %.3g (bound %.3g)"
          % (what, n, d, gap, sr.sample_bound(n, d), score_gap, sr.score_bound(n, d)))
    assert not np.isnan(samples).any()
    assert gap <= sr.sample_bound(n, d), what
    assert score_gap <= sr.score_bound(n, d), what
    return want


def _labeling(rs, n, k):
    """n labels in [0, k) in no order: skewed shares (so the largest cluster outgrows a tile at the larger n), cluster
    k - 1 a singleton where there is room for one."""
    share = rs.dirichlet(np.full(k, 0.5))
    lab = rs.choice(k, n, p=share)
    if n > 2:
        lab[lab == k - 1] = 0
        lab[rs.randint(n)] = k - 1
    return lab.astype(np.int64)


def _rows(rs, n, d, kind):
    if kind == "counts":            # small integers: many duplicate rows
        return rs.poisson(1.5, size=(n, d)).astype(np.float64)
    return rs.standard_normal((n, d)) * 10.0 ** rs.randint(-2, 3)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_statement(gpu, n, d):
    """Every k of KS as one labeling each of a single call; rows as counts for odd d, as reals for even d."""
    rs = np.random.RandomState(100 * n + d)
    x = _rows(rs, n, d, "counts" if d % 2 else "reals")
    labelings = np.stack([_labeling(rs, n, k) for k in KS])
    got = _device(gpu, x, labelings, KS, torch.int32 if n % 2 else torch.int64)
    want = _check(got, x, labelings, KS)
    if n > 2:
        for lab, k, s, w in zip(labelings, KS, got[0], want):
            assert (lab == k - 1).sum() == 1 and s[lab == k - 1] == 0 and w[lab == k - 1] == 0      # the singleton
    if n == 1000:
        assert np.bincount(labelings[0]).max() >= 257          # longer than a tile of any row width


@pytest.mark.parametrize("d", [7, 20, 40])
def test_runs_that_straddle_tiles(gpu, d):
    """Cluster sizes around the tile lengths (256 candidates up to d = 16, 128 up to 32, 64 beyond), so runs start and
    end inside, at and just past a tile boundary; rows of a cluster scattered over the matrix."""
    rs = np.random.RandomState(d)
    sizes = [63, 1, 64, 65, 127, 129, 255, 257, 40]
    lab = rs.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int64)
    x = _rows(rs, len(lab), d, "counts")
    _check(_device(gpu, x, lab[None, :], [len(sizes)]), x, lab[None, :], [len(sizes)])
    single = _device(gpu, x, lab, len(sizes))                 # labels as [n]: samples [n], scores [1]
    assert single[0].shape == (len(lab),) and single[1].shape == (1,)


def test_identical_rows_score_zero(gpu):
    x = np.tile(np.array([[1 / 3, 2 / 7, 5.0]]), (300, 1))
    lab = np.random.RandomState(1).randint(0, 4, 300)
    samples, scores = _device(gpu, x, lab[None, :], [4])
    assert (samples == 0).all() and (scores == 0).all()


def test_tight_cluster_beside_a_distant_one_scores_one(gpu):
    """270 copies of one row against 40 scattered far away: a = 0 exactly, so s = 1 exactly on the copies."""
    rs = np.random.RandomState(2)
    x = np.concatenate([np.tile(rs.uniform(0, 1, (1, 9)), (270, 1)), 100 + rs.uniform(0, 1, (40, 9))])
    lab = np.concatenate([np.zeros(270), np.ones(40)]).astype(np.int64)
    perm = rs.permutation(310)
    x, lab = x[perm], lab[perm]
    got = _device(gpu, x, lab[None, :], [2])
    assert (got[0][0][lab == 0] == 1).all()
    _check(got, x, lab[None, :], [2])


@pytest.fixture(scope="module")
def sweep():
    rs = np.random.RandomState(9)
    x = rs.poisson(2.0, size=(600, 20)).astype(np.float64)
    ks = list(range(2, 11))
    return x, np.stack([rs.randint(0, k, 600) for k in ks]), ks


def test_nine_labelings_in_one_call_equal_nine_calls_bit_for_bit(gpu, sweep):
    x, labelings, ks = sweep
    together = _device(gpu, x, labelings, ks)
    _check(together, x, labelings, ks, "M=9")
    for m, k in enumerate(ks):
        alone = _device(gpu, x, labelings[m:m + 1], [k])
        np.testing.assert_array_equal(alone[0][0].view(np.uint64), together[0][m].view(np.uint64))
        np.testing.assert_array_equal(alone[1].view(np.uint64), together[1][m:m + 1].view(np.uint64))


def test_same_call_twice_gives_the_same_bits(gpu, sweep):
    x, labelings, ks = sweep
    a, b = _device(gpu, x, labelings, ks), _device(gpu, x, labelings, ks)
    np.testing.assert_array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    np.testing.assert_array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


@pytest.mark.parametrize("name", ts.INPUTS)
def test_golden_fixture(gpu, name):
    """Integer inputs: within the bound of sklearn's samples.  Frequencies: as near to sklearn as the statement is, plus
    the bound."""
    g = ts.fixture()
    ks = [int(k) for k in g["ks"]]
    labelings = np.stack([g["%s_labels_k%d" % (name, k)] for k in ks])
    samples, _ = _device(gpu, g[name + "_x"], labelings, ks)
    skl, bound = ts.fixture_sklearn(name), sr.sample_bound(700, 7)
    print("%s: max |device - sklearn| = %.3g" % (name, np.abs(samples - skl).max()))
    if name in ts.INTEGER_INPUTS:
        assert np.abs(samples - skl).max() <= bound
    else:
        assert (np.abs(samples - skl) <= np.abs(ts.fixture_reference(name) - skl) + bound).all()
    assert np.abs(samples - ts.fixture_reference(name)).max() <= bound


def test_guards(gpu):
    from ark_analysis_amd import _capi, som_device
    x = torch.zeros((6, 3), dtype=torch.float64, device=gpu)
    lab = torch.zeros(6, dtype=torch.int64, device=gpu)
    for fn in (som_device.silhouette_samples, som_device.silhouette_scores):
        with pytest.raises(ValueError, match="64"):
            fn(torch.zeros((6, 65), dtype=torch.float64, device=gpu), lab, 2)
        with pytest.raises(ValueError, match="32"):
            fn(x, lab, 33)
        with pytest.raises(ValueError, match="n >= 2"):
            fn(x[:1], lab[:1], 2)
        with pytest.raises(ValueError, match="float64"):
            fn(x.float(), lab, 2)
        with pytest.raises(ValueError, match="device"):
            fn(x, lab.cpu(), 2)
        with pytest.raises(ValueError, match="n_clusters"):
            fn(x, lab + 2, 2)
    out = torch.zeros(64, dtype=torch.float64, device=gpu)
    lab32 = lab.int()
    args = (lab32.data_ptr(), lab32.data_ptr(), 1)
    tail = (out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), _capi.stream_ptr())
    for n, d, k, what in ((6, 65, 2, b"64"), (6, 3, 33, b"32"), (1, 3, 2, b"n=1")):
        assert _capi.lib().pxsom_silhouette(x.data_ptr(), n, d, *args, k, *tail) == -1
        assert what in _capi.lib().pxsom_last_error()


def _raw_call(gpu, x, lab, order, k, guard=1024, sentinel=0x5A5A5A5A):
    """pxsom_silhouette into slices of buffers filled with a sentinel: (counts, sums, samples, scores) and whether every
    guard word on both sides of the four outputs is untouched."""
    from ark_analysis_amd import _capi
    n, d = x.shape
    x_d = torch.from_numpy(x).to(gpu)
    lab_d, ord_d = torch.from_numpy(lab.astype(np.int32)).to(gpu), torch.from_numpy(order.astype(np.int32)).to(gpu)
    words = [k, 2 * n * k, 2 * n, 2]            # int32 words of counts, sums, samples, scores
    bufs = [torch.full((guard + w + guard,), sentinel, dtype=torch.int32, device=gpu) for w in words]
    ptrs = [b.data_ptr() + guard * 4 for b in bufs]
    rc = _capi.lib().pxsom_silhouette(x_d.data_ptr(), n, d, lab_d.data_ptr(), ord_d.data_ptr(), 1, k, *ptrs,
                                      _capi.stream_ptr())
    _capi.check(rc, "pxsom_silhouette")
    torch.cuda.synchronize()
    hosts = [b.cpu().numpy() for b in bufs]
    intact = all((h[:guard] == sentinel).all() and (h[guard + w:] == sentinel).all() for h, w in zip(hosts, words))
    inner = [h[guard:guard + w].copy() for h, w in zip(hosts, words)]
    return (inner[0], inner[1].view(np.float64).reshape(n, k), inner[2].view(np.float64), inner[3].view(np.float64)), intact


def test_raw_call_with_labels_out_of_range_touches_nothing_else(gpu):
    """The C entry with labels outside [0, k) and entries of `order` outside [0, n): the call returns, the guard words
    around every output are intact, and a correct call after it gives the rows of a correct call before it."""
    rs = np.random.RandomState(8)
    n, d, k = 700, 7, 5
    x = rs.poisson(2.0, size=(n, d)).astype(np.float64)
    lab = rs.randint(0, k, n)
    order = np.argsort(lab, kind="stable")
    before, intact = _raw_call(gpu, x, lab, order, k)
    assert intact
    np.testing.assert_array_equal(before[0], np.bincount(lab, minlength=k))
    want = sr.silhouette_samples(x, lab, k)
    assert np.abs(before[2] - want).max() <= sr.sample_bound(n, d)
    sums = sr.cluster_sums(x, lab, k)
    assert (np.abs(before[1] - sums) <= (n + d + 3) * sr.U * sums).all()      # (d + 3) u a distance, (n - 1) u the sum

    bad = lab.copy()
    bad[[0, 17, 300, 699]] = [k, -1, 2 ** 31 - 1, -2 ** 31]
    bad_order = np.argsort(bad, kind="stable")
    bad_order[[5, 400]] = [n, -7]
    got, intact = _raw_call(gpu, x, bad, bad_order, k)
    assert intact
    assert got[0].sum() == n - 4 and np.isnan(got[2][[0, 17, 300, 699]]).all()

    after, intact = _raw_call(gpu, x, lab, order, k)
    assert intact
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                      b.view(np.uint64) if b.dtype == np.float64 else b)


@pytest.mark.parametrize("subsample", [None, 50])
def test_compute_cluster_metrics_silhouette_hip(gpu, monkeypatch, subsample):
    """Three FOVs, about 600 cells: every device call of the sweep against the stand-in on the same arrays."""
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    real, calls = sau._silhouette_device, []

    def both(x, labelings, n_clusters):
        got, want = real(x, labelings, n_clusters), sr.host_stand_in(x, labelings, n_clusters)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= sr.score_bound(*np.shape(x))
        calls.append(got)
        return got
    monkeypatch.setattr(sau, "_silhouette_device", both)
    got = na.compute_cluster_metrics_silhouette(ts.neighborhood_matrix(), min_k=2, max_k=6, subsample=subsample)
    ts._check_series(got, 2, 6)
    assert len(calls) == (1 if subsample is None else 5)
    np.testing.assert_array_equal(got.values, np.concatenate(calls))
    assert (np.abs(got.values) <= 1).all() and got.values.max() > 0.1
