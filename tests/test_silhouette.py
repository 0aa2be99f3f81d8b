"""K15 on the CPU: the numpy statement of tests/silhouette_reference.py against sklearn's recorded silhouette_samples
(tests/golden/silhouette_sklearn.npz, tests/golden/make_golden_silhouette.py), the host logic of the two k sweeps with the
device entry point swapped for the statement, and the ABI.

Tolerance (derived, silhouette_reference.sample_bound): both sides compute a distance within (d + 3) u, u = 2^-53; a sum of
n of them in any order adds (n - 1) u; a, b and the quotient add a few more; |s| <= 1: |delta s_i| <= 8 (n + d) u and
|delta score| <= 9 (n + d) u."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from tests import silhouette_reference as sr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = "silhouette_sklearn"
INTEGER_INPUTS, INPUTS = ("counts", "distinct"), ("counts", "freqs", "distinct")
_CACHE = {}


def fixture():
    if "g" not in _CACHE:
        with np.load(os.path.join(GOLD, FIXTURE + ".npz"), allow_pickle=False) as z:
            _CACHE["g"] = {k: z[k] for k in z.files}
    return _CACHE["g"]


def fixture_reference(name):
    """The statement's [3, n] samples of one fixture input under its three labelings (computed once per process)."""
    if name not in _CACHE:
        g = fixture()
        ks = [int(k) for k in g["ks"]]
        _CACHE[name] = sr.silhouette_samples_for(g[name + "_x"], [g["%s_labels_k%d" % (name, k)] for k in ks], ks)
        _CACHE[name].setflags(write=False)
    return _CACHE[name]


def fixture_sklearn(name):
    g = fixture()
    return np.stack([g["%s_samples_k%d" % (name, int(k))] for k in g["ks"]])


# ---- the fixture and the statement --------------------------------------------------------------------------------
def test_regenerated_fixture_equals_committed(tmp_path):
    """Inputs, labels and the samples of the integer inputs are equal; the samples of the frequencies, where sklearn's
    expansion cancels and a BLAS build may round another way, agree within the cap test_statement... puts on that error."""
    pytest.importorskip("sklearn")
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_silhouette.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    a, b = fixture(), np.load(os.path.join(str(tmp_path), FIXTURE + ".npz"), allow_pickle=False)
    assert sorted(a) == sorted(b.files)
    for key in a:
        if key.startswith("freqs_samples"):
            np.testing.assert_allclose(a[key], b[key], rtol=0, atol=1e-8, err_msg=key)
        else:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_fixture_holds_the_inputs_it_is_meant_to():
    g = fixture()
    assert [int(k) for k in g["ks"]] == [2, 5, 10]
    for name in INPUTS:
        assert g[name + "_x"].shape == (700, 7) and g[name + "_x"].dtype == np.float64
        for k in (2, 5, 10):
            lab = g["%s_labels_k%d" % (name, k)]
            assert lab.dtype == np.int32 and sorted(np.unique(lab)) == list(range(k))
            assert g["%s_samples_k%d" % (name, k)].shape == (700,)
    for name in INTEGER_INPUTS:
        assert (g[name + "_x"] == np.round(g[name + "_x"])).all()
    np.testing.assert_array_equal(g["freqs_x"], g["counts_x"] / g["counts_x"].sum(axis=1, keepdims=True))
    assert len(np.unique(g["distinct_x"], axis=0)) == 12
    assert len(np.unique(g["counts_x"], axis=0)) < 700        # duplicate rows are the common case


@pytest.mark.parametrize("name", INTEGER_INPUTS)
def test_statement_equals_sklearn_on_integers(name):
    ref, skl = fixture_reference(name), fixture_sklearn(name)
    gap = np.abs(ref - skl).max()
    print("%s: max |statement - sklearn| = %.3g, bound %.3g" % (name, gap, sr.sample_bound(700, 7)))
    assert gap <= sr.sample_bound(700, 7)


def test_statement_against_sklearn_on_frequencies():
    """sklearn's expansion loses digits here: the gap is recorded, and capped only for sanity."""
    gap = np.abs(fixture_reference("freqs") - fixture_sklearn("freqs")).max()
    print("freqs: max |statement - sklearn| = %.3g" % gap)
    assert gap < 1e-8


def test_statement_rules():
    """A singleton scores 0, identical rows score 0, a tight cluster beside a distant one scores 1 where a = 0."""
    x = np.array([[0.0, 0], [0, 0], [0, 0], [10, 0], [10, 0], [3, 4]])
    s = sr.silhouette_samples(x, [0, 0, 0, 1, 1, 2], 3)
    assert (s[:5] == 1).all() and s[5] == 0
    assert (sr.silhouette_samples(np.ones((9, 3)), np.arange(9) % 2, 2) == 0).all()
    assert (sr.silhouette_samples(x, [0, 0, 0, 3, 3, 1], 4)[:5] == 1).all()      # an empty cluster is no neighbour
    np.testing.assert_array_equal(sr.cluster_sums(x, [0, 0, 0, 1, 1, 2], 3)[5], [15.0, 2 * np.sqrt(65.0), 0.0])


# ---- the public functions through the stand-in --------------------------------------------------------------------
def neighborhood_matrix(n_per_fov=(210, 190, 200), seed=3):
    rs = np.random.RandomState(seed)
    frames = []
    for f, m in enumerate(n_per_fov):
        centre = rs.choice([0.5, 3.0, 8.0], size=(4, 6))
        counts = rs.poisson(centre[rs.randint(0, 4, m)]).astype(np.float64)
        frame = pd.DataFrame(counts, columns=["type%d" % t for t in range(6)])
        frame.insert(0, "cell_meta_cluster", rs.choice(["a", "b", "c"], m))
        frame.insert(0, "label", np.arange(1, m + 1))
        frame.insert(0, "fov", "fov%d" % f)
        frames.append(frame)
    return pd.concat(frames, ignore_index=True)


@pytest.fixture
def host_device(monkeypatch):
    from ark_analysis_amd.analysis import spatial_analysis_utils
    calls = []

    def counting(x, labelings, n_clusters):
        calls.append((np.array(x), np.array(labelings), list(n_clusters)))
        return sr.host_stand_in(x, labelings, n_clusters)
    monkeypatch.setattr(spatial_analysis_utils, "_silhouette_device", counting)
    return calls


@pytest.fixture
def fits(monkeypatch):
    """Every KMeans the product fits, in order.  A second fit of the same data may differ from the first in the last bit
    of its inertia (the threads of scikit-learn's reduction), so the tests read the product's own fits."""
    import sklearn.cluster
    made, real = [], sklearn.cluster.KMeans

    def recorded(*args, **kwargs):
        made.append((real(*args, **kwargs), args, kwargs))
        return made[-1][0]
    monkeypatch.setattr(sklearn.cluster, "KMeans", recorded)
    return made


def _check_fits(fits, ks, seed, data):
    assert [(args, kwargs) for _, args, kwargs in fits] == [((), dict(n_clusters=k, random_state=seed, n_init="auto"))
                                                            for k in ks]
    for fit, _, _ in fits:
        assert fit.n_features_in_ == data.shape[1] and len(fit.labels_) == len(data)
        np.testing.assert_array_equal(fit.predict(data), fit.labels_)         # fitted on these very rows


def _check_series(series, min_k, max_k):
    assert isinstance(series, pd.Series) and series.dtype == np.float64
    assert series.index.name == "cluster_num" and list(series.index) == list(range(min_k, max_k + 1))
    assert series.loc[min_k] == series.values[0]


def test_silhouette_sweep_is_one_device_call(host_device, fits):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    mat = neighborhood_matrix()
    got = na.compute_cluster_metrics_silhouette(mat, min_k=2, max_k=5, included_fovs=["fov0", "fov2"])
    _check_series(got, 2, 5)
    assert len(host_device) == 1
    x, labelings, ks = host_device[0]
    data = mat[mat["fov"].isin(["fov0", "fov2"])].drop(["fov", "label", "cell_meta_cluster"], axis=1)
    np.testing.assert_array_equal(x, data.to_numpy())              # the id columns are gone, the other FOV too
    assert labelings.shape == (4, len(data)) and ks == [2, 3, 4, 5]
    _check_fits(fits, ks, 42, data)
    for row, (fit, _, _) in zip(labelings, fits):
        np.testing.assert_array_equal(row, fit.labels_)
    from sklearn.metrics import silhouette_score
    want = [silhouette_score(data, row, metric="euclidean") for row in labelings]
    assert np.abs(got.values - want).max() <= sr.score_bound(len(data), 6)      # integer counts: sklearn is exact
    default = na.compute_cluster_metrics_silhouette(mat[mat["fov"] == "fov1"], max_k=3)
    _check_series(default, 2, 3)


def test_silhouette_subsample_equals_the_pandas_calls(host_device, fits):
    import warnings
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    data = neighborhood_matrix((150,)).drop(["fov", "label", "cell_meta_cluster"], axis=1)
    data.iloc[:3] = 40.0                           # a cluster of three cells: smaller than the subsample
    got = sau.compute_kmeans_silhouette(data, min_k=3, max_k=4, seed=7, subsample=20)
    _check_series(got, 3, 4)
    assert len(host_device) == 2                  # the rows differ per k: one call each
    replaced = False
    _check_fits(fits, (3, 4), 7, data)
    for (x, labelings, ks), k, (fit, _, _) in zip(host_device, (3, 4), fits):
        sub = data.copy()
        sub["cluster"] = fit.labels_
        replaced |= bool((sub["cluster"].value_counts() < 20).any())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sub = sub.groupby("cluster").apply(
                lambda g: g.sample(20, replace=len(g) < 20, random_state=7)).reset_index(drop=True)
        assert len(sub) == 20 * k and ks == [k]
        np.testing.assert_array_equal(x, sub.drop("cluster", axis=1).to_numpy())
        np.testing.assert_array_equal(labelings, sub["cluster"].to_numpy()[None, :])
    assert replaced


def test_inertia_is_kmeans_inertia(fits):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    mat = neighborhood_matrix((120, 80))
    got = na.compute_cluster_metrics_inertia(mat, min_k=2, max_k=4, seed=5, included_fovs=["fov1"])
    _check_series(got, 2, 4)
    data = mat[mat["fov"] == "fov1"].drop(["fov", "label", "cell_meta_cluster"], axis=1)
    _check_fits(fits, (2, 3, 4), 5, data)
    np.testing.assert_array_equal(got.values, [fit.inertia_ for fit, _, _ in fits])
    centres = fits[1][0].cluster_centers_          # and inertia_ is what it says: squared distances to the nearest centre
    nearest = ((data.to_numpy()[:, None, :] - centres[None]) ** 2).sum(axis=2).min(axis=1).sum()
    np.testing.assert_allclose(got.loc[3], nearest, rtol=1e-12)


def test_sweep_error_paths(host_device):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    mat = neighborhood_matrix((60, 40))
    for fn in (na.compute_cluster_metrics_inertia, na.compute_cluster_metrics_silhouette):
        for bad in (dict(min_k=1), dict(max_k=1), dict(min_k=0, max_k=3)):
            with pytest.raises(ValueError, match="Invalid k provided for clustering"):
                fn(mat, **bad)
        with pytest.raises(ValueError):
            fn(mat, included_fovs=["fov0", "fov9"])
    data = mat.drop(["fov", "label", "cell_meta_cluster"], axis=1)
    holed = data.copy()
    holed.iloc[5, 2] = np.nan
    with pytest.raises(ValueError):
        sau.compute_kmeans_silhouette(holed, max_k=3)
    holed.iloc[5, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinite"):
        sau.compute_kmeans_silhouette(holed, max_k=3)
    assert host_device == []
    with pytest.raises(ValueError, match="Number of labels is 1"):
        sau._encode_labels(np.zeros(10), 10)
    with pytest.raises(ValueError, match="Number of labels is 4"):
        sau._encode_labels(np.arange(4), 4)
    codes, k = sau._encode_labels(np.array([7, 3, 7, 9]), 4)
    assert list(codes) == [1, 0, 1, 2] and k == 3


def test_device_entry_point_is_loud_without_gpu():
    import torch
    if torch.cuda.is_available():
        return          # nothing to refuse where a HIP device is visible
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    with pytest.raises(RuntimeError, match="no HIP device"):
        sau._silhouette_device(np.zeros((4, 2)), np.array([[0, 0, 1, 1]]), [2])


# ---- ABI and the host-side argument checks ------------------------------------------------------------------------
def test_symbol_exported_and_abi_unchanged():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    assert "pxsom_silhouette" in _capi.SYMBOLS and hasattr(lib, "pxsom_silhouette")
    assert lib.pxsom_abi_version() == _capi.ABI_VERSION == 9


def test_entry_point_rejects_sizes_beyond_the_limits_before_any_hip_call():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    one = 8          # any non-null address: the checks come first and nothing is dereferenced
    for n, d, k, what in ((10, 65, 2, b"64"), (10, 0, 2, b"64"), (10, 3, 33, b"32"), (10, 3, 1, b"32"), (1, 3, 2, b"n=1")):
        rc = lib.pxsom_silhouette(one, n, d, one, one, 1, k, one, one, one, one, None)
        assert rc == -1 and what in lib.pxsom_last_error()
    assert lib.pxsom_silhouette(None, 10, 3, one, one, 1, 2, one, one, one, one, None) == -1


def test_som_device_argument_errors_on_host_tensors():
    import torch
    from ark_analysis_amd import som_device
    assert som_device.SILHOUETTE_MAX_D == 64 and som_device.SILHOUETTE_MAX_K == 32
    x, lab = torch.zeros((6, 3), dtype=torch.float64), torch.zeros(6, dtype=torch.int64)
    for fn in (som_device.silhouette_samples, som_device.silhouette_scores):
        with pytest.raises(ValueError, match="float64"):
            fn(x.float(), lab, 2)
        with pytest.raises(ValueError, match="labels"):
            fn(x, lab[:5], 2)
        with pytest.raises(ValueError, match="labels"):
            fn(x, lab.double(), 2)
        with pytest.raises(ValueError, match="64"):
            fn(torch.zeros((6, 65), dtype=torch.float64), lab, 2)
        for k in (1, 33):
            with pytest.raises(ValueError, match="32"):
                fn(x, lab, k)
        with pytest.raises(ValueError, match="per labeling"):
            fn(x, torch.zeros((3, 6), dtype=torch.int32), [2, 3])
        with pytest.raises(ValueError, match="n >= 2"):
            fn(x[:1], lab[:1], 2)
        with pytest.raises(ValueError, match="HBM"):        # a host tensor: refused like nearest_type_means refuses it
            fn(x, lab, 2)
