"""The neighbourhood matrix on CPU: the numpy statement of pxsom_neighbor_counts (tests/neighborhood_reference.py) against
the g18 fixture of the reference (tests/golden/make_golden_neighborhood.py), the host logic of
ark_analysis_amd.analysis through a host stand-in for the device entry point, the two thresholds, the k-means tables with
injected labels, and the error paths.

The ``check_*`` helpers run unchanged on the GPU box (tests/test_gpu_neighborhood.py) with the real device path."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import neighborhood_reference as nr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = "g18_neighborhood"
RENAMED = {"fov": "sample", "label": "cell_id", "cell_meta_cluster": "pheno", "centroid-0": "cy", "centroid-1": "cx"}
WARNING = "More than 5% of cells have no neighbor within the provided radius"


def _g():
    return np.load(os.path.join(GOLD, FIXTURE + ".npz"), allow_pickle=False)


def load_frame(g, prefix):
    cols = [str(c) for c in g[prefix + "columns"]]
    data = {}
    for i, (col, dtype) in enumerate(zip(cols, g[prefix + "dtypes"])):
        v = g[prefix + "col%d" % i]
        data[col] = np.array(v.tolist(), dtype=object) if str(dtype) == "object" else v.astype(str(dtype))
    idx = g[prefix + "index"]
    index = pd.Index(idx.tolist(), dtype=object) if idx.dtype.kind == "U" else pd.Index(idx)
    df = pd.DataFrame(data, columns=cols, index=index)
    assert [str(t) for t in df.dtypes] == [str(t) for t in g[prefix + "dtypes"]]
    return df


def fixture_case(g, i, master=None):
    """The table, the arguments and the expected (counts, freqs, warnings) of fixture case i."""
    master = load_frame(g, "master_") if master is None else master
    p = "c%d_" % i
    table = pd.concat([master[master["fov"] == str(f)] for f in g[p + "fovs"]], ignore_index=True)
    kwargs = dict(included_fovs=None if bool(g[p + "included_none"]) else [str(f) for f in g[p + "included"]],
                  distlim=g[p + "distlim"].item(), self_neighbor=bool(g[p + "self_neighbor"]))
    if bool(g[p + "renamed"]):
        table = table.rename(columns=RENAMED)
        table.index = np.random.RandomState(i).permutation(len(table)) + 1000
        kwargs.update(fov_col="sample", cell_label_col="cell_id", cell_type_col="pheno", centroid_cols=("cy", "cx"))
    want = load_frame(g, p + "counts_"), load_frame(g, p + "freqs_")
    return table, kwargs, want, [str(w) for w in g[p + "warnings"]]


def check_fixture_cases():
    """create_neighborhood_matrix against every case of the fixture: frames under assert_frame_equal, warnings equal."""
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    g = _g()
    master = load_frame(g, "master_")
    assert int(g["n_cases"]) >= 5
    for i in range(int(g["n_cases"])):
        table, kwargs, want, want_warnings = fixture_case(g, i, master)
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter("always")
            got = na.create_neighborhood_matrix(table, "a directory that is never opened", **kwargs)
        assert [str(w.message) for w in wl if issubclass(w.category, UserWarning)] == want_warnings, i
        for frame, exp in zip(got, want):
            pd.testing.assert_frame_equal(frame, exp, check_exact=True)
    assert any(WARNING in w for i in range(int(g["n_cases"])) for w in g["c%d_warnings" % i])
    assert not len(g["c0_warnings"])


def check_per_fov_function():
    """compute_neighbor_counts on one FOV of the fixture's cohort: sorted phenotype columns (one phenotype is absent from
    fovB), the input's index, freqs = counts / neighbours with 0 for none; and a missing phenotype has no column."""
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    master = load_frame(_g(), "master_")
    for fov, distlim, self_neighbor in (("fovB", 50, False), ("fovA", 37.5, True), ("fovC", 50, False)):
        rows = master[master["fov"] == fov]
        xy = rows[["centroid-0", "centroid-1"]].to_numpy()
        counts, freqs = sau.compute_neighbor_counts(rows, xy, distlim, self_neighbor)
        names = sorted(set(rows["cell_meta_cluster"]))
        assert list(counts.columns) == names == list(freqs.columns)
        assert counts.index.equals(rows.index) and freqs.index.equals(rows.index)
        codes = np.array([names.index(v) for v in rows["cell_meta_cluster"]])
        want = nr.neighbor_counts(xy, codes, [0, len(rows)], len(names), distlim, self_neighbor).astype(np.float64)
        np.testing.assert_array_equal(counts.to_numpy(), want)
        assert counts.to_numpy().dtype == np.float64
        total = want.sum(axis=1, keepdims=True)
        np.testing.assert_array_equal(freqs.to_numpy(), np.where(total > 0, want / np.where(total > 0, total, 1), 0))
    assert len(set(master.loc[master["fov"] == "fovB", "cell_meta_cluster"])) == 4
    rows = master[master["fov"] == "fovD"].copy()
    rows["cell_meta_cluster"] = rows["cell_meta_cluster"].where(rows["cell_meta_cluster"] != "tumor", None)
    xy = rows[["centroid-0", "centroid-1"]].to_numpy()
    counts, _ = sau.compute_neighbor_counts(rows, xy, 50)
    full, _ = sau.compute_neighbor_counts(master[master["fov"] == "fovD"], xy, 50)
    pd.testing.assert_frame_equal(counts, full.drop(columns="tumor"), check_exact=True)


@pytest.fixture
def host_device(monkeypatch):
    from ark_analysis_amd.analysis import spatial_analysis_utils
    monkeypatch.setattr(spatial_analysis_utils, "_neighbor_counts_device", nr.host_stand_in)


# ---- the numpy statement against the reference --------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference is not on this machine")
def test_regenerated_fixture_equals_committed(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_neighborhood.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    a, b = _g(), np.load(os.path.join(str(tmp_path), FIXTURE + ".npz"), allow_pickle=False)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_numpy_statement_equals_fixture():
    """Per included FOV, the statement's counts (cells without a neighbour dropped) are the fixture's rows of that FOV."""
    g = _g()
    master = load_frame(g, "master_")
    for i in range(int(g["n_cases"])):
        table, kwargs, (want_counts, want_freqs), _ = fixture_case(g, i, master)
        fov_col = kwargs.get("fov_col", "fov")
        type_col = kwargs.get("cell_type_col", "cell_meta_cluster")
        cen = list(kwargs.get("centroid_cols", ("centroid-0", "centroid-1")))
        names = list(pd.unique(table[type_col]))
        assert list(want_counts.columns[3:]) == names
        included = kwargs["included_fovs"] or list(pd.unique(table[fov_col]))
        assert set(want_counts[fov_col]) <= set(included)
        for fov in included:
            rows = table[table[fov_col] == fov]
            codes = np.array([names.index(v) for v in rows[type_col]])
            counts = nr.neighbor_counts(rows[cen].to_numpy(), codes, [0, len(rows)], len(names), kwargs["distlim"],
                                        kwargs["self_neighbor"]).astype(np.float64)
            keep = counts.sum(axis=1) != 0
            sel = (want_counts[fov_col] == fov).to_numpy()
            np.testing.assert_array_equal(want_counts.loc[sel, names].to_numpy(), counts[keep])
            np.testing.assert_array_equal(want_freqs.loc[sel, names].to_numpy(),
                                          counts[keep] / counts[keep].sum(axis=1, keepdims=True))


def test_exact_ties_are_excluded_in_the_fixture_grid():
    """The 20 x 20 pitch-10 grid: 3 376 ordered pairs at exactly 50 do not count at distlim 50 and do at 50.000004."""
    g = _g()
    master = load_frame(g, "master_")
    xy = master.loc[master["fov"] == "fovB", ["centroid-0", "centroid-1"]].to_numpy()
    zeros = np.zeros(len(xy), dtype=np.int64)
    at = nr.neighbor_counts(xy, zeros, [0, len(xy)], 1, 50).sum()
    above = nr.neighbor_counts(xy, zeros, [0, len(xy)], 1, float(np.nextafter(np.float32(50), np.float32(60)))).sum()
    assert above - at == int(g["tie_pairs"]) == 3376


# ---- thresholds ---------------------------------------------------------------------------------------------------
DISTLIMS = [50, 37.5, 0.1 + 0.2, 1e-3, 4096, 50.5, 100, np.float32(37.5), np.float64(0.1 + 0.2), np.float64(50),
            np.float32(1e-3), np.float64(1e-3), 1, 2.0 ** -20, 3.0e5]


def _ulps_around(s, span=2000):
    bits = np.array(s, dtype=np.float64).view(np.uint64).astype(np.int64)
    lo = max(int(bits) - span, 0)
    return np.arange(lo, int(bits) + span + 1, dtype=np.int64).astype(np.uint64).view(np.float64)


@pytest.mark.parametrize("distlim", DISTLIMS, ids=lambda d: "%s-%r" % (type(d).__name__, float(d)))
def test_neighbor_thresholds_flip_exactly_where_float32_does(distlim):
    from ark_analysis_amd.som_device import neighbor_thresholds
    s_lim, s_zero = neighbor_thresholds(distlim)
    assert isinstance(s_lim, float) and isinstance(s_zero, float)
    assert (s_lim, s_zero) == nr.thresholds(distlim)
    lim = np.result_type(np.float32, distlim).type(distlim)
    assert lim.dtype == (np.float64 if isinstance(distlim, np.float64) else np.float32)
    for centre in (s_lim, s_zero):
        s = _ulps_around(centre)
        assert s.size >= 2001
        d32 = np.sqrt(s).astype(np.float32)
        np.testing.assert_array_equal(d32 < lim, s < s_lim)
        np.testing.assert_array_equal(d32 == 0, s <= s_zero)
        np.testing.assert_array_equal(d32 != 0, s > s_zero)
    assert 2.0 ** -300 <= s_zero < 2.0 ** -299      # half the smallest float32 subnormal, squared (sqrt rounds first)


def test_neighbor_thresholds_edge_values():
    from ark_analysis_amd.som_device import neighbor_thresholds
    assert neighbor_thresholds(0)[0] == 0.0 and neighbor_thresholds(-3.5)[0] == 0.0     # nothing is < 0
    assert neighbor_thresholds(float("nan"))[0] == 0.0
    s_inf, _ = neighbor_thresholds(float("inf"))
    with np.errstate(over="ignore"):
        assert np.float32(np.sqrt(s_inf)) == np.inf and np.float32(np.sqrt(np.nextafter(s_inf, 0))) < np.inf


# ---- host logic through the stand-in ------------------------------------------------------------------------------
def test_create_neighborhood_matrix_equals_fixture(host_device):
    check_fixture_cases()


def test_compute_neighbor_counts_rules(host_device):
    check_per_fov_function()


def test_dist_mat_dir_is_optional_and_positional_order_is_the_reference_s(host_device):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    g = _g()
    table, kwargs, want, _ = fixture_case(g, 1)
    got = na.create_neighborhood_matrix(table, None, None, 37.5, True, "fov", "label", "cell_meta_cluster")
    pd.testing.assert_frame_equal(got[0], want[0], check_exact=True)
    got = na.create_neighborhood_matrix(table, distlim=37.5, self_neighbor=True)
    pd.testing.assert_frame_equal(got[1], want[1], check_exact=True)


def test_numpy_scalar_distlim_compares_in_its_own_dtype(host_device):
    """np.float64(0.1 + 0.2) * 100 style limits: a float64 scalar compares in float64, a Python float in float32."""
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    table = pd.DataFrame({"fov": "f", "label": [1, 2, 3], "cell_meta_cluster": ["a", "b", "a"],
                          "centroid-0": [0.0, 0.0, 0.0], "centroid-1": [0.0, float(np.float32(0.3)), 5.0]})
    py, _ = na.create_neighborhood_matrix(table, distlim=0.3)                 # float32(0.3) < float32(0.3): no
    f64, _ = na.create_neighborhood_matrix(table, distlim=np.float64(0.3))    # 0.30000001192... < 0.3: no
    up, _ = na.create_neighborhood_matrix(table, distlim=np.float64(0.30000002))
    assert len(py) == 0 and len(f64) == 0
    assert up[["a", "b"]].to_numpy().tolist() == [[0.0, 1.0], [1.0, 0.0]] and list(up["label"]) == [1, 2]


def test_error_paths(host_device):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    g = _g()
    table, _, _, _ = fixture_case(g, 0)
    with pytest.raises(ValueError, match="centroid-1"):
        na.create_neighborhood_matrix(table.drop(columns="centroid-1"))
    with pytest.raises(ValueError, match="cy"):
        na.create_neighborhood_matrix(table, centroid_cols=("cy", "centroid-1"))
    with pytest.raises(ValueError, match="fovZ"):
        na.create_neighborhood_matrix(table, included_fovs=["fovA", "fovZ"])
    counts, _ = na.create_neighborhood_matrix(table)
    with pytest.raises(ValueError, match="Invalid k"):
        na.generate_cluster_matrix_results(table, counts, 1)
    with pytest.raises(ValueError, match="fovZ"):
        na.generate_cluster_matrix_results(table, counts, 3, included_fovs=["fovZ"])
    with pytest.raises(ValueError, match="chanZ"):
        na.generate_cluster_matrix_results(table, counts, 3, excluded_channels=["chanZ"])
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    with pytest.raises(ValueError, match="one .* pair per row"):
        sau.compute_neighbor_counts(table, np.zeros((3, 2)), 50)


def test_fov_rows_and_segments():
    from ark_analysis_amd.analysis._cells import fov_rows_and_segments
    # -1 entries are left out, a FOV's rows keep table order, FOVs 1 and 4 .. 5 (beyond the largest code) are empty
    rows, seg = fov_rows_and_segments(np.array([2, -1, 0, 3, 2, -1, 0, 2]), 6)
    assert rows.tolist() == [2, 6, 0, 4, 7, 3]
    assert seg.tolist() == [0, 2, 2, 5, 6, 6, 6] and seg.dtype == np.int64
    for codes in (np.full(4, -1), np.zeros(0, dtype=np.int64)):      # no wanted rows at all
        rows, seg = fov_rows_and_segments(codes, 3)
        assert rows.size == 0 and seg.tolist() == [0, 0, 0, 0] and seg.dtype == np.int64
    rows, seg = fov_rows_and_segments(np.zeros(0, dtype=np.int64), 0)
    assert rows.size == 0 and seg.tolist() == [0] and seg.dtype == np.int64
    codes = np.random.RandomState(5).randint(-1, 7, size=500)
    rows, seg = fov_rows_and_segments(codes, 9)
    assert seg[-1] == (codes >= 0).sum() and seg.shape == (10,)
    for f in range(9):
        assert np.array_equal(rows[seg[f]:seg[f + 1]], np.flatnonzero(codes == f))      # ascending: table order


@pytest.mark.parametrize("who,table_name", [("create_neighborhood_matrix", "all_data"),
                                            ("compute_mixing_scores", "cell_table"),
                                            ("generate_cell_distance_analysis", "cell_table")])
def test_centroid_check_names_the_missing_column_in_each_caller_s_words(who, table_name):
    from ark_analysis_amd.analysis._cells import centroid_columns
    table = pd.DataFrame({"centroid-0": [1, 2], "cx": [3.5, 4.0]})
    with pytest.raises(ValueError) as err:
        centroid_columns(table, ("centroid-0", "centroid-1"), who, table_name)
    assert str(err.value) == ("%s needs two centroid columns in %s; missing: ['centroid-1'] (pass centroid_cols=... if "
                              "they are named differently)" % (who, table_name))
    with pytest.raises(ValueError, match=r"%s needs two centroid columns in %s; missing: \['cx'\]" % (who, table_name)):
        centroid_columns(table, ("cx",), who, table_name)      # not two columns: the ones given are named
    assert centroid_columns(table, ("centroid-0", "cx"), who, table_name) == ["centroid-0", "cx"]


def test_device_entry_point_is_loud_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    table, _, _, _ = fixture_case(_g(), 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        na.create_neighborhood_matrix(table)


# ---- k-means tables -----------------------------------------------------------------------------------------------
def check_cluster_matrix_results(monkeypatch_setattr):
    """generate_cluster_matrix_results with the fixture's labels injected equals the fixture's three frames."""
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    g = _g()
    table, kwargs, _, _ = fixture_case(g, int(g["k_case"]))
    counts, _ = na.create_neighborhood_matrix(table, **kwargs)
    seen = {}

    def injected(data, cluster_num, seed=42):
        seen.update(shape=data.shape, k=cluster_num, seed=seed, columns=list(data.columns))
        return g["k_labels"].copy()
    monkeypatch_setattr(sau, "generate_cluster_labels", injected)
    got = na.generate_cluster_matrix_results(table, counts, int(g["k_num"]), seed=int(g["k_seed"]),
                                             excluded_channels=[str(c) for c in g["k_excluded"]])
    assert seen == dict(shape=(len(counts), counts.shape[1] - 3), k=int(g["k_num"]), seed=int(g["k_seed"]),
                        columns=list(counts.columns[3:]))
    for frame, tag in zip(got, ("cells", "per_type", "means")):
        want = load_frame(g, "k_%s_" % tag)
        if tag == "per_type":
            want.columns.name = "cell_meta_cluster"
        pd.testing.assert_frame_equal(frame, want, check_exact=True)
    assert "kmeans_neighborhood" in got[0].columns and "chanB" not in got[2].columns
    return got


def test_cluster_matrix_results_with_injected_labels(host_device, monkeypatch):
    check_cluster_matrix_results(monkeypatch.setattr)


def test_generate_cluster_labels_is_sklearn_kmeans():
    from sklearn.cluster import KMeans
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    g = _g()
    counts = load_frame(g, "c0_counts_")
    data = counts.drop(columns=["fov", "label", "cell_meta_cluster"])
    for k, seed in ((3, 42), (5, 7)):
        labels = sau.generate_cluster_labels(data, k, seed=seed)
        want = KMeans(n_clusters=k, random_state=seed, n_init=10).fit(data).labels_ + 1
        np.testing.assert_array_equal(labels, want)
        assert labels.min() == 1 and labels.max() == k and len(labels) == len(data)


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_symbol_exported_and_abi_unchanged():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    assert "pxsom_neighbor_counts" in _capi.SYMBOLS and hasattr(lib, "pxsom_neighbor_counts")
    assert lib.pxsom_abi_version() == _capi.ABI_VERSION == 9
    # rejected before any HIP call
    assert lib.pxsom_neighbor_counts(None, None, None, 1, -1, 3, 1.0, 0.0, 0, None, None) == -1
    assert b"n=-1" in lib.pxsom_last_error()
    assert lib.pxsom_neighbor_counts(None, None, None, 1, 4, 0, 1.0, 0.0, 0, None, None) == -1
    assert lib.pxsom_neighbor_counts(None, None, None, 1, 4, 3, 1.0, 0.0, 2, None, None) == -1
    assert lib.pxsom_neighbor_counts(None, None, None, 1, 4, 3, float("nan"), 0.0, 0, None, None) == -1
    assert lib.pxsom_neighbor_counts(None, None, None, 1, 4, 3, 1.0, 0.0, 0, None, None) == -1
    assert b"null" in lib.pxsom_last_error()


# ---- the fuzz generator of tests/test_gpu_fuzz_neighborhood.py ----------------------------------------------------
def test_fuzz_generator_visits_every_class_and_means_something():
    from tests import test_gpu_fuzz_neighborhood as fz
    seen, ties, scalar_types = set(), 0, set()
    for i in range(len(fz.CLASSES)):
        c = fz.gen_case(i)
        again = fz.gen_case(i)
        assert all(np.array_equal(c[k], again[k]) for k in ("xy", "types", "seg")) and c["distlim"] == again["distlim"]
        n = len(c["xy"])
        assert c["xy"].shape == (n, 2) and c["xy"].dtype == np.float64 and c["types"].shape == (n,)
        assert c["seg"][0] == 0 and c["seg"][-1] == n and (np.diff(c["seg"]) >= 0).all()
        assert n == 0 or (0 <= c["types"].min() and c["types"].max() < c["n_types"])
        assert type(c["distlim"]) is fz.SCALAR[c["cls"][0]] and c["distlim"] > 0
        seen.add(c["cls"])
        scalar_types.add(type(c["distlim"]))
        counts = nr.neighbor_counts(c["xy"], c["types"], c["seg"], c["n_types"], c["distlim"], c["self_neighbor"])
        wider = nr.neighbor_counts(c["xy"], c["types"], c["seg"], c["n_types"],
                                   np.nextafter(np.float32(c["distlim"]), np.float32(np.inf)), c["self_neighbor"])
        assert n == 0 or counts.sum() > 0, (i, c["cls"])
        ties += int(wider.sum() - counts.sum()) if c["cls"][2] == "lattice" else 0
    assert seen == set(fz.CLASSES) and scalar_types == {int, float, np.float32, np.float64}
    assert ties > 100        # the lattices put pairs at exactly distlim
