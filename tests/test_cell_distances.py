"""The cell-distance and diversity analysis on CPU: the numpy statement of pxsom_nearest_type_means
(tests/cell_distance_reference.py) against the g19 fixture of the reference (tests/golden/make_golden_cell_distances.py),
the host logic of ark_analysis_amd.analysis.cell_neighborhood_stats through a host stand-in for the device entry point,
numpy's float32 row-sum order, the diversity functions against a literal per-cell loop, and the error paths.

The ``check_*`` helpers run unchanged on the GPU box (tests/test_gpu_cell_distances.py) with the real device path."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from tests import cell_distance_reference as cr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = "g19_cell_distances"
RENAMED = {"fov": "sample", "label": "cell_id", "cell_meta_cluster": "pheno", "centroid-0": "cy", "centroid-1": "cx"}
IDS = ["fov", "label", "cell_meta_cluster"]


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_float32(got, want, msg=""):
    """float32 arrays equal bit for bit, NaN in the same places (any NaN payload)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, msg)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=msg)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok], err_msg=msg)


def fixture_case(g, i, master=None):
    """The table, the arguments and the expected (returned, re-read from the CSV) frames of fixture case i."""
    master = load_frame(g, "master_") if master is None else master
    p = "c%d_" % i
    table = pd.concat([master[master["fov"] == str(f)] for f in g[p + "fovs"]], ignore_index=True)
    kwargs = dict(k=int(g[p + "k"]))
    if bool(g[p + "renamed"]):
        table = table.rename(columns=RENAMED)
        table.index = np.random.RandomState(i).permutation(len(table)) + 1000
        kwargs.update(fov_col="sample", cell_label_col="cell_id", cell_type_col="pheno", centroid_cols=("cy", "cx"))
    return table, kwargs, (load_frame(g, p + "dists_"), load_frame(g, p + "saved_"))


def check_fixture_cases(tmp_dir):
    """generate_cell_distance_analysis against every case of the fixture: the returned frame and the CSV it wrote."""
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    g = _g()
    master = load_frame(g, "master_")
    assert int(g["n_cases"]) >= 5 and sorted(int(g["c%d_k" % i]) for i in range(int(g["n_cases"]))) == [1, 5, 5, 8, 13]
    for i in range(int(g["n_cases"])):
        table, kwargs, (want, want_saved) = fixture_case(g, i, master)
        k = kwargs.pop("k")
        path = os.path.join(str(tmp_dir), "dists_%d.csv" % i)
        got = cns.generate_cell_distance_analysis(table, "a directory that is never opened", path, k, **kwargs)
        pd.testing.assert_frame_equal(got, want, check_exact=True)
        pd.testing.assert_frame_equal(pd.read_csv(path), want_saved, check_exact=True)
        assert want.iloc[:, 3:].isna().to_numpy().any() and (want.dtypes.iloc[3:] == np.float64).all()


def check_per_fov_functions():
    """The two per-FOV functions on FOVs of the fixture's cohort, against the statement."""
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    master = load_frame(_g(), "master_")
    for fov, k in (("fovB", 5), ("fovC", 8), ("fovA", 1)):
        rows = master[master["fov"] == fov]
        rows = rows.set_index(np.arange(len(rows))[::-1] + 7)
        xy = rows[["centroid-0", "centroid-1"]].to_numpy()
        names = sorted(set(rows["cell_meta_cluster"]))
        codes = np.array([names.index(v) for v in rows["cell_meta_cluster"]])
        want = cr.nearest_type_means(xy, codes, [0, len(rows)], len(names), k)
        frame = cns.calculate_mean_distance_to_all_cell_types(rows, None, k)
        assert list(frame.columns) == names and frame.index.equals(rows.index)
        assert (frame.dtypes == np.float64).all()
        np.testing.assert_array_equal(frame.to_numpy(), want.astype(np.float64))
        for t, name in enumerate(names):
            one = cns.calculate_mean_distance_to_cell_type(rows, None, name, k)
            if (codes == t).sum() < k:
                assert isinstance(one, list) and len(one) == len(rows) and np.isnan(one).all()
            else:
                assert_same_float32(one, want[:, t], "%s %s" % (fov, name))
    assert len(set(master.loc[master["fov"] == "fovB", "cell_meta_cluster"])) == 4


@pytest.fixture
def host_device(monkeypatch):
    from ark_analysis_amd.analysis import cell_neighborhood_stats
    monkeypatch.setattr(cell_neighborhood_stats, "_nearest_type_means_device", cr.host_stand_in)


# ---- the numpy statement against the reference --------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference is not on this machine")
def test_regenerated_fixture_equals_committed(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_cell_distances.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    a, b = _g(), np.load(os.path.join(str(tmp_path), FIXTURE + ".npz"), allow_pickle=False)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_numpy_statement_equals_fixture():
    """Per FOV, the statement's [n, T] means are the fixture's rows of that FOV: same bits, NaN in the same places."""
    g = _g()
    master = load_frame(g, "master_")
    nan_own_type = 0
    for i in range(int(g["n_cases"])):
        table, kwargs, (want, _) = fixture_case(g, i, master)
        fov_col, type_col = kwargs.get("fov_col", "fov"), kwargs.get("cell_type_col", "cell_meta_cluster")
        label_col = kwargs.get("cell_label_col", "label")
        cen = list(kwargs.get("centroid_cols", ("centroid-0", "centroid-1")))
        assert list(want.columns[:3]) == [fov_col, label_col, type_col]
        assert list(pd.unique(want[fov_col])) == sorted(set(table[fov_col]))          # np.unique order
        for fov in pd.unique(table[fov_col]):
            rows = table[table[fov_col] == fov]
            names = sorted(set(rows[type_col]))
            codes = np.array([names.index(v) for v in rows[type_col]])
            means = cr.nearest_type_means(rows[cen].to_numpy(), codes, [0, len(rows)], len(names), kwargs["k"])
            sel = want[want[fov_col] == fov]
            assert list(sel[label_col]) == list(rows[label_col]) and list(sel.index) == list(rows.index)
            got64 = sel[names].to_numpy()
            assert_same_float32(got64.astype(np.float32), means, "case %d %s" % (i, fov))
            np.testing.assert_array_equal(got64.astype(np.float32).astype(np.float64), got64)
            absent = [c for c in want.columns[3:] if c not in names]
            assert sel[absent].isna().to_numpy().all()
            own = means[np.arange(len(rows)), codes]
            nan_own_type += int(np.isnan(own).sum())
    assert nan_own_type > 0


def test_fixture_holds_the_cases_it_is_meant_to():
    g = _g()
    master = load_frame(g, "master_")
    c = master[master["fov"] == "fovC"]
    assert sorted(c["cell_meta_cluster"].value_counts().tolist()) == sorted(g["c_members"].tolist()) == [4, 5, 8, 13, 34]
    a = master[master["fov"] == "fovA"]
    assert a[["centroid-0", "centroid-1"]].duplicated().sum() == 2 and not a["label"].is_monotonic_increasing
    b = master[master["fov"] == "fovB"][["centroid-0", "centroid-1"]].to_numpy()
    assert (b == np.round(b)).all()
    want = load_frame(g, "c1_dists_")
    grid = want[want["fov"] == "fovB"].iloc[:, 3:].to_numpy()
    assert np.isnan(grid).all(axis=0).sum() == 1                     # the phenotype fovB lacks
    # at k = 5 on the grid every mean is a sum of five float32 square roots of integers: the values repeat
    assert len(np.unique(grid[~np.isnan(grid)])) < 0.5 * (~np.isnan(grid)).sum()


# ---- numpy's float32 row-sum order --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", list(range(1, 41)) + [64, 129, 300])
def test_row_sum_order_is_numpy_s(k):
    rs = np.random.RandomState(k)
    wide = np.sort((rs.uniform(0, 1, (64, k + 7)) * 10.0 ** rs.randint(-3, 4, (64, 1))).astype(np.float32), axis=1)
    want = wide[:, :k].mean(axis=1)
    assert want.dtype == np.float32
    got = np.array([cr.row_sum_order(row[:k]) for row in wide], dtype=np.float32)
    np.testing.assert_array_equal(bits(got), bits(want))
    if k >= 8:      # the order matters: a plain fold differs somewhere
        fold = np.array([np.float32(np.add.accumulate(row[:k], dtype=np.float32)[-1] / np.float32(k)) for row in wide])
        assert (bits(fold) != bits(want)).any()


# ---- host logic through the stand-in ------------------------------------------------------------------------------
def test_generate_cell_distance_analysis_equals_fixture(host_device, tmp_path):
    check_fixture_cases(tmp_path)


def test_per_fov_functions(host_device):
    check_per_fov_functions()


def test_one_device_call_for_the_cohort_and_positional_order(monkeypatch, tmp_path):
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    calls = []

    def counting(xy, types, seg, n_types, k):
        calls.append((len(xy), list(seg), n_types, k))
        return cr.host_stand_in(xy, types, seg, n_types, k)
    monkeypatch.setattr(cns, "_nearest_type_means_device", counting)
    g = _g()
    table, kwargs, (want, _) = fixture_case(g, 1)
    got = cns.generate_cell_distance_analysis(table, None, str(tmp_path / "a.csv"), 5, "cell_meta_cluster", "fov", "label")
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert calls == [(len(table), [0, 60, 285, 349, 399], 5, 5)]


def test_error_paths(host_device, tmp_path):
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    table, _, _ = fixture_case(_g(), 0)
    path = str(tmp_path / "x.csv")
    with pytest.raises(ValueError, match="centroid-1"):
        cns.generate_cell_distance_analysis(table.drop(columns="centroid-1"), None, path, 5)
    with pytest.raises(ValueError, match="cy"):
        cns.generate_cell_distance_analysis(table, None, path, 5, centroid_cols=("cy", "centroid-1"))
    for bad in (0, 33, 100):
        with pytest.raises(ValueError, match="32"):
            cns.generate_cell_distance_analysis(table, None, path, bad)
        with pytest.raises(ValueError, match="32"):
            cns.calculate_mean_distance_to_all_cell_types(table[table["fov"] == "fovA"], None, bad)
    assert not os.path.exists(path)


def test_device_entry_point_is_loud_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    table, _, _ = fixture_case(_g(), 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        cns.generate_cell_distance_analysis(table, None, str(tmp_path / "x.csv"), 5)


def test_som_device_rejects_k_beyond_the_limit_before_touching_a_device():
    import torch
    from ark_analysis_amd import som_device
    assert som_device.NEAREST_MAX_K == 32
    with pytest.raises(ValueError):      # a host tensor: refused like neighbor_counts refuses it
        som_device.nearest_type_means(torch.zeros((4, 2), dtype=torch.float64), torch.zeros(4, dtype=torch.int32),
                                      torch.tensor([0, 4]), 1, 5)


# ---- diversity ----------------------------------------------------------------------------------------------------
def literal_diversity(neighborhood_mat, cell_type_col):
    """The reference's compute_neighborhood_diversity, cell by cell (its expression, restated)."""
    frames = []
    for fov in np.unique(neighborhood_mat["fov"]):
        sub = neighborhood_mat[neighborhood_mat["fov"] == fov]
        scores = []
        for label in sub["label"]:
            p = sub[sub["label"] == label].drop(columns=["fov", "label", cell_type_col]).values[0]
            positive = p > 0
            scores.append(-np.sum(p[positive] * np.log2(p[positive])))
        frames.append(pd.DataFrame({"fov": [fov] * len(sub), "label": sub["label"], cell_type_col: sub[cell_type_col],
                                    "diversity_" + cell_type_col: scores}))
    return pd.concat(frames)


def random_freqs(seed, n=300, m=12):
    rs = np.random.RandomState(seed)
    counts = rs.poisson(rs.choice([0.05, 0.4, 1.5, 6.0], (n, 1)), (n, m)).astype(np.float64)
    counts[rs.choice(n, 20, replace=False)] = 0                       # cells without neighbours
    total = counts.sum(axis=1, keepdims=True)
    freqs = np.divide(counts, total, out=np.zeros_like(counts), where=total > 0)
    frame = pd.DataFrame(freqs, columns=["type%d" % j for j in range(m)])
    frame.insert(0, "fov", rs.choice(["fov2", "fov10", "fov1"], n))
    frame.insert(1, "label", rs.permutation(n) + 1)
    frame.insert(2, "pheno", rs.choice(["a", "b", "c"], n))
    frame.index = rs.permutation(n) + 50
    return frame, freqs


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_diversity_equals_the_literal_loop(seed):
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    frame, freqs = random_freqs(seed)
    n_pos = (freqs > 0).sum(axis=1)
    assert (n_pos == 0).any() and (n_pos >= 8).any() and (n_pos < 8).any()
    want = literal_diversity(frame, "pheno")
    got = cns.compute_neighborhood_diversity(frame, "pheno")
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    np.testing.assert_array_equal(got["diversity_pheno"].to_numpy().view(np.uint64),
                                  want["diversity_pheno"].to_numpy().view(np.uint64))       # -0.0 for an empty row too
    for row in freqs[:40]:
        assert cns.shannon_diversity(row) == -np.sum(row[row > 0] * np.log2(row[row > 0]))


def test_diversity_takes_the_first_row_of_a_repeated_label():
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    frame, _ = random_freqs(5, n=60)
    frame.iloc[10:14, frame.columns.get_loc("label")] = frame["label"].iloc[3]
    frame.iloc[10:14, frame.columns.get_loc("fov")] = [frame["fov"].iloc[3]] * 3 + ["another"]
    pd.testing.assert_frame_equal(cns.compute_neighborhood_diversity(frame, "pheno"), literal_diversity(frame, "pheno"),
                                  check_exact=True)


def test_diversity_error_paths(tmp_path):
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    frame, _ = random_freqs(7, n=30)
    bad = frame.copy()
    bad.iloc[4, 5] = 1.5
    with pytest.raises(ValueError, match="Input must be frequency values."):
        cns.compute_neighborhood_diversity(bad, "pheno")
    with pytest.raises(ValueError, match="cell_type_column"):
        cns.compute_neighborhood_diversity(frame, "not a column")
    with pytest.raises(FileNotFoundError):
        cns.generate_neighborhood_diversity_analysis(str(tmp_path), 50, ["pheno"])


def test_diversity_equals_fixture(tmp_path):
    from ark_analysis_amd.analysis import cell_neighborhood_stats as cns
    g = _g()
    columns, radius = [str(c) for c in g["d_columns"]], int(g["d_radius"])
    assert len(columns) == 2
    for col in columns:
        freqs = load_frame(g, "d_freqs_%s_" % col)
        pd.testing.assert_frame_equal(cns.compute_neighborhood_diversity(freqs, col),
                                      load_frame(g, "d_single_%s_" % col), check_exact=True)
        freqs.to_csv(os.path.join(str(tmp_path), "neighborhood_freqs-%s_radius%d.csv" % (col, radius)), index=False)
    got = cns.generate_neighborhood_diversity_analysis(str(tmp_path), radius, columns)
    pd.testing.assert_frame_equal(got, load_frame(g, "d_merged_"), check_exact=True)
    assert list(got.columns) == ["fov", "label", columns[0], "diversity_" + columns[0], columns[1],
                                 "diversity_" + columns[1]]


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_symbol_exported_and_abi_unchanged():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    assert "pxsom_nearest_type_means" in _capi.SYMBOLS and hasattr(lib, "pxsom_nearest_type_means")
    assert lib.pxsom_abi_version() == _capi.ABI_VERSION == 9
    f = lib.pxsom_nearest_type_means
    # rejected before any HIP call
    assert f(None, None, None, 1, -1, 3, 5, 0.0, None, None) == -1
    assert b"n=-1" in lib.pxsom_last_error()
    assert f(None, None, None, 1, 4, 0, 5, 0.0, None, None) == -1
    assert f(None, None, None, 1, 4, 3, 0, 0.0, None, None) == -1
    assert b"32" in lib.pxsom_last_error()
    assert f(None, None, None, 1, 4, 3, 33, 0.0, None, None) == -1
    assert b"k=33" in lib.pxsom_last_error() and b"32" in lib.pxsom_last_error()
    assert f(None, None, None, 1, 4, 3, 5, float("nan"), None, None) == -1
    assert f(None, None, None, 1, 4, 3, 5, 0.0, None, None) == -1
    assert b"null" in lib.pxsom_last_error()
    import ctypes
    seg = (ctypes.c_int64 * 2)(0, 4)
    assert f(None, None, ctypes.addressof(seg), 1, 4, 3, 5, 0.0, None, None) == -1
    assert b"null array" in lib.pxsom_last_error()


# ---- the fuzz generator of tests/test_gpu_fuzz_cell_distances.py --------------------------------------------------
def test_fuzz_generator_visits_every_class_and_means_something():
    from tests import test_gpu_fuzz_cell_distances as fz
    seen, ks, finite, nans = set(), set(), 0, 0
    for i in range(len(fz.CLASSES)):
        c, again = fz.gen_case(i), fz.gen_case(i)
        assert all(np.array_equal(c[key], again[key]) for key in ("xy", "types", "seg")) and c["k"] == again["k"]
        n = len(c["xy"])
        assert c["xy"].shape == (n, 2) and c["xy"].dtype == np.float64 and c["types"].shape == (n,)
        assert c["seg"][0] == 0 and c["seg"][-1] == n and (np.diff(c["seg"]) >= 0).all()
        assert n == 0 or (0 <= c["types"].min() and c["types"].max() < c["n_types"])
        assert 1 <= c["k"] <= 32
        seen.add(c["cls"])
        ks.add(c["k"])
        if n <= 1500:
            want = cr.nearest_type_means(c["xy"], c["types"], c["seg"], c["n_types"], c["k"])
            finite += int(np.isfinite(want).sum())
            nans += int(np.isnan(want).sum())
    assert seen == set(fz.CLASSES) and len(ks) >= 6 and max(ks) > 16 and min(ks) < 8
    assert finite > 1000 and nans > 100
