"""The spatial-LDA preprocessing on CPU: radius_threshold against np.sqrt, the argument checks of
pxsom_neighborhood_sums through the ABI, ark_analysis_amd.spLDA.processing through host stand-ins for its device entry
points against the per-anchor pandas loop of tests/splda_reference.py, the g27 fixture of the reference
(tests/golden/make_golden_splda.py), and the topic EDA.

The ``check_*`` helpers run unchanged on the GPU box (tests/test_gpu_splda.py) with the real device path."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from tests import kmeans_reference as kr
from tests import silhouette_reference as silr
from tests import splda_reference as sr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = "g27_splda"
U = 2.0 ** -53
MARKERS = ["m0", "m1", "m2", "m3", "m4", "m5"]
FEATURIZATIONS = ["cluster", "marker", "avg_marker", "count"]


def fixture():
    return np.load(os.path.join(GOLD, FIXTURE + ".npz"), allow_pickle=False)


def load_frame(g, prefix):
    cols = [str(c) for c in g[prefix + "columns"]]
    dtypes = [str(t) for t in g[prefix + "dtypes"]]
    data = {}
    for i, (col, dt) in enumerate(zip(cols, dtypes)):
        v = g[prefix + "col%d" % i]
        data[col] = v.astype(object) if dt == "object" else v
    df = pd.DataFrame(data, columns=cols)
    assert [str(t) for t in df.dtypes] == dtypes
    return df


@pytest.fixture
def host_entries(monkeypatch):
    """The device entry points of the spatial-LDA modules swapped for the numpy statements of the same contracts."""
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    from ark_analysis_amd.spLDA import processing as pros
    from ark_analysis_amd.utils import spatial_lda_utils as spu
    monkeypatch.setattr(pros, "_neighborhood_sums_device",
                        lambda xy, feats, seg, radius: sr.host_stand_in(pros.RADIUS_TEST)(xy, feats, seg, radius))
    monkeypatch.setattr(spu, "_silhouette_sums_device", sr.silhouette_sums_stand_in)
    monkeypatch.setattr(sau, "_kmeans_lloyd_device", kr.host_stand_in)
    monkeypatch.setattr(sau, "_silhouette_device", silr.host_stand_in)
    return pros


# ---- radius_threshold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("radius", [25, 32, 50, 64, 100, 2.5, float(np.nextafter(32.0, 0.0))])
def test_radius_threshold_is_where_sqrt_flips(radius, closed):
    """s < s_lim exactly when sqrt(s) < radius (closed: <=), on the 8 doubles either side of s_lim.  32 and 64 are the
    cases ``radius ** 2`` gets wrong, in the closed test: the root of the double above 1024 (4096) lies just below the
    midpoint of 32 (64) and the double above it and rounds down to the radius, so ``sqrt(s) <= radius`` holds for an s
    that ``s <= radius ** 2`` leaves out.  (The open test ``s < radius ** 2`` is right for all seven radii: the root of
    the double below 1024 lies just below the midpoint under 32 and rounds down, away from the radius.)"""
    from ark_analysis_amd.som_device import radius_threshold
    s_lim = radius_threshold(radius, closed)
    assert isinstance(s_lim, float)
    s = np.float64(s_lim)
    around = [s]
    lo = hi = s
    for _ in range(8):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        around += [lo, hi]
    for v in around:
        inside = np.sqrt(v) <= np.float64(radius) if closed else np.sqrt(v) < np.float64(radius)
        assert bool(v < s) == bool(inside), (radius, closed, float(v))
    if radius in (32, 64):
        above = np.nextafter(np.float64(radius) ** 2, np.inf)
        assert np.sqrt(above) == radius
        assert s_lim == (np.nextafter(above, np.inf) if closed else float(radius) ** 2)


def test_radius_threshold_edge_values():
    from ark_analysis_amd.som_device import radius_threshold
    assert radius_threshold(float("nan")) == 0.0 and radius_threshold(float("nan"), True) == 0.0
    assert radius_threshold(-1.0) == 0.0 and radius_threshold(0.0) == 0.0
    assert radius_threshold(0.0, True) == 5e-324            # only s == 0 is inside
    assert radius_threshold(float("inf"), True) == float("inf")


def test_facade_exports_the_new_names():
    from ark_analysis_amd import som_device
    from ark_analysis_amd.som_device import clustering, spatial
    assert som_device.neighborhood_sums is spatial.neighborhood_sums
    assert som_device.radius_threshold is spatial.radius_threshold
    assert som_device.silhouette_sums is clustering.silhouette_sums


# ---- the entry's argument checks (no GPU: they come before any HIP call) ---------------------------------------------------
def test_entry_argument_checks():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fn = lib.pxsom_neighborhood_sums
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    seg = (ctypes.c_int64 * 2)(0, 4)
    ok_args = dict(xy=base, feat=base, seg=ctypes.addressof(seg), n_fovs=1, n=4, n_feat=2, s_lim=1.0, sums=base,
                   counts=base)

    def call(**kw):
        a = dict(ok_args, **kw)
        return fn(a["xy"], a["feat"], a["seg"], a["n_fovs"], a["n"], a["n_feat"], a["s_lim"], a["sums"], a["counts"],
                  None)
    assert call(n=-1) == -1 and b"n=-1" in lib.pxsom_last_error()
    assert call(n_fovs=-1) == -1
    assert call(n_feat=-1) == -1 and b"n_feat=-1" in lib.pxsom_last_error()
    assert call(seg=None) == -1 and b"null seg" in lib.pxsom_last_error()
    assert call(xy=base + 8) == -1 and b"16-byte" in lib.pxsom_last_error()
    assert call(s_lim=float("nan")) == -1 and b"NaN" in lib.pxsom_last_error()
    assert call(xy=None) == -1 and b"null array" in lib.pxsom_last_error()
    assert call(feat=None) == -1 and call(sums=None) == -1 and call(counts=None) == -1
    assert call(n=0) == 0                                    # nothing to launch
    assert call(n=0, xy=None, feat=None, sums=None, counts=None) == 0
    assert call(n=0, seg=None) == -1


# ---- featurisation end to end -----------------------------------------------------------------------------------------------
def synthetic_formatted_table():
    """Three FOVs of 300, 40 and 1 cells on square fields sized for about 10 neighbours at radius 50; five clusters, one
    of them absent from the second FOV; six markers in [0, 1] with some values exactly 0.5; a few non-anchor cells."""
    rs = np.random.RandomState(24)
    table = {}
    for fov, m in (("fovB", 300), ("fovA", 40), ("fovC", 1)):
        side = max(np.sqrt(m * np.pi * 50.0 ** 2 / 10.0), 1.0)
        df = pd.DataFrame({"cell_size": rs.randint(20, 300, m), "x": rs.uniform(0, side, m), "y": rs.uniform(0, side, m)})
        for name in MARKERS:
            v = rs.uniform(0, 1, m)
            v[rs.uniform(size=m) < 0.1] = 0.5
            df[name] = v
        df["cluster"] = rs.choice(["c0", "c1", "c2", "c3"] if fov == "fovA" else ["c0", "c1", "c2", "c3", "c4"], m)
        df["is_index"] = rs.uniform(size=m) > 0.05 if m > 1 else True
        df["isimmune"] = True
        table[fov] = df
    assert set(table["fovB"]["cluster"]) == {"c0", "c1", "c2", "c3", "c4"} and not table["fovB"]["is_index"].all()
    table["fovs"] = np.array(["fovB", "fovA", "fovC"])        # the order the result follows
    table["markers"] = list(MARKERS)
    table["clusters"] = ["c0", "c1", "c2", "c3", "c4"]
    return table


_STATEMENT = {}


def statement(featurization, fold=False):
    """The per-anchor pandas loop on the synthetic table at radius 50, computed once per process."""
    key = (featurization, fold)
    if key not in _STATEMENT:
        _STATEMENT[key] = sr.featurize(synthetic_formatted_table(), featurization, 50, fold=fold)
    return _STATEMENT[key]


def check_featurization(pros, featurization):
    """neighborhood_features of the synthetic table against the per-anchor pandas loop: index tuples, column order,
    integers equal; avg_marker bit-for-bit equal to the statement's fold and, with m neighbours, within
    2 (m + 1) 2^-53 sum|x| / m of pandas' mean -- both are sums of the same m doubles in some order, each within
    (m - 1) 2^-53 sum|x| of the exact sum to first order, and one division each follows."""
    table = synthetic_formatted_table()
    got = pros.neighborhood_features(table, featurization, 50, "is_index")
    want, sizes, abs_sums = statement(featurization)
    anchors = [(f, p) for f in table["fovs"] for p in np.flatnonzero(table[f]["is_index"].to_numpy())]
    assert list(got.index) == anchors == list(want.index)
    assert [f for f, _ in anchors][0] == "fovB" and 0 < len(anchors) < 341
    assert list(got.columns) == list(want.columns)
    if featurization == "avg_marker":
        assert list(got.columns) == MARKERS and all(str(t) == "float64" for t in got.dtypes)
        folded, _, _ = statement(featurization, fold=True)
        np.testing.assert_array_equal(got.to_numpy(), folded.to_numpy())
        bound = 2 * (sizes[:, None] + 1) * U * abs_sums / sizes[:, None]
        assert (np.abs(got.to_numpy() - want.to_numpy()) <= bound).all()
        assert sizes.min() >= 1 and sizes.max() > 10
    else:
        assert all(str(t) == "int64" for t in got.dtypes)
        np.testing.assert_array_equal(got.to_numpy(), want.to_numpy().astype(np.int64))
        if featurization == "cluster":
            assert list(got.columns) == ["c0", "c1", "c2", "c3", "c4"]
            assert got.loc["fovA", "c4"].sum() == 0 and got["c4"].sum() > 0
            np.testing.assert_array_equal(got.sum(axis=1).to_numpy(), sizes)
        elif featurization == "marker":
            assert list(got.columns) == MARKERS
        else:
            assert list(got.columns) == ["count"] and got.loc[("fovC", 0), "count"] == 1


def check_featurize_cell_table(pros):
    """featurize_cell_table on the two larger FOVs: the three-key dict, the frame of neighborhood_features, the training
    rows a stratified subset that the seed reproduces; and scikit-learn's error for a FOV with one reference cell."""
    table = synthetic_formatted_table()
    with pytest.raises(ValueError, match="least populated class"):
        pros.featurize_cell_table(table, "count", radius=50)
    table["fovs"] = table["fovs"][:2]
    del table["fovC"]
    out = pros.featurize_cell_table(table, "marker", radius=50, n_processes=3, seed=7)
    assert list(out) == ["featurized_fovs", "train_features", "featurization"] and out["featurization"] == "marker"
    pd.testing.assert_frame_equal(out["featurized_fovs"], pros.neighborhood_features(table, "marker", 50, "is_index"))
    train = out["train_features"]
    assert abs(len(train) - 0.75 * len(out["featurized_fovs"])) < 1
    pd.testing.assert_frame_equal(train, out["featurized_fovs"].loc[train.index])
    again = pros.featurize_cell_table(table, "marker", radius=50, seed=7)
    assert list(again["train_features"].index) == list(train.index)
    other = pros.featurize_cell_table(table, "marker", radius=50, seed=8)
    assert list(other["train_features"].index) != list(train.index)


@pytest.mark.parametrize("featurization", FEATURIZATIONS)
def test_featurization_equals_the_pandas_loop(host_entries, featurization):
    check_featurization(host_entries, featurization)


def test_featurize_cell_table_dict_and_split(host_entries):
    check_featurize_cell_table(host_entries)


def test_radius_test_le_takes_the_cells_at_the_radius(host_entries, monkeypatch):
    """Cells at (0, 0), (30, 40), (50, 0), (0, 50): at radius 50 the first has 1 neighbour under "lt" and 4 under "le"."""
    df = pd.DataFrame({"x": [0.0, 30.0, 50.0, 0.0], "y": [0.0, 40.0, 0.0, 50.0], "cluster": ["a"] * 4,
                       "is_index": [True] * 4})
    table = {"f": df, "fovs": np.array(["f"]), "markers": None, "clusters": ["a"]}
    assert host_entries.RADIUS_TEST == "lt" and host_entries.RECALLED["radius_test"] == "lt"
    assert host_entries.neighborhood_features(table, "count", 50)["count"].tolist()[0] == 1
    monkeypatch.setattr(host_entries, "RADIUS_TEST", "le")
    assert host_entries.neighborhood_features(table, "count", 50)["count"].tolist()[0] == 4


def test_train_fraction_of_1000_rows(host_entries):
    """As the reference's test: 1000 cells in two FOVs, 0.75 and 0.5 of them drawn for training."""
    rs = np.random.RandomState(5)
    table = {}
    for fov in ("a", "b"):
        table[fov] = pd.DataFrame({"x": rs.uniform(0, 1024, 500), "y": rs.uniform(0, 1024, 500),
                                   "cluster": rs.choice(["x", "y", "z"], 500), "is_index": True})
    table.update({"fovs": np.array(["a", "b"]), "markers": None, "clusters": ["x", "y", "z"]})
    for frac in (0.75, 0.5):
        out = host_entries.featurize_cell_table(table, "cluster", train_frac=frac)
        assert out["featurized_fovs"].shape == (1000, 3) and out["train_features"].shape[0] == frac * 1000
        per_fov = out["train_features"].index.map(lambda x: x[0]).value_counts()
        assert per_fov["a"] == per_fov["b"] == frac * 500


def test_argument_errors_of_featurize_and_difference_matrices(host_entries):
    table = synthetic_formatted_table()
    with pytest.raises(TypeError, match="radius should be of type 'int'"):
        host_entries.featurize_cell_table(table, radius=50.0)
    with pytest.raises(ValueError, match="radius must not be less than 25"):
        host_entries.featurize_cell_table(table, radius=24)
    with pytest.raises(ValueError, match="One or both of 'training' or 'inference' must be True"):
        host_entries.create_difference_matrices(table, {}, training=False, inference=False)
    with pytest.raises(NotImplementedError, match="spatial_lda.featurization.make_merged_difference_matrices"):
        host_entries.create_difference_matrices(table, {})
    for doc in (host_entries.__doc__, open(os.path.join(os.path.dirname(GOLD), "..", "README.md")).read(),
                open(os.path.join(os.path.dirname(GOLD), "..", "DESIGN.md")).read()):
        assert "parity with spatial_lda itself unpinned" in " ".join(doc.split())


# ---- the g27 fixture of the reference -----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference is not on this machine")
def test_regenerated_fixture_equals_committed(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_splda.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    a, b = fixture(), np.load(os.path.join(str(tmp_path), FIXTURE + ".npz"), allow_pickle=False)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_fixture_is_small_and_holds_the_generators_inputs():
    assert os.path.getsize(os.path.join(GOLD, FIXTURE + ".npz")) < 256 * 1024
    g = fixture()
    pd.testing.assert_frame_equal(load_frame(g, "master_"), sr.golden_cell_table())
    data, labels = sr.golden_within_case()
    np.testing.assert_array_equal(g["w_data"], data)
    np.testing.assert_array_equal(g["w_labels"], labels)


@pytest.mark.parametrize("case", list(sr.FORMAT_CASES))
def test_format_cell_table_and_fov_density_equal_the_reference(case):
    from ark_analysis_amd.spLDA import processing as pros
    g = fixture()
    table = load_frame(g, "master_")
    before = table.copy()
    formatted = pros.format_cell_table(table, **sr.FORMAT_CASES[case])
    pd.testing.assert_frame_equal(table, before)
    got = {}
    sr.record_formatted(got, "f_%s_" % case, formatted)
    want_keys = [k for k in g.files if k.startswith("f_%s_" % case)]
    assert sorted(got) == sorted(want_keys)
    for k in want_keys:
        np.testing.assert_array_equal(got[k], g[k], err_msg=k)
    dens = pros.fov_density(formatted, total_pix=512 ** 2)
    assert list(dens) == ["average_area", "cellular_density", "total_cells"]
    for key in dens:
        assert list(dens[key]) == list(formatted["fovs"])
        np.testing.assert_array_equal([dens[key][f] for f in formatted["fovs"]], g["d_%s_%s" % (case, key)])


def test_checker_errors_have_the_references_texts():
    from ark_analysis_amd.spLDA import processing as pros
    from ark_analysis_amd.utils import spatial_lda_utils as spu
    g = fixture()
    table = load_frame(g, "master_")
    formatted = pros.format_cell_table(table, **sr.FORMAT_CASES["both"])
    got = sr.golden_errors(spu, table, formatted)
    assert list(got) == [str(n) for n in g["e_names"]] and len(got) == 13
    for name, text in zip(g["e_names"], g["e_texts"]):
        assert got[str(name)] == str(text), name


def test_within_cluster_sums_host_equals_the_reference():
    from ark_analysis_amd.utils import spatial_lda_utils as spu
    g = fixture()
    assert spu.within_cluster_sums(g["w_data"], g["w_labels"]) == g["w_sum"]
    assert spu.within_cluster_sums(pd.DataFrame(g["w_data"]), g["w_labels"]) == g["w_sum"]
    with pytest.raises(ValueError, match="pairs must be"):
        spu.within_cluster_sums(g["w_data"], g["w_labels"], pairs="gpu")


# ---- the pooled within-cluster sum through the device route ------------------------------------------------------------------
def check_within_cluster_sums_device(spu):
    """pairs="device" against the host pdist form on 300 x 7 with 4 labels, one of them a singleton.

    Bound.  Every term is non-negative, so relative errors do not grow through the sums.  A distance carries at most
    d + 2 roundings on either side (d differences, whose errors double in the squares; d additions of squares; the root
    halves the total and adds one).  Device side: S[i, c] is at most n additions, the fold of a cluster's rows at most n
    more, one division (4 n_c is exact), at most k additions over the clusters: m = d + 2 + 2 n + 1 + k roundings.  Host
    side: pdist's sum is numpy's pairwise sum, whose chain of additions is shorter than n here (blocks of 128 in 8
    lanes, then a tree), one division, k additions: fewer than m.  Each side is within gamma_m = m u / (1 - m u) of the
    exact value relatively, u = 2^-53, so they differ by at most 2 gamma_m relative (1.4e-13 here)."""
    rs = np.random.RandomState(15)
    n, d, k = 300, 7, 4
    data = rs.normal(size=(n, d))
    labels = rs.randint(0, 3, n) * 5 + 2            # values 2, 7, 12: not 0 .. k - 1
    labels[17] = 40                                 # a singleton: pdist of one row is empty, its sum 0
    assert sorted(np.unique(labels)) == [2, 7, 12, 40]
    host = spu.within_cluster_sums(data, labels)
    dev = spu.within_cluster_sums(data, labels, pairs="device")
    m = d + 2 + 2 * n + 1 + k
    gamma = m * U / (1 - m * U)
    print("within_cluster_sums host %.17g device %.17g relative %.3g bound %.3g"
          % (host, dev, abs(dev - host) / host, 2 * gamma))
    assert host > 0 and abs(dev - host) <= 2 * gamma * host
    assert spu.within_cluster_sums(pd.DataFrame(data), labels, pairs="device") == dev


def test_within_cluster_sums_device_route(host_entries):
    from ark_analysis_amd.utils import spatial_lda_utils as spu
    check_within_cluster_sums_device(spu)


# ---- topic EDA -----------------------------------------------------------------------------------------------------------------
def blobs(n=400, d=5, seed=3):
    """Four well-separated Gaussian blobs (unit spread, centres 40 apart along different axes) as a frame, and the blob
    of every row."""
    rs = np.random.RandomState(seed)
    centres = np.zeros((4, d))
    centres[1, 0], centres[2, 1], centres[3, 2] = 40.0, 40.0, 40.0
    which = np.arange(n) % 4
    rs.shuffle(which)
    x = centres[which] + rs.normal(size=(n, d))
    return pd.DataFrame(x, columns=["f%d" % i for i in range(d)]), which


def test_topic_eda_host():
    from sklearn.cluster import KMeans
    from ark_analysis_amd.spLDA import processing as pros
    from ark_analysis_amd.utils import spatial_lda_utils as spu
    rs = np.random.RandomState(2)
    features = pd.DataFrame(rs.randint(0, 12, (200, 6)), columns=list("abcdef"))
    topics = [3, 5]
    # scikit-learn adds the inertia up in an order that depends on its thread pool: one thread, the same bits
    from threadpoolctl import threadpool_limits
    with threadpool_limits(limits=1):
        stats = pros.compute_topic_eda(features, "cluster", topics, silhouette=True, num_boots=25, seed=11)
        want_inertia = {k: KMeans(n_clusters=k, n_init="auto", random_state=11).fit(features).inertia_ for k in topics}
        bare = pros.compute_topic_eda(features, "cluster", topics, seed=11)
    assert list(stats) == spu.EDA_KEYS == ['inertia', 'silhouette', 'gap_stat', 'gap_sds', 'cell_counts', "featurization"]
    assert stats["featurization"] == "cluster"
    for k in topics:
        assert stats["inertia"][k] == want_inertia[k]
        counts = stats["cell_counts"][k]
        assert counts.shape == (6, k) and list(counts.index) == list("abcdef")
        np.testing.assert_array_equal(counts.sum(axis=1).to_numpy(), features.sum(axis=0).to_numpy())
        assert -1 <= stats["silhouette"][k] <= 1
        assert np.isfinite(stats["gap_stat"][k]) and stats["gap_sds"][k] >= 0
    assert bare["silhouette"] == {} and bare["gap_stat"] == {} and bare["gap_sds"] == {}
    assert bare["inertia"] == stats["inertia"]


def test_topic_eda_errors():
    from ark_analysis_amd.spLDA import processing as pros
    features = pd.DataFrame(np.arange(60.0).reshape(20, 3))
    with pytest.raises(ValueError, match="Number of bootstrap samples must be at least 25"):
        pros.compute_topic_eda(features, "cluster", [3, 4], num_boots=24)
    with pytest.raises(ValueError, match=r"Number of topics must be in \[2, 19\]"):
        pros.compute_topic_eda(features, "cluster", [2, 4])
    with pytest.raises(ValueError, match=r"Number of topics must be in \[2, 19\]"):
        pros.compute_topic_eda(features, "cluster", [3, 19])
    with pytest.raises(ValueError, match="kmeans must be 'host' or 'device'"):
        pros.compute_topic_eda(features, "cluster", [3, 4], kmeans="gpu")
    with pytest.raises(ValueError, match="kmeans must be 'host' or 'device'"):
        pros.gap_stat(features, 3, 1.0, kmeans="gpu")


def test_gap_stat_host_is_finite_and_seeded():
    from ark_analysis_amd.spLDA import processing as pros
    from threadpoolctl import threadpool_limits
    features, _ = blobs(120, 3)
    with threadpool_limits(limits=1):        # scikit-learn's sums in one order
        gap, s = pros.gap_stat(features, 4, 50.0, num_boots=25, seed=9)
        again = pros.gap_stat(features, 4, 50.0, num_boots=25, seed=9)
    assert np.isfinite(gap) and np.isfinite(s) and s >= 0
    assert again == (gap, s)


def check_topic_eda_device(pros, sau):
    """compute_topic_eda(kmeans="device") on four well-separated blobs, n = 400, d = 5, topics 3, 4, 5: at k = 4 the
    labels are the blobs; inertia[4] equals sum((x - centre[label])^2) recomputed on the host from the same fit within
    (n d + 2) 2^-53 relative (that many non-negative terms added in another order); the silhouette entries are
    _silhouette_device called directly; the same seed gives the same gap statistics."""
    features, which = blobs()
    n, d = features.shape
    topics = [3, 4, 5]
    stats = pros.compute_topic_eda(features, "avg_marker", topics, silhouette=True, num_boots=25, kmeans="device", seed=4)
    assert list(stats) == ['inertia', 'silhouette', 'gap_stat', 'gap_sds', 'cell_counts', "featurization"]
    fits = sau.kmeans_fits_device(features, topics, 4, "auto")
    fit = fits[1]
    pairs = set(zip(which.tolist(), fit.labels_.tolist()))
    assert len(pairs) == 4 and len({a for a, _ in pairs}) == 4 and len({b for _, b in pairs}) == 4
    x = features.to_numpy()
    recomputed = ((x - fit.cluster_centers_[fit.labels_]) ** 2).sum()
    print("inertia[4] %.17g recomputed %.17g relative %.3g bound %.3g"
          % (stats["inertia"][4], recomputed, abs(stats["inertia"][4] - recomputed) / recomputed, (n * d + 2) * U))
    assert abs(stats["inertia"][4] - recomputed) <= (n * d + 2) * U * recomputed
    encoded = [sau._encode_labels(f.labels_, n) for f in fits]
    direct = sau._silhouette_device(x, np.stack([c for c, _ in encoded]), [k for _, k in encoded])
    assert [stats["silhouette"][k] for k in topics] == [float(v) for v in direct]
    assert stats["silhouette"][4] > 0.9 and stats["silhouette"][4] == max(stats["silhouette"].values())
    for k in topics:
        counts = stats["cell_counts"][k]
        assert counts.shape == (d, k)
        np.testing.assert_allclose(counts.sum(axis=1).to_numpy(), features.sum(axis=0).to_numpy(), rtol=1e-12)
        assert np.isfinite(stats["gap_stat"][k]) and stats["gap_sds"][k] >= 0
    again = pros.compute_topic_eda(features, "avg_marker", topics, num_boots=25, kmeans="device", seed=4)
    assert again["gap_stat"] == stats["gap_stat"] and again["gap_sds"] == stats["gap_sds"] and again["silhouette"] == {}
    one = pros.gap_stat(features, 4, 100.0, num_boots=25, kmeans="device", seed=4)
    assert one == pros.gap_stat(features, 4, 100.0, num_boots=25, kmeans="device", seed=4) and one[1] >= 0


def test_topic_eda_device_route_through_host_stand_ins(host_entries):
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    check_topic_eda_device(host_entries, sau)
