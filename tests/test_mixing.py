"""Close-pair counts and mixing scores on CPU: the numpy statement of pxsom_close_pair_counts
(tests/close_pairs_reference.py) against the g23 fixture of the reference (tests/golden/make_golden_mixing.py), the host
functions of ark_analysis_amd.analysis through host stand-ins for the device entry points, the 64 x 64 blocking, the
error paths and the ABI.

The ``check_*`` helpers run unchanged on the GPU box (tests/test_gpu_close_pairs.py) with the real device path."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import close_pairs_reference as cpr
from tests import neighborhood_reference as nr
from tests import test_neighborhood as tn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = "g23_mixing"
CEN = ["centroid-0", "centroid-1"]


def _g():
    return np.load(os.path.join(GOLD, FIXTURE + ".npz"), allow_pickle=False)


def _master(g):
    return tn.load_frame(g, "master_")


def close_case(g, i, master):
    """Fixture close-pair case i: the FOV's rows, the arguments of compute_close_cell_num after the centroids, and the
    boolean membership [n, sets] the case describes."""
    p = "k%d_" % i
    rows = master[master["fov"] == str(g[p + "fov"])]
    analysis, dist_lim = str(g[p + "analysis"]), g[p + "dist_lim"].item()
    channels = [str(c) for c in g["channels"]]
    if analysis == "channel":
        kwargs = dict(current_fov_data=rows, current_fov_channel_data=rows[channels], thresh_vec=g["thresholds"])
        member = np.stack([(rows[c] > t).to_numpy() for c, t in zip(channels, g["thresholds"])], 1)
    else:
        kwargs = dict(current_fov_data=rows, cluster_ids=g["phenotype_ids"])
        member = np.stack([(rows["cell_meta_cluster_id"] == k).to_numpy() for k in g["phenotype_ids"]], 1)
    return rows, (dist_lim, analysis), kwargs, member


def mixing_case(g, i):
    p = "m%d_" % i
    args = ([str(c) for c in g[p + "target"]], [str(c) for c in g[p + "reference"]], str(g[p + "mixing_type"]))
    kwargs = dict(ratio_threshold=g[p + "ratio_threshold"].item(), cell_count_thresh=g[p + "cell_count_thresh"].item())
    return args, kwargs, g[p + "distlim"].item(), bool(g[p + "self_neighbor"])


def check_close_cell_num_cases():
    """compute_close_cell_num against every close-pair case of the fixture: the uint16 table (wrapped where the
    reference wraps), the counts of positive cells, their labels; exact=True gives the same counts unwrapped."""
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    g = _g()
    master = _master(g)
    assert int(g["n_close"]) >= 10
    wrapped = 0
    for i in range(int(g["n_close"])):
        rows, args, kwargs, member = close_case(g, i, master)
        p = "k%d_" % i
        close_num, mark1_num, poslabels = sau.compute_close_cell_num(rows[CEN].to_numpy(), *args, **kwargs)
        assert close_num.dtype == np.uint16
        np.testing.assert_array_equal(close_num, g[p + "close_num"], err_msg=str(i))
        assert [int(v) for v in mark1_num] == g[p + "mark1_num"].tolist()
        np.testing.assert_array_equal(np.concatenate([s.to_numpy() for s in poslabels]), g[p + "poslabels"])
        np.testing.assert_array_equal(np.concatenate([np.asarray(s.index) for s in poslabels]), g[p + "posindex"])
        exact, _, _ = sau.compute_close_cell_num(rows[CEN].to_numpy(), *args, exact=True, **kwargs)
        assert exact.dtype == np.int64
        np.testing.assert_array_equal(exact % 65536, g[p + "close_num"])
        if exact.max() > 65535:
            wrapped += 1
            assert exact[0, 0] == int(g["wrap_true_count"]) == len(rows) * (len(rows) - 1)
            assert int(close_num[0, 0]) == exact[0, 0] - 65536
    assert wrapped >= 2


def check_mixing_cases():
    """compute_mixing_scores over the fixture's cohort equals the reference's per-FOV scores and counts, NaN for NaN;
    compute_mixing_score and compute_cell_ratios over this package's neighbourhood matrix equal them too."""
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    g = _g()
    master = _master(g)
    fovs = [str(f) for f in g["fovs"]]
    seen_scores = 0
    for i in range(int(g["n_mixing"])):
        args, kwargs, distlim, self_neighbor = mixing_case(g, i)
        p = "m%d_" % i
        got = na.compute_mixing_scores(master, *args, distlim=distlim, self_neighbor=self_neighbor, **kwargs)
        assert list(got.columns) == ["fov", "mixing_score", "cell_count"] and list(got["fov"]) == fovs
        np.testing.assert_array_equal(got["mixing_score"].to_numpy(), g[p + "scores"], err_msg=str(i))
        np.testing.assert_array_equal(got["cell_count"].to_numpy(), g[p + "counts"], err_msg=str(i))
        seen_scores += int(np.isfinite(g[p + "scores"]).sum())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            neighbors, _ = na.create_neighborhood_matrix(master, distlim=distlim, self_neighbor=self_neighbor)
            per_fov = [na.compute_mixing_score(neighbors[neighbors["fov"] == fov], *args, **kwargs) for fov in fovs]
        np.testing.assert_array_equal(np.array([s for s, _ in per_fov], dtype=np.float64), g[p + "scores"])
        assert [c for _, c in per_fov] == g[p + "counts"].tolist()
        ratios = na.compute_cell_ratios(neighbors, args[0], args[1], fovs)
        pd.testing.assert_frame_equal(ratios, tn.load_frame(g, p + "ratios_"), check_exact=True)
    assert seen_scores >= 6


def mixing_loop(table, target, reference, mixing_type, distlim, self_neighbor, fovs, label_col="label", **kwargs):
    """The notebook's loop over this package's own functions: the neighbourhood matrix, then one score per FOV."""
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    names = {k: kwargs.pop(k) for k in ("fov_col", "cell_type_col", "centroid_cols") if k in kwargs}
    fov_col, type_col = names.get("fov_col", "fov"), names.get("cell_type_col", "cell_meta_cluster")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        neighbors, _ = na.create_neighborhood_matrix(table, distlim=distlim, self_neighbor=self_neighbor,
                                                     cell_label_col=label_col, **names)
        pairs = [na.compute_mixing_score(neighbors[neighbors[fov_col] == fov], target, reference, mixing_type,
                                         cell_col=type_col, fov_col=fov_col, label_col=label_col, **kwargs)
                 for fov in fovs]
    return pd.DataFrame({"fov": list(fovs), "mixing_score": np.array([s for s, _ in pairs], dtype=np.float64),
                         "cell_count": np.array([c for _, c in pairs], dtype=np.int64)})


@pytest.fixture
def host_device(monkeypatch):
    from ark_analysis_amd.analysis import spatial_analysis_utils
    monkeypatch.setattr(spatial_analysis_utils, "_close_pair_counts_device", cpr.host_stand_in)
    monkeypatch.setattr(spatial_analysis_utils, "_neighbor_counts_device", nr.host_stand_in)


# ---- the numpy statement against the reference --------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference is not on this machine")
def test_regenerated_fixture_equals_committed(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_mixing.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    a, b = _g(), np.load(os.path.join(str(tmp_path), FIXTURE + ".npz"), allow_pickle=False)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_numpy_statement_equals_fixture():
    """The statement's table of every close-pair case, wrapped to uint16, is the reference's; through the packed masks
    and through the boolean memberships alike.  The wrap is pinned: the disc FOV's true count is 72 630."""
    g = _g()
    master = _master(g)
    for i in range(int(g["n_close"])):
        rows, (dist_lim, _), _, member = close_case(g, i, master)
        seg = [0, len(rows)]
        want = g["k%d_close_num" % i]
        direct = cpr.set_pair_counts(rows[CEN].to_numpy(), seg, member, member, dist_lim)[0]
        packed = cpr.pack(member)
        np.testing.assert_array_equal(cpr.close_pair_counts(rows[CEN].to_numpy(), packed, packed, seg, member.shape[1],
                                                            member.shape[1], dist_lim)[0], direct)
        np.testing.assert_array_equal(direct.astype(np.uint16), want, err_msg=str(i))
        np.testing.assert_array_equal(direct, direct.T)
    assert int(g["wrap_true_count"]) == 270 * 269 > 65535


def test_numpy_statement_gives_the_interaction_totals_of_the_fixture():
    """The 2 x 2 table of target / reference close pairs reproduces the reference's scores where it computes one."""
    g = _g()
    master = _master(g)
    fovs = [str(f) for f in g["fovs"]]
    for i in range(int(g["n_mixing"])):
        (target, reference, mixing_type), _, distlim, self_neighbor = mixing_case(g, i)
        for f, fov in enumerate(fovs):
            want = g["m%d_scores" % i][f]
            if np.isnan(want):
                continue
            rows = master[master["fov"] == fov]
            member = np.stack([rows["cell_meta_cluster"].isin(target), rows["cell_meta_cluster"].isin(reference)], 1)
            t = cpr.set_pair_counts(rows[CEN].to_numpy(), [0, len(rows)], member, member, distlim, self_neighbor)[0]
            score = t[0, 1] / (t[0, 1] + t[0, 0]) if mixing_type == "percent" else t[0, 1] / (t[0, 0] + t[1, 1])
            assert score == want, (i, fov)


def test_exact_ties_and_coincident_cells_in_the_statement():
    g = _g()
    master = _master(g)
    xy = master.loc[master["fov"] == "fovB", CEN].to_numpy()
    ones = np.ones((len(xy), 1), dtype=bool)
    at = cpr.set_pair_counts(xy, [0, len(xy)], ones, ones, 50)[0, 0, 0]
    above = cpr.set_pair_counts(xy, [0, len(xy)], ones, ones, float(np.nextafter(np.float32(50), np.float32(60))))[0, 0, 0]
    d32 = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1)).astype(np.float32)
    assert above - at == int((d32 == 50).sum()) > 1000
    xy = np.array([[1 / 3, 2 / 7]] * 3 + [[1 / 3, 2 / 7 + 10]])
    ones = np.ones((4, 1), dtype=bool)
    assert cpr.set_pair_counts(xy, [0, 4], ones, ones, 50)[0, 0, 0] == 6           # the three coincident cells pair only with the fourth
    assert cpr.set_pair_counts(xy, [0, 4], ones, ones, 50, True)[0, 0, 0] == 16


# ---- host logic through the stand-ins -----------------------------------------------------------------------------
def test_compute_close_cell_num_equals_fixture(host_device):
    check_close_cell_num_cases()


def test_mixing_functions_equal_fixture(host_device):
    check_mixing_cases()


def test_get_pos_cell_labels(host_device):
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    g = _g()
    rows = _master(g)
    rows = rows[rows["fov"] == "fovA"]
    got = sau.get_pos_cell_labels_channel(1.0, rows[["chanA", "chanB"]], rows["label"], "chanB")
    pd.testing.assert_series_equal(got, rows["label"][rows["chanB"] > 1.0])
    got = sau.get_pos_cell_labels_cluster(3, rows, "label", "cell_meta_cluster_id")
    pd.testing.assert_series_equal(got, rows["label"][rows["cell_meta_cluster_id"] == 3])
    assert len(got) == int((rows["cell_meta_cluster"] == "CD8T").sum()) > 0


def check_mixing_scores_equal_loop():
    """compute_mixing_scores equals the per-FOV loop over create_neighborhood_matrix, NaN for NaN: every fixture case on
    the whole cohort, on a reordered subset of FOVs, and with renamed columns and a shuffled index."""
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    g = _g()
    master = _master(g)
    fovs = [str(f) for f in g["fovs"]]
    renamed = master.rename(columns=tn.RENAMED)
    renamed.index = np.random.RandomState(2).permutation(len(renamed)) + 1000
    names = dict(fov_col="sample", cell_type_col="pheno", centroid_cols=("cy", "cx"))
    finite = 0
    for i in range(int(g["n_mixing"])):
        args, kwargs, distlim, self_neighbor = mixing_case(g, i)
        for neighbor in (self_neighbor, not self_neighbor):
            got = na.compute_mixing_scores(master, *args, distlim=distlim, self_neighbor=neighbor, **kwargs)
            want = mixing_loop(master, *args, distlim, neighbor, fovs, **kwargs)
            pd.testing.assert_frame_equal(got, want, check_exact=True)
            finite += int(np.isfinite(want["mixing_score"]).sum())
        some = ["fovE", "fovB", "fovD"]
        sub = master[master["fov"].isin(some)]
        got = na.compute_mixing_scores(master, *args, distlim=distlim, self_neighbor=self_neighbor, included_fovs=some,
                                       **kwargs)
        pd.testing.assert_frame_equal(got, mixing_loop(sub, *args, distlim, self_neighbor, some, **kwargs), check_exact=True)
        got = na.compute_mixing_scores(renamed, *args, distlim=distlim, self_neighbor=self_neighbor, **names, **kwargs)
        pd.testing.assert_frame_equal(got, mixing_loop(renamed, *args, distlim, self_neighbor, fovs, "cell_id", **names,
                                                       **kwargs),
                                      check_exact=True)
    assert finite >= 12
    # cells without a neighbour are not counted: in fovD a fifth of the cells leave the neighbourhood matrix
    args, kwargs, distlim, self_neighbor = mixing_case(g, 0)
    got = na.compute_mixing_scores(master, *args, distlim=distlim, **kwargs)
    rows = master[master["fov"] == "fovD"]
    everyone = int(rows["cell_meta_cluster"].isin(args[0] + args[1]).sum())
    assert 0 < int(got.loc[got["fov"] == "fovD", "cell_count"].iloc[0]) < everyone


def test_mixing_scores_equal_the_loop(host_device):
    check_mixing_scores_equal_loop()


@pytest.mark.parametrize("n_sets", [65, 130])
def test_blocks_of_64_sets_equal_the_unblocked_statement(host_device, monkeypatch, n_sets):
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    rs = np.random.RandomState(n_sets)
    sizes = [90, 0, 41]
    seg = np.concatenate([[0], np.cumsum(sizes)])
    xy = rs.uniform(0, 120, (sum(sizes), 2))
    member_q = rs.rand(len(xy), n_sets) < 0.3
    member_c = rs.rand(len(xy), 70) < 0.5
    member_q[:, 64] = True                       # the first set of the second block holds every cell
    calls = []

    def counting(*args):
        calls.append(args[4:6])
        return cpr.host_stand_in(*args)
    monkeypatch.setattr(sau, "_close_pair_counts_device", counting)
    for self_neighbor in (False, True):
        got = sau.set_pair_counts(xy, seg, member_q, member_q, 37.5, self_neighbor)
        np.testing.assert_array_equal(got, cpr.set_pair_counts(xy, seg, member_q, member_q, 37.5, self_neighbor))
        assert got.shape == (3, n_sets, n_sets) and got.dtype == np.int64 and got[1].sum() == 0
    blocks = -(-n_sets // 64)
    assert len(calls) == 2 * blocks * blocks and max(max(c) for c in calls) == 64
    assert sorted(set(calls))[0] == (n_sets - 64 * (blocks - 1),) * 2
    got = sau.set_pair_counts(xy, seg, member_q, member_c, 50)
    np.testing.assert_array_equal(got, cpr.set_pair_counts(xy, seg, member_q, member_c, 50))
    assert got.shape == (3, n_sets, 70)


def test_close_cell_num_with_more_than_64_clusters(host_device):
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    rs = np.random.RandomState(5)
    n, k = 400, 70
    rows = pd.DataFrame({"label": rs.permutation(n) + 1, "cell_meta_cluster_id": rs.randint(1, k + 1, n)})
    xy = rs.uniform(0, 300, (n, 2))
    ids = np.arange(1, k + 1)
    close_num, mark1_num, _ = sau.compute_close_cell_num(xy, 50, "cluster", current_fov_data=rows, cluster_ids=ids)
    member = rows["cell_meta_cluster_id"].to_numpy()[:, None] == ids[None, :]
    np.testing.assert_array_equal(close_num, cpr.set_pair_counts(xy, [0, n], member, member, 50)[0])
    assert close_num.shape == (k, k) and mark1_num == member.sum(axis=0).tolist() and close_num.sum() > 0


def test_compute_mixing_score_leaves_its_argument_unchanged(host_device):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    g = _g()
    master = _master(g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        neighbors, _ = na.create_neighborhood_matrix(master)
    fov = neighbors[neighbors["fov"] == "fovB"]
    before = fov.copy(deep=True)
    score, count = na.compute_mixing_score(fov, ["CD4T"], ["tumor"], "percent", cell_count_thresh=50)
    assert np.isfinite(score) and count > 50
    pd.testing.assert_frame_equal(fov, before, check_exact=True)
    assert list(fov.columns) == list(before.columns) and set(fov["cell_meta_cluster"]) == set(before["cell_meta_cluster"])


def test_error_paths(host_device):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.analysis import spatial_analysis_utils as sau
    g = _g()
    master = _master(g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        neighbors, _ = na.create_neighborhood_matrix(master)
    fov = neighbors[neighbors["fov"] == "fovB"]
    with pytest.raises(ValueError, match="both the target and reference populations: .*tumor"):
        na.compute_mixing_score(fov, ["tumor", "CD4T"], ["tumor"], "percent")
    with pytest.raises(ValueError, match='valid mixing_type: "percent" or "homogeneous"'):
        na.compute_mixing_score(fov, ["CD4T"], ["tumor"], "mixed")
    with pytest.raises(ValueError, match="cell_neighbors_columns"):
        na.compute_mixing_score(fov.drop(columns="label"), ["CD4T"], ["tumor"], "percent")
    with pytest.raises(ValueError, match="both the target and reference populations"):
        na.compute_mixing_scores(master, ["tumor"], ["tumor"], "percent")
    with pytest.raises(ValueError, match="valid mixing_type"):
        na.compute_mixing_scores(master, ["CD4T"], ["tumor"], "neither")
    with pytest.raises(ValueError, match="fovZ"):
        na.compute_mixing_scores(master, ["CD4T"], ["tumor"], "percent", included_fovs=["fovZ"])
    with pytest.raises(ValueError, match="centroid-1"):
        na.compute_mixing_scores(master.drop(columns="centroid-1"), ["CD4T"], ["tumor"], "percent")
    rows = master[master["fov"] == "fovA"]
    with pytest.raises(ValueError, match="good_analyses"):
        sau.compute_close_cell_num(rows[CEN].to_numpy(), 50, "marker", current_fov_data=rows, cluster_ids=[1])
    with pytest.raises(ValueError, match="one .* pair per row"):
        sau.compute_close_cell_num(np.zeros((3, 2)), 50, "cluster", current_fov_data=rows, cluster_ids=[1])
    with pytest.raises(ValueError, match="memberships"):
        sau.set_pair_counts(np.zeros((3, 2)), [0, 3], np.ones((2, 1), bool), np.ones((3, 1), bool), 50)


def test_cell_ratios_accept_and_ignore_bin_number(host_device):
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    table = pd.DataFrame({"fov": ["a"] * 3 + ["b"] * 2, "label": [1, 2, 3, 1, 2],
                          "cell_meta_cluster": ["t", "t", "r", "t", "x"], "t": 0.0, "r": 0.0, "x": 0.0})
    got = na.compute_cell_ratios(table, ["t"], ["r"], ["a", "b"], bin_number=3)
    assert list(got.columns) == ["fov", "cell_ratio"] and list(got["fov"]) == ["a", "b"]
    assert got["cell_ratio"].iloc[0] == 2.0 and np.isnan(got["cell_ratio"].iloc[1])


def test_device_entry_point_is_loud_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    with pytest.raises(RuntimeError, match="no HIP device"):
        na.compute_mixing_scores(_master(_g()), ["CD4T"], ["tumor"], "percent")


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_symbol_exported_and_abi_unchanged():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    assert "pxsom_close_pair_counts" in _capi.SYMBOLS and hasattr(lib, "pxsom_close_pair_counts")
    assert lib.pxsom_abi_version() == _capi.ABI_VERSION == 9
    call = lib.pxsom_close_pair_counts
    # rejected before any HIP call
    assert call(None, None, None, None, 1, -1, 2, 2, 1.0, 0.0, 0, None, None) == -1
    assert b"pxsom_close_pair_counts: n=-1" in lib.pxsom_last_error()
    for nq, nc in ((0, 2), (2, 0), (65, 2), (2, 65)):
        assert call(None, None, None, None, 1, 4, nq, nc, 1.0, 0.0, 0, None, None) == -1
        assert b"outside 1 .. 64" in lib.pxsom_last_error()
    assert call(None, None, None, None, 1, 4, 2, 2, 1.0, 0.0, 2, None, None) == -1
    assert b"self_neighbor=2" in lib.pxsom_last_error()
    assert call(None, None, None, None, 1, 4, 2, 2, float("nan"), 0.0, 0, None, None) == -1
    assert call(None, None, None, None, 1, 4, 2, 2, 1.0, float("nan"), 0, None, None) == -1
    assert b"NaN" in lib.pxsom_last_error()
    assert call(None, None, None, None, 1, 2 ** 31, 2, 2, 1.0, 0.0, 0, None, None) == -1
    assert call(None, None, None, None, 1, 4, 2, 2, 1.0, 0.0, 0, None, None) == -1
    assert b"null seg" in lib.pxsom_last_error()
    seg = np.array([0, 4], dtype=np.int64)
    assert call(None, None, None, seg.ctypes.data, 1, 4, 2, 2, 1.0, 0.0, 0, None, None) == -1
    assert b"null array" in lib.pxsom_last_error()
    assert call(None, None, None, seg.ctypes.data, 0, 0, 2, 2, 1.0, 0.0, 0, None, None) == 0      # no FOV: nothing to write


# ---- the fuzz generator of tests/test_gpu_fuzz_close_pairs.py -----------------------------------------------------
def test_fuzz_generator_is_seeded_and_means_something():
    from tests import test_gpu_fuzz_close_pairs as fz
    ties = coincident = bit63 = shared = 0
    for i in range(0, fz.CASES, 5):
        c, again = fz.gen_case(i), fz.gen_case(i)
        assert all(np.array_equal(c[k], again[k]) for k in ("xy", "member_q", "member_c", "seg"))
        n = len(c["xy"])
        assert c["xy"].shape == (n, 2) and c["member_q"].dtype == np.uint64 and c["member_c"].shape == (n,)
        assert c["seg"][0] == 0 and c["seg"][-1] == n and (np.diff(c["seg"]) >= 0).all() and np.diff(c["seg"]).max() <= 2000
        assert 1 <= c["n_sets_q"] <= 64 and 1 <= c["n_sets_c"] <= 64
        ones = np.ones((n, 1), dtype=bool)
        at = cpr.set_pair_counts(c["xy"], c["seg"], ones, ones, c["distlim"]).sum()
        wider = cpr.set_pair_counts(c["xy"], c["seg"], ones, ones,
                                    np.nextafter(np.float32(c["distlim"]), np.float32(np.inf))).sum()
        with_self = cpr.set_pair_counts(c["xy"], c["seg"], ones, ones, c["distlim"], True).sum()
        ties += int(wider - at)
        coincident += int(with_self - at) - n
        bit63 += int((c["member_q"] >> np.uint64(63)).any())
        shared += int(c["member_c"] is c["member_q"])
    assert ties > 100 and coincident > 10 and bit63 > 0 and 0 < shared < fz.CASES
