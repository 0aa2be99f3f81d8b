"""The fibre object table on CPU: the numpy statements of tests/fiber_reference.py against the g26
fixture of the reference (tests/golden/make_golden_fibers.py), ark_analysis_amd.segmentation.fiber_segmentation through
host stand-ins for its device entry points, Euler numbers and orientations counted by hand, the entries that are not
built, the error paths and the ABI.

The ``check_*`` helpers run unchanged on the GPU box (tests/test_gpu_fibers.py) with the real device path."""
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

from ark_analysis_amd import image_io
from ark_analysis_amd.segmentation import regionprops_extraction as rpe
from tests import fiber_reference as fr

GOLD = fr.GOLD
PROPERTIES = ["major_axis_length", "minor_axis_length", "orientation", "area", "eccentricity", "euler_number"]
TABLE_COLUMNS = ["fov", "label", "centroid-0", "centroid-1", "major_axis_length", "minor_axis_length", "orientation",
                 "area", "eccentricity", "euler_number"]


@pytest.fixture
def fs(monkeypatch):
    fr.install_stand_ins(monkeypatch.setattr)
    from ark_analysis_amd.segmentation import fiber_segmentation
    return fiber_segmentation


def _quiet(f, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*args, **kwargs)


# ---- helpers shared with the GPU tests --------------------------------------------------------------------------------
def check_alignment_cases(fs):
    """calculate_fiber_alignment against every alignment case of the fixture, exactly."""
    g = fr.fixture()
    for prefix in ("a_", "t_"):
        table = fr.load_frame(g, prefix)
        for k in g["k_values"].tolist():
            got = fs.calculate_fiber_alignment(table, k=k)
            assert list(got.columns) == list(table.columns) + ["alignment_score"] and len(got) == len(table)
            np.testing.assert_array_equal(got["label"].to_numpy(), table["label"].to_numpy())
            np.testing.assert_array_equal(got["alignment_score"].to_numpy(dtype=np.float64),
                                          g[prefix + "scores_k%d" % k], err_msg="%s k=%d" % (prefix, k))


def _mean_bound(values):
    """n 2^-52 mean|x|: the summation order inside pandas is not part of the contract."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    return 0.0 if v.size == 0 else v.size * 2.0 ** -52 * float(np.mean(np.abs(v)))


def _compare_stats(got, want, groups, mean_columns):
    """Frames ``got`` and ``want`` (one row per entry of ``groups``, the rows of the object table behind it): every
    column outside ``mean_columns`` equal, those within n 2^-52 mean|x| of the group's values, NaN in the same places."""
    assert list(got.columns) == list(want.columns) and len(got) == len(want) == len(groups)
    for col in want.columns:
        a, b = got[col].to_numpy(), want[col].to_numpy()
        if col not in mean_columns:
            if b.dtype.kind == "f":
                np.testing.assert_array_equal(a.astype(np.float64), b, err_msg=col)
            else:
                assert [str(v) for v in a] == [str(v) for v in b], col
            continue
        a = a.astype(np.float64)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=col)
        for i, rows in enumerate(groups):
            if not np.isnan(b[i]):
                assert abs(a[i] - b[i]) <= _mean_bound(rows[col[len("avg_"):]]), (col, i, a[i], b[i])


def check_summary_cases(fs, tmp_dir):
    """generate_summary_stats (and through it generate_tile_stats and calculate_density) against every summary case."""
    g = fr.fixture()
    for i in range(int(g["n_summary"])):
        p = "s%d_" % i
        name, tile_length, min_fiber_num = str(g[p + "cohort"]), int(g[p + "tile_length"]), int(g[p + "min_fiber_num"])
        table = fr.load_frame(g, "c_%s_" % name)
        fovs = [str(f) for f in g["c_%s_fovs" % name]]
        case_dir = os.path.join(str(tmp_dir), "case%d" % i)
        os.makedirs(case_dir)
        sides = {}
        for fov in fovs:
            plane = g["c_%s_plane_%s" % (name, fov)]
            sides[fov] = plane.shape[0]
            image_io.write_image(os.path.join(case_dir, fov + "_fiber_labels.tiff"), plane)
        fov_stats, tile_stats = fs.generate_summary_stats(table, case_dir, tile_length=tile_length,
                                                          min_fiber_num=min_fiber_num)
        written = sorted(os.path.relpath(os.path.join(d, f), case_dir) for d, _, files in os.walk(case_dir)
                         for f in files if f.endswith(".csv"))
        assert written == [str(w) for w in g[p + "written"]]
        by_fov = [table[table.fov == fov] for fov in np.unique(table.fov)]
        means = ["avg_" + m for m in PROPERTIES + ["alignment_score"]]
        _compare_stats(fov_stats, fr.load_frame(g, p + "fov_"), by_fov, means)
        tiles = []
        for rows in by_fov:
            per_side = sides[rows.fov.iloc[0]] // tile_length
            for ty in range(per_side):
                for tx in range(per_side):
                    inside = (rows["centroid-0"] >= ty * tile_length) & (rows["centroid-0"] < (ty + 1) * tile_length) & \
                        (rows["centroid-1"] >= tx * tile_length) & (rows["centroid-1"] < (tx + 1) * tile_length)
                    tiles.append(rows[inside])
        _compare_stats(tile_stats.reset_index(drop=True), fr.load_frame(g, p + "tile_"), tiles, means)
        back = pd.read_csv(os.path.join(case_dir, "fiber_stats_table.csv"))
        assert list(back.columns) == list(fov_stats.columns) and len(back) == len(fov_stats)


def fibre_plane():
    """A 130 x 340 int32 label plane: a thin fibre 300 pixels long, a ring, a figure-eight, a label nested in the ring's
    hole, a diagonal, labels with gaps."""
    seg = np.zeros((130, 340), dtype=np.int32)
    for j in range(300):                                  # label 3: 300 long, two pixels thick, slowly descending
        seg[10 + j // 12:12 + j // 12, 20 + j] = 3
    seg[50:59, 10:19] = 7
    seg[52:57, 12:17] = 0                                 # the ring's hole
    seg[54, 14] = 9                                       # nested in it
    seg[70:77, 30:43] = 12
    seg[72:75, 32:35] = 0
    seg[72:75, 38:41] = 0                                 # figure-eight
    for j in range(25):
        seg[90 + j, 100 + j] = 40                         # 8-connected diagonal
    seg[100:118, 200:203] = 41
    return seg


def check_object_props(fs):
    """fiber_object_props over :func:`fibre_plane`: the integers of regionprops_extraction.host_raw and the statement's
    Euler numbers, the float columns bit-equal to the host formula over them."""
    seg = fibre_plane()
    got = fs.fiber_object_props(seg, "fovX")
    assert list(got.columns) == TABLE_COLUMNS
    raw = rpe.host_raw(seg)
    raw["euler"] = fr.euler_by_quads(seg, raw["keys"])
    want = rpe.morphology(raw, orientation=True)
    np.testing.assert_array_equal(got["label"].to_numpy(), [3, 7, 9, 12, 40, 41])
    np.testing.assert_array_equal(got["area"].to_numpy(), raw["count"])
    assert got["area"].to_numpy()[0] == 600 and (got["fov"] == "fovX").all()
    np.testing.assert_array_equal(got["euler_number"].to_numpy(), [1, 0, 1, -1, 1, 1])
    for col in TABLE_COLUMNS[2:]:
        np.testing.assert_array_equal(got[col].to_numpy(), want[col], err_msg=col)
    assert got["euler_number"].dtype == np.int64 and got["area"].dtype == np.int64 and got["label"].dtype == np.int64
    return got


def check_fiber_objects(fs, tmp_dir):
    """fiber_objects = ndi.label, the area filter, the object table; the labels keep their gaps and are saved."""
    from scipy import ndimage
    rs = np.random.RandomState(5)
    mask = ndimage.binary_dilation(rs.uniform(size=(96, 150)) < 0.02, iterations=2) & (rs.uniform(size=(96, 150)) < 0.8)
    table, labels = fs.fiber_objects(mask, "fovY", out_dir=str(tmp_dir), min_fiber_size=15)
    lab, n = ndimage.label(mask)
    areas = np.bincount(lab.ravel(), minlength=n + 1)
    kept = np.flatnonzero(areas >= 15)
    kept = kept[kept != 0]
    assert 0 < kept.size < n and kept[-1] > kept.size              # something is dropped and gaps stay
    np.testing.assert_array_equal(labels, np.where(np.isin(lab, kept), lab, 0))
    np.testing.assert_array_equal(table["label"].to_numpy(), kept)
    np.testing.assert_array_equal(table["area"].to_numpy(), areas[kept])
    np.testing.assert_array_equal(image_io.read_image(os.path.join(str(tmp_dir), "fovY_fiber_labels.tiff")), labels)


def check_table_from_labels(fs, tmp_dir):
    """The cohort call over the label planes of the fixture's small cohort and :func:`fibre_plane`."""
    g = fr.fixture()
    planes = {"s1": g["c_small_plane_s1"], "s2": g["c_small_plane_s2"], "s10": fibre_plane()}
    for fov, plane in planes.items():
        image_io.write_image(os.path.join(str(tmp_dir), fov + "_fiber_labels.tiff"), plane)
    table = _quiet(fs.fiber_object_table_from_labels, str(tmp_dir))
    assert list(table.columns) == TABLE_COLUMNS + ["alignment_score"]
    assert list(pd.unique(table["fov"])) == ["s1", "s2", "s10"]     # natural order
    np.testing.assert_array_equal(table["alignment_score"].to_numpy(), fr.alignment_scores(table[TABLE_COLUMNS]))
    assert np.isfinite(table["alignment_score"].to_numpy()).sum() >= 3
    back = pd.read_csv(os.path.join(str(tmp_dir), "fiber_object_table.csv"))
    assert list(back.columns) == list(table.columns) and len(back) == len(table)
    np.testing.assert_array_equal(back["euler_number"].to_numpy(), table["euler_number"].to_numpy())
    only = _quiet(fs.fiber_object_table_from_labels, str(tmp_dir), fovs=["s10"])
    np.testing.assert_array_equal(only["label"].to_numpy(), [3, 7, 9, 12, 40, 41])


# ---- the fixture and the statements -----------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference is not on this machine")
def test_regenerated_fixture_equals_committed(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_fibers.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    a, b = fr.fixture(), np.load(os.path.join(str(tmp_path), fr.FIXTURE + ".npz"), allow_pickle=False)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLD, fr.FIXTURE + ".npz")) < 512 * 1024


def test_statement_equals_fixture_scores_exactly():
    g = fr.fixture()
    for prefix in ("a_", "t_"):
        table = fr.load_frame(g, prefix)
        for k in g["k_values"].tolist():
            np.testing.assert_array_equal(fr.alignment_scores(table, k), g[prefix + "scores_k%d" % k],
                                          err_msg="%s k=%d" % (prefix, k))
    table = fr.load_frame(g, "a_")
    scores = g["a_scores_k4"]
    ratio = _quiet(lambda: table["major_axis_length"].to_numpy() / table["minor_axis_length"].to_numpy())
    assert np.isinf(ratio).sum() == 6 and np.isfinite(scores[np.isinf(ratio)]).all()      # x / 0 is kept
    assert np.isnan(ratio).sum() == 8 and np.isnan(scores[np.isnan(ratio)]).all()         # 0 / 0 is dropped
    lone = (table["fov"] == "fov1").to_numpy() & (ratio >= 2)
    assert lone.sum() == 1 and scores[lone][0] == 0.0 and not np.signbit(scores[lone][0])


def test_ties_and_identity(fs):
    """Coincident centroids: the statement gives ties to the lower position and never a point itself, and the module's
    scores over such a table are the ones counted by hand."""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 1.0], [5.0, 5.0], [5.0, 5.0]])
    idx = fr.nearest_indices(xy, [0, 4, 6], 3)
    np.testing.assert_array_equal(idx, [[2, 1, 3], [0, 2, 3], [0, 1, 3], [0, 2, 1], [5, -1, -1], [4, -1, -1]])
    assert fr.nearest_indices(np.zeros((0, 2)), [0, 0, 0], 2).shape == (0, 2)
    table = pd.DataFrame({"fov": "f", "label": [1, 2, 3], "centroid-0": [0.0, 0.0, 1.0], "centroid-1": [0.0, 0.0, 0.0],
                          "major_axis_length": 4.0, "minor_axis_length": 1.0, "orientation": [0.125, 0.5, 1.0]})
    got = fs.calculate_fiber_alignment(table, k=1)["alignment_score"].to_numpy()
    np.testing.assert_array_equal(got, [0.375, 0.375, 0.875])      # 1 <-> 2 on one spot; 3 ties between them: the first
    got = fs.calculate_fiber_alignment(table, k=2)["alignment_score"].to_numpy()
    np.testing.assert_array_equal(got, [np.sqrt(0.375 ** 2 + 0.875 ** 2) / 2, np.sqrt(0.375 ** 2 + 0.5 ** 2) / 2,
                                        np.sqrt(0.875 ** 2 + 0.5 ** 2) / 2])


def test_module_equals_fixture(fs):
    check_alignment_cases(fs)


def test_summaries_equal_fixture(fs, tmp_path):
    check_summary_cases(fs, tmp_path)


def test_density_equals_fixture(fs):
    g = fr.fixture()
    for name in ("small", "large"):
        table = fr.load_frame(g, "c_%s_" % name)
        for j, fov in enumerate(str(f) for f in g["c_%s_fovs" % name]):
            side = g["c_%s_plane_%s" % (name, fov)].shape[0]
            assert fs.calculate_density(table[table.fov == fov], side ** 2) == tuple(g["c_%s_density" % name][j])


def test_rank_order_sums_follow_numpy(fs):
    rs = np.random.RandomState(3)
    terms = rs.uniform(0, 3, (50, 32)) ** 7
    counts = rs.randint(0, 33, 50)
    got = fs._rank_order_sums(terms, counts)
    for i in range(50):
        assert got[i] == np.sum(np.ascontiguousarray(terms[i, :counts[i]]))


# ---- Euler numbers and orientations ---------------------------------------------------------------------------------------
def test_euler_by_quads_equals_scipy_labels():
    rs = np.random.RandomState(11)
    for _ in range(400):
        h, w = rs.randint(1, 12, 2)
        mask = rs.uniform(size=(h, w)) < rs.uniform(0.2, 0.8)
        want = fr.euler_by_labels(mask)
        assert fr.euler_by_quads(mask.astype(np.int32) * 5, [5])[0] == want
        assert rpe.euler_numbers(mask.astype(np.int32) * 5, [5])[0] == want


def test_euler_of_several_labels_at_once():
    rs = np.random.RandomState(12)
    for shape in [(1, 1), (1, 7), (2, 2), (17, 23)]:
        seg = rs.randint(0, 4, shape).astype(np.int32) * 1000
        keys = np.array([1000, 1500, 2000, 3000])
        want = [fr.euler_by_labels(seg == k) if (seg == k).any() else 0 for k in keys]
        np.testing.assert_array_equal(rpe.euler_numbers(seg, keys), want)
        np.testing.assert_array_equal(fr.euler_by_quads(seg, keys), want)
    checker = (np.add.outer(np.arange(6), np.arange(9)) % 2 + 1).astype(np.int32)     # every pixel an 8-connected net
    np.testing.assert_array_equal(rpe.euler_numbers(checker, [1, 2]), [fr.euler_by_labels(checker == 1),
                                                                      fr.euler_by_labels(checker == 2)])


def test_ring_figure_eight_and_nested_label(fs):
    got = check_object_props(fs).set_index("label")
    assert got.loc[7, "euler_number"] == 0 and got.loc[12, "euler_number"] == -1
    assert got.loc[9, "euler_number"] == 1 and got.loc[40, "euler_number"] == 1


def _orientation_of(mask):
    seg = np.zeros((mask.shape[0] + 3, mask.shape[1] + 4), dtype=np.int32)
    seg[1:1 + mask.shape[0], 2:2 + mask.shape[1]] = mask * 6
    got = rpe.morphology(rpe.host_raw(seg), orientation=True)["orientation"][0]
    assert got == fr.orientation(*np.nonzero(seg))
    return got


def test_orientation_by_hand():
    assert _orientation_of(np.ones((9, 1), dtype=int)) == 0.0                 # vertical bar
    assert _orientation_of(np.ones((1, 9), dtype=int)) == math.pi / 2         # horizontal bar: +pi/2, not -pi/2
    assert _orientation_of(np.eye(7, dtype=int)) == -math.pi / 4              # main diagonal
    assert _orientation_of(np.eye(7, dtype=int)[::-1]) == math.pi / 4         # anti-diagonal
    assert _orientation_of(np.ones((4, 4), dtype=int)) == math.pi / 4         # a == d, b = -0.0: not below 0
    rs = np.random.RandomState(2)
    for _ in range(20):
        got = _orientation_of((rs.uniform(size=(rs.randint(2, 9), rs.randint(2, 30))) < 0.6).astype(int) | np.eye(1, dtype=int))
        assert -math.pi / 2 <= got <= math.pi / 2


def test_cell_table_property_lists_accept_the_new_columns():
    base, single, _ = rpe.resolve_lists(["area", "orientation", "euler_number"], [], [])
    frame = rpe.props_frame(rpe.host_raw(fibre_plane(), euler=True), base, single)
    assert "euler" not in rpe.host_raw(fibre_plane()) and "orientation" not in rpe.morphology(rpe.host_raw(fibre_plane()))
    assert list(frame.columns) == ["label", "area", "orientation", "euler_number", "centroid-0", "centroid-1"]
    np.testing.assert_array_equal(frame["euler_number"].to_numpy(), [1, 0, 1, -1, 1, 1])
    with pytest.raises(NotImplementedError, match="solidity"):
        rpe.resolve_lists(["solidity"], [], [])


# ---- the module through the stand-ins ---------------------------------------------------------------------------------
def test_fiber_objects(fs, tmp_path):
    check_fiber_objects(fs, tmp_path)


def test_table_from_labels(fs, tmp_path):
    check_table_from_labels(fs, tmp_path)


def test_empty_tables(fs, tmp_path):
    empty = fs.fiber_object_props(np.zeros((5, 9), dtype=np.uint16), "fovE")
    assert list(empty.columns) == TABLE_COLUMNS and len(empty) == 0
    scored = fs.calculate_fiber_alignment(empty)
    assert list(scored.columns) == TABLE_COLUMNS + ["alignment_score"] and len(scored) == 0
    image_io.write_image(os.path.join(str(tmp_path), "fovE_fiber_labels.tiff"), np.zeros((5, 9), dtype=np.uint16))
    table = fs.fiber_object_table_from_labels(str(tmp_path))
    assert len(table) == 0 and os.path.exists(os.path.join(str(tmp_path), "fiber_object_table.csv"))
    none = fs.calculate_fiber_alignment(pd.DataFrame({
        "fov": ["f", "f"], "label": [1, 2], "centroid-0": [0.0, 1.0], "centroid-1": [0.0, 1.0],
        "major_axis_length": [1.0, 1.0], "minor_axis_length": [1.0, 1.0], "orientation": [0.1, 0.2]}))
    assert np.isnan(none["alignment_score"].to_numpy(dtype=np.float64)).all()


def test_save_tiles_leaves_the_image_intact(fs, tmp_path):
    g = fr.fixture()
    table = fr.load_frame(g, "c_small_")
    plane = g["c_small_plane_s1"].copy()
    before = plane.copy()
    assert before.max() > 1
    stats = fs.generate_tile_stats(table[table.fov == "s1"], plane, 32, 8, 1, str(tmp_path), True)
    np.testing.assert_array_equal(plane, before)
    assert len(stats) == 16
    for ty in range(0, 32, 8):
        for tx in range(0, 32, 8):
            tile = image_io.read_image(os.path.join(str(tmp_path), "s1", "tile_%d,%d.tiff" % (ty, tx)))
            np.testing.assert_array_equal(tile, (before[ty:ty + 8, tx:tx + 8] > 0).astype(before.dtype))


def test_argument_errors(fs, tmp_path):
    g = fr.fixture()
    table = fr.load_frame(g, "c_small_")
    with pytest.raises(ValueError, match="Tile length must be a factor"):
        fs.generate_summary_stats(table, str(tmp_path), tile_length=7)
    with pytest.raises(FileNotFoundError):
        fs.generate_summary_stats(table, os.path.join(str(tmp_path), "absent"))
    with pytest.raises(FileNotFoundError):
        fs.fiber_object_table_from_labels(str(tmp_path), fovs=["absent"])
    with pytest.raises(ValueError, match="fiber_labels"):
        fs.fiber_object_table_from_labels(str(tmp_path))
    with pytest.raises(NotImplementedError, match="solidity.*euler_number"):
        fs.fiber_object_props(np.ones((3, 3), dtype=np.int32), "f", object_properties=("label", "solidity"))
    with pytest.raises(NotImplementedError, match="k <= 32"):
        fs.calculate_fiber_alignment(fr.load_frame(g, "t_"), k=33)
    with pytest.raises(ValueError, match="at least 1"):
        fs.calculate_fiber_alignment(fr.load_frame(g, "t_"), k=0)
    with pytest.raises(ValueError, match="non-empty"):
        fs.fiber_objects(np.zeros((0, 4)), "f")


def test_entries_that_are_not_built(fs, tmp_path):
    data_dir, out_dir = os.path.join(str(tmp_path), "data"), os.path.join(str(tmp_path), "out")
    os.makedirs(os.path.join(data_dir, "fov1"))
    os.makedirs(out_dir)
    image_io.write_image(os.path.join(data_dir, "fov1", "Collagen1.tiff"), np.zeros((4, 4), dtype=np.uint16))
    for call in (lambda: fs.run_fiber_segmentation(data_dir, "Collagen1", out_dir),
                 lambda: fs.plot_fiber_segmentation_steps(data_dir, "fov1", "Collagen1"),
                 lambda: fs.segment_fibers(None, "Collagen1", out_dir, "fov1")):
        with pytest.raises(NotImplementedError, match="frangi.*fiber_objects.*fiber_object_table_from_labels"):
            call()
    with pytest.raises(FileNotFoundError):
        fs.run_fiber_segmentation(os.path.join(str(tmp_path), "absent"), "Collagen1", out_dir)
    with pytest.raises(FileNotFoundError):
        fs.run_fiber_segmentation(data_dir, "Collagen1", os.path.join(str(tmp_path), "absent"))
    with pytest.raises(ValueError, match="fiber_channel"):
        fs.run_fiber_segmentation(data_dir, "bad_channel", out_dir)
    with pytest.raises(FileNotFoundError):
        fs.plot_fiber_segmentation_steps(os.path.join(str(tmp_path), "absent"), "fov1", "Collagen1")
    with pytest.raises(ValueError, match="fiber_channel"):
        fs.plot_fiber_segmentation_steps(data_dir, "fov1", "bad_channel")
    with pytest.raises(FileNotFoundError):
        fs.segment_fibers(None, "Collagen1", os.path.join(str(tmp_path), "absent"), "fov1")


# ---- the ABI and the entries without a device -----------------------------------------------------------------------------
def test_new_symbols_resolve_and_refuse_bad_arguments():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    assert lib.pxsom_abi_version() == _capi.ABI_VERSION == 9
    for name in ("pxsom_region_euler_workspace_bytes", "pxsom_region_euler", "pxsom_nearest_indices"):
        assert name in _capi.SYMBOLS and getattr(lib, name) is not None
    assert lib.pxsom_region_euler_workspace_bytes(10, 1, 10, 0) == 256
    assert lib.pxsom_region_euler_workspace_bytes(10, 1, 10, 1) == 0
    assert lib.pxsom_region_euler_workspace_bytes(2, 1, 2 ** 31 - 1, 0) == 0
    bad = -1
    one = 1 << 12                                        # a non-null address that is never dereferenced
    assert lib.pxsom_nearest_indices(one, one, 1, 5, 0, one, None) == bad          # k
    assert lib.pxsom_nearest_indices(one, one, 1, 5, 33, one, None) == bad
    assert lib.pxsom_nearest_indices(one, one, 1, -1, 4, one, None) == bad         # n
    assert lib.pxsom_nearest_indices(one, None, 1, 5, 4, one, None) == bad         # seg
    assert lib.pxsom_nearest_indices(None, one, 1, 5, 4, one, None) == bad         # xy
    assert lib.pxsom_nearest_indices(one + 8, one, 1, 5, 4, one, None) == bad      # alignment
    assert lib.pxsom_nearest_indices(one, one, 1, 2 ** 31, 4, one, None) == bad    # int32 positions
    assert b"pxsom_nearest_indices" in lib.pxsom_last_error()
    assert lib.pxsom_region_euler(one, 9, 8, 4, 8, one, 2, 1, 2, one, one, 256, 0, None) == bad     # dtype
    assert lib.pxsom_region_euler(one, 3, 7, 4, 8, one, 2, 1, 2, one, one, 256, 0, None) == bad     # ld < w
    assert lib.pxsom_region_euler(one, 3, 8, 0, 8, one, 2, 1, 2, one, one, 256, 0, None) == bad     # h
    assert lib.pxsom_region_euler(one, 3, 8, 4, 8, one, 2, 1, 2, one, one, 256, 2, None) == bad     # flags
    assert lib.pxsom_region_euler(one, 3, 2 ** 31 - 1, 4, 2 ** 31 - 100, one, 2, 1, 2, one, one, 256, 0, None) == bad   # w
    assert lib.pxsom_region_euler(one, 3, 8, 2 ** 31 - 128, 8, one, 2, 1, 2, one, one, 256, 0, None) == bad  # h
    assert lib.pxsom_region_euler(None, 3, 8, 4, 8, one, 2, 1, 2, one, one, 256, 0, None) == bad    # image
    assert lib.pxsom_region_euler(one, 3, 8, 4, 8, one, 2, 1, 2, None, one, 256, 0, None) == bad    # output
    assert lib.pxsom_region_euler(one, 3, 8, 4, 8, one, 2, 2, 1, one, one, 256, 0, None) == bad     # key range
    assert lib.pxsom_region_euler(one, 3, 8, 4, 8, one, 2, 1, 2, one, one, 8, 0, None) == bad       # workspace
    assert b"pxsom_region_euler" in lib.pxsom_last_error()


def test_wrappers_refuse_bad_arguments_without_a_device():
    import torch
    from ark_analysis_amd import som_device
    xy, seg = torch.zeros((4, 2), dtype=torch.float64), torch.tensor([0, 4])
    for k in (0, 33):
        with pytest.raises(ValueError, match="1 .. 32"):
            som_device.nearest_indices(xy, seg, k)
    with pytest.raises(ValueError, match="float64 HBM"):
        som_device.nearest_indices(xy, seg, 4)
    plane = torch.zeros((4, 4), dtype=torch.int32)
    for call in (som_device.region_euler, som_device.region_moments):
        with pytest.raises(ValueError, match="HBM"):
            call(plane)
        with pytest.raises(ValueError, match="HBM"):
            call(plane.to(torch.float32))
