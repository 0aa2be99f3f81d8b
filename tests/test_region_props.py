"""The morphology regionprops of generate_cell_table(fast_extraction=False) on CPU: answers counted by
hand, the host formulas and the host route against tests/region_props_reference.py, generate_cell_table with the property
lists named through a host stand-in for the device entry points, and a two-rank gloo run.

``install_host_stand_in`` and ``morph_cohort`` are shared with tests/test_gpu_region_props.py."""
import os
import warnings

import numpy as np
import pandas as pd
import pytest

from ark_analysis_amd.segmentation import regionprops_extraction as rpe
from tests import cell_table_reference as ctr
from tests import region_props_reference as rpr
from tests.test_cell_table import _free_port, _numpy_quantify, write_cohort

BASE_COLS = ["area", "eccentricity", "major_axis_length", "minor_axis_length", "perimeter", "convex_area",
             "equivalent_diameter", "centroid-0", "centroid-1"]
SINGLE_COLS = list(rpe.REGIONPROPS_SINGLE_COMP)


def _host_region_raw(seg, q=None, **thresholds):
    return rpe.host_raw(seg, **thresholds)


def install_host_stand_in(setattr_):
    from ark_analysis_amd.segmentation import marker_quantification as mq
    setattr_(mq, "_upload_image", np.ascontiguousarray)
    setattr_(mq, "_quantify", _numpy_quantify)
    setattr_(mq, "_region_raw", _host_region_raw)


@pytest.fixture
def mq(monkeypatch):
    install_host_stand_in(monkeypatch.setattr)
    from ark_analysis_amd.segmentation import marker_quantification
    return marker_quantification


def _one(mask, pad=2, **thresholds):
    """The columns of a single shape placed in an image with ``pad`` pixels of background around it."""
    mask = np.asarray(mask, dtype=bool)
    seg = np.zeros((mask.shape[0] + 2 * pad, mask.shape[1] + 2 * pad), dtype=np.int32)
    seg[pad:pad + mask.shape[0], pad:pad + mask.shape[1]] = mask * 7
    raw = rpe.host_raw(seg, **thresholds)
    cols = rpe.morphology(raw)
    if not thresholds:
        rpr.compare(raw, cols, rpr.reference(seg))
    return {k: v[0] for k, v in cols.items()}


# ---- answers counted by hand ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", [(2, 2), (2, 9), (3, 5), (6, 4), (13, 13)])
def test_rectangle(h, w):
    c = _one(np.ones((h, w)))
    assert c["area"] == h * w == c["convex_area"] and c["num_concavities"] == 0
    assert c["perimeter"] == 2 * h + 2 * w - 4
    axes = sorted([4 * np.sqrt((h * h - 1) / 12), 4 * np.sqrt((w * w - 1) / 12)])
    np.testing.assert_allclose([c["minor_axis_length"], c["major_axis_length"]], axes, rtol=1e-14)
    assert c["convex_hull_resid"] == 0 and c["centroid_dif"] == 0


def test_single_pixel():
    c = _one(np.ones((1, 1)))
    assert c["area"] == 1 and c["convex_area"] == 1 and c["num_concavities"] == 0
    assert c["perimeter"] == 0 and c["major_axis_length"] == 0 and c["minor_axis_length"] == 0
    assert c["eccentricity"] == 0 and np.isnan(c["major_minor_axis_ratio"])
    assert c["perim_square_over_area"] == 0 and c["centroid_dif"] == 0 and c["convex_hull_resid"] == 0
    assert c["equivalent_diameter"] == np.sqrt(4 / np.pi)


@pytest.mark.parametrize("n, vertical", [(2, False), (7, False), (7, True), (40, True)])
def test_lines(n, vertical):
    c = _one(np.ones((n, 1) if vertical else (1, n)))
    assert c["area"] == n == c["convex_area"] and c["num_concavities"] == 0
    assert c["perimeter"] == n - 2                  # the two ends have one border neighbour: code 3, weight 0
    assert c["minor_axis_length"] == 0 and np.isnan(c["major_minor_axis_ratio"]) and c["eccentricity"] == 1
    np.testing.assert_allclose(c["major_axis_length"], 4 * np.sqrt((n * n - 1) / 12), rtol=1e-14)


def test_diagonal_staircase():
    n = 9
    c = _one(np.eye(n))
    assert c["area"] == n == c["convex_area"]       # the hull's long edges are c - r = +-1/2: no other centre inside
    assert c["perimeter"] == (n - 2) * np.sqrt(2.0)  # inner pixels: two diagonal border neighbours, code 21
    assert c["minor_axis_length"] == 0 and np.isnan(c["major_minor_axis_ratio"])
    np.testing.assert_allclose(c["major_axis_length"], 4 * np.sqrt(2 * (n * n - 1) / 12), rtol=1e-14)


def test_l_plus_and_c():
    l_shape = np.ones((4, 4), dtype=bool)
    l_shape[:2, 2:] = False
    c = _one(l_shape)
    assert c["area"] == 12 and c["convex_area"] == 13 and c["num_concavities"] == 0    # the edge c - r = 3/2 takes (1, 2)
    plus = np.zeros((5, 5), dtype=bool)
    plus[2, :] = plus[:, 2] = True
    c = _one(plus)
    assert c["area"] == 9 and c["convex_area"] == 13       # the edges r + c = 3/2, ...: one centre per quadrant
    assert c["centroid_dif"] == 0
    small_plus = np.zeros((3, 3), dtype=bool)
    small_plus[1, :] = small_plus[:, 1] = True
    assert _one(small_plus)["convex_area"] == 5
    c = _one(rpr.c_shape(7, 3))
    assert c["area"] == 34 and c["convex_area"] == 49
    assert c["num_concavities"] == 1                        # 3 x 5 = 15 px > 10, p = 12, p^2 / a = 9.6 < 60
    np.testing.assert_allclose(c["convex_hull_resid"], 15 / 49, rtol=1e-15)
    assert c["centroid_dif"] > 0


def test_ring_concavities():
    assert _one(rpr.ring(17, 13))["num_concavities"] == 1           # 169 px > 150
    assert _one(rpr.ring(9, 3))["num_concavities"] == 0             # 9 px <= 10
    assert _one(rpr.ring(10, 4))["num_concavities"] == 1            # 16 px > 10, p = 12, p^2 / a = 9 < 60
    slit = np.ones((3, 102), dtype=bool)
    slit[1, 1:101] = False                                          # 100 px <= 150, p = 98, p^2 / a = 96.04 > 60
    assert _one(slit)["num_concavities"] == 0
    assert _one(slit, max_compactness=100)["num_concavities"] == 1
    assert _one(slit, large_concavity_minimum=99)["num_concavities"] == 1
    assert _one(rpr.ring(10, 4), small_concavity_minimum=16)["num_concavities"] == 0


def test_thin_cells_keep_their_minor_axis():
    """Cells whose l2 is far below l1: the minor axis is held at relative 1e-12 against the exact root (_one compares),
    which the form l2 = trace - l1 cannot meet here (its error is eps * l1 against an l2 10^5 .. 10^7 times smaller)."""
    for n in (60, 200, 500):
        line = np.zeros((2, n), dtype=bool)
        line[0, :] = True
        line[1, n - 1] = True                  # one pixel off the line
        c = _one(line)
        assert 0 < c["minor_axis_length"] < 1 and c["major_axis_length"] > n
        assert np.isfinite(c["major_minor_axis_ratio"])
        c = _one(line.T)
        assert 0 < c["minor_axis_length"] < 1


def notched(h=6, w=7, rows=(2, 4), cols=(2, 7)):
    """A block with a notch open to the right edge: the hull is the block, the notch its one concavity -- by default
    2 x 5 = 10 px (p = 2 * 2 + 2 * 5 - 4 = 10, p^2 / a = 10), an area exactly on small_concavity_minimum."""
    m = np.ones((h, w), dtype=bool)
    m[rows[0]:rows[1], cols[0]:cols[1]] = False
    return m


def test_concavity_area_on_a_threshold():
    """'a > minimum', not '>=': integer areas, so no ulp is involved.  (The reference refuses such an image, by design;
    the answers here are counted by hand.)"""
    assert _one(notched(), small_concavity_minimum=10)["num_concavities"] == 0
    assert _one(notched(), small_concavity_minimum=9)["num_concavities"] == 1
    assert _one(notched(), max_compactness=5, large_concavity_minimum=10)["num_concavities"] == 0
    assert _one(notched(), max_compactness=5, large_concavity_minimum=9)["num_concavities"] == 1
    assert _one(notched(), small_concavity_minimum=9, max_compactness=10)["num_concavities"] == 0      # p^2 / a = 100 / 10 exactly: '<', not '<='
    assert _one(notched(), small_concavity_minimum=9, max_compactness=10.5)["num_concavities"] == 1


# ---- the host formulas and the host route against the reference ---------------------------------------------------
@pytest.mark.parametrize("h, w, cells, seed", [(64, 64, 20, 1), (90, 131, 40, 2), (33, 200, 12, 3)])
def test_host_route_equals_reference(h, w, cells, seed):
    seg, ref = rpr.settled(lambda s: ctr.fragment(rpr.voronoi(h, w, cells, seed=s), [3], pieces=4, seed=s), seed)
    raw = rpe.host_raw(seg)
    rpr.compare(raw, rpe.morphology(raw), ref)


def test_fill_left_out_and_frame():
    seg = ctr.voronoi_labels(80, 80, 6, seed=5)
    raw = rpe.host_raw(seg)
    part = {k: np.array(v) for k, v in raw.items()}
    part["hull"][[0, 2]] = 0
    part["left_out"][[0, 2]] = 1
    rpe.fill_left_out(part, seg)
    for k in raw:
        np.testing.assert_array_equal(part[k], raw[k])
    base, single, _ = rpe.resolve_lists(None, None, None)
    frame = rpe.props_frame(raw, base, single)
    assert list(frame.columns) == ["label", "area", "eccentricity", "major_axis_length", "minor_axis_length",
                                   "perimeter", "centroid-0", "centroid-1", "convex_area", "equivalent_diameter"] + \
        SINGLE_COLS
    assert frame["label"].dtype == np.int64 and frame["area"].dtype == np.int64
    assert frame["convex_area"].dtype == np.int64 and frame["num_concavities"].dtype == np.int64


def test_resolve_lists_errors():
    with pytest.raises(ValueError, match="extras_props"):
        rpe.resolve_lists(None, ["bad_prop"], None)
    with pytest.raises(ValueError, match="nuclear_props"):
        rpe.resolve_lists(None, None, ["bad_prop"])
    with pytest.raises(NotImplementedError, match="solidity"):
        rpe.resolve_lists(["label", "solidity"], None, None)
    base, single, multi = rpe.resolve_lists(["area", "coords"], [], [])
    assert base == ["label", "area", "centroid"] and single == [] and multi == []
    assert rpe.table_names(base, single) == ["area", "centroid-0", "centroid-1"]


# ---- generate_cell_table with the lists named ---------------------------------------------------------------------------
def morph_cohort(n_fovs=2, h=48, w=60, c=2, seed=0):
    """A small cohort whose whole-cell and nuclear images both keep the reference's margin (rpr.settled)."""
    rs = np.random.RandomState(seed)
    fovs = ["fov%d" % i for i in range(n_fovs)]
    channels = ["chan%d" % j for j in range(c)]
    images, segs = {}, {}

    def both(s):
        seg = rpr.voronoi(h, w, 14, seed=s)
        # a nucleus inside every odd cell: the cell's pixels two steps away from any other label
        return np.stack([seg, np.where((seg % 2 == 1) & ndimage_core(seg), seg + 1000, 0).astype(np.int32)])
    for i, fov in enumerate(fovs):
        images[fov] = (rs.gamma(0.7, 4.0, size=(h, w, c)) * (rs.rand(h, w, c) < 0.8)).astype(np.float32)
        pair = both(seed * 10 + i + 1)
        segs[fov + "_whole_cell.tiff"] = rpr.reference(pair[0], drop=True)[0]
        segs[fov + "_nuclear.tiff"] = rpr.reference(pair[1], drop=True)[0]
    return fovs, channels, images, segs


def ndimage_core(seg):
    from scipy import ndimage
    same = np.ones(seg.shape, dtype=bool)
    for axis in (0, 1):
        for shift in (-2, -1, 1, 2):
            same &= np.roll(seg, shift, axis=axis) == seg
    return same & ndimage.binary_erosion(seg > 0, iterations=2)


def _expected_names(channels, nuclear, with_ratio):
    names = ["cell_size"] + channels + ["label"] + BASE_COLS + SINGLE_COLS + (["nc_ratio"] if with_ratio else [])
    if nuclear:
        names = names + [n + "_nuclear" for n in names]
    return names + ["fov", "mask_type"]


def test_cell_table_with_lists_fails_on_parent(mq, tmp_path):
    """The call the parent commit refuses: fast_extraction=False with a property list named."""
    fovs, channels, images, segs = morph_cohort()
    seg_dir, tiff_dir = write_cohort(str(tmp_path), images, segs, channels)
    norm, asinh = mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=False,
                                         regionprops_base=list(rpe.REGIONPROPS_BASE))
    assert list(norm.columns) == _expected_names(channels, False, False) == list(asinh.columns)
    assert norm["label"].dtype == np.int32
    assert all(norm[c].dtype == np.float64 for c in BASE_COLS + SINGLE_COLS + ["cell_size"] + channels)
    fast, fast_asinh = mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=True,
                                              regionprops_base=["nonsense"])          # the lists are ignored
    shared = list(fast.columns)
    pd.testing.assert_frame_equal(norm[shared], fast, check_exact=True)
    pd.testing.assert_frame_equal(asinh[shared], fast_asinh, check_exact=True)
    pd.testing.assert_frame_equal(norm[BASE_COLS + SINGLE_COLS], asinh[BASE_COLS + SINGLE_COLS], check_exact=True)
    np.testing.assert_array_equal(norm["area"], norm["cell_size"])
    for fov in fovs:
        ref = rpr.reference(segs[fov + "_whole_cell.tiff"])
        part = norm[norm["fov"] == fov]
        np.testing.assert_array_equal(part["label"], ref["keys"])
        np.testing.assert_array_equal(part["convex_area"], ref["hull"][:, 0])
        np.testing.assert_array_equal(part["num_concavities"], ref["hull"][:, 3])
        np.testing.assert_allclose(part["perimeter"], ref["perimeter"], rtol=1e-13, atol=0)
        np.testing.assert_allclose(part["centroid_dif"], ref["centroid_dif"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(part["major_axis_length"], ref["major_axis_length"], rtol=1e-12, atol=0)


def test_cell_table_nuclear_and_nc_ratio(mq, tmp_path):
    fovs, channels, images, segs = morph_cohort()
    segs["fov1_nuclear.tiff"] = np.zeros_like(segs["fov1_nuclear.tiff"])       # no nucleus anywhere in fov1
    seg_dir, tiff_dir = write_cohort(str(tmp_path), images, segs, channels)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        per_fov = {f: mq.generate_cell_table(seg_dir, tiff_dir, fovs=[f], nuclear_counts=True,
                                             regionprops_multi_comp=["nc_ratio"])[0] for f in fovs}
    assert [str(w.message) for w in wl if "nuclei" in str(w.message)] == [
        "No nuclei found in the following image: fov1"]
    assert list(per_fov["fov0"].columns) == _expected_names(channels, True, True)
    assert list(per_fov["fov1"].columns) == _expected_names(channels, True, False)     # the reference's quirk
    t = per_fov["fov0"]
    has = t["label_nuclear"] > 0
    assert has.any() and (~has).any()
    np.testing.assert_array_equal(t["nc_ratio"], t["area_nuclear"] / t["area"])
    np.testing.assert_array_equal(t["nc_ratio"], t["nc_ratio_nuclear"])
    assert (t.loc[~has, [c for c in t.columns if c.endswith("_nuclear")]] == 0).all().all()
    nuc_ref = rpr.reference(segs["fov0_nuclear.tiff"])
    rows = np.searchsorted(nuc_ref["keys"], t.loc[has, "label_nuclear"].to_numpy().astype(np.int64))
    np.testing.assert_array_equal(t.loc[has, "convex_area_nuclear"], nuc_ref["hull"][rows, 0])
    np.testing.assert_allclose(t.loc[has, "perimeter_nuclear"], nuc_ref["perimeter"][rows], rtol=1e-13, atol=0)
    both = mq.generate_cell_table(seg_dir, tiff_dir, nuclear_counts=True, regionprops_multi_comp=["nc_ratio"])[0]
    assert "nc_ratio" in both.columns and both.loc[both["fov"] == "fov1", "nc_ratio"].isna().all()
    none = mq.generate_cell_table(seg_dir, tiff_dir, fovs=["fov0"], nuclear_counts=True, regionprops_multi_comp=[],
                                  regionprops_single_comp=["num_concavities"])[0]
    assert "nc_ratio" not in none.columns and "num_concavities_nuclear" in none.columns


def test_cell_table_thresholds_empty_and_errors(mq, tmp_path):
    fovs, channels, images, segs = morph_cohort(n_fovs=2, h=40, w=110)
    slit = np.zeros((40, 110), dtype=np.int32)
    slit[5:8, 4:106] = 9
    slit[6, 5:105] = 0
    segs["fov0_whole_cell.tiff"] = slit
    segs["fov1_whole_cell.tiff"] = np.zeros((40, 110), dtype=np.int32)
    seg_dir, tiff_dir = write_cohort(str(tmp_path), images, segs, channels)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        plain = mq.generate_cell_table(seg_dir, tiff_dir, regionprops_single_comp=["num_concavities"])[0]
        loose = mq.generate_cell_table(seg_dir, tiff_dir, regionprops_single_comp=["num_concavities"],
                                       regionprops_kwargs={"max_compactness": 100})[0]
    assert [str(w.message) for w in wl] == ["No cells found in the following image: fov1"] * 2
    assert list(plain["fov"]) == ["fov0"] and list(plain["num_concavities"]) == [0]
    assert list(loose["num_concavities"]) == [1]
    assert list(plain.columns) == ["cell_size"] + channels + ["label"] + BASE_COLS + ["num_concavities", "fov",
                                                                                       "mask_type"]
    empty = mq.get_single_compartment_props(np.zeros((8, 9), dtype=np.int32), list(rpe.REGIONPROPS_BASE),
                                            list(rpe.REGIONPROPS_SINGLE_COMP))
    assert len(empty) == 0 and "centroid-0" in empty.columns and "num_concavities" in empty.columns
    frame = mq.get_single_compartment_props(slit, ["label", "area", "centroid"], ["num_concavities"],
                                            large_concavity_minimum=50)
    assert list(frame.columns) == ["label", "area", "centroid-0", "centroid-1", "num_concavities"]
    assert frame.iloc[0].tolist() == [9, 206, 6.0, 54.5, 1]
    with pytest.raises(ValueError, match="extras_props"):
        mq.generate_cell_table(seg_dir, tiff_dir, regionprops_single_comp=["bad_prop"])
    with pytest.raises(NotImplementedError, match="solidity"):
        mq.generate_cell_table(seg_dir, tiff_dir, regionprops_base=["label", "solidity"])
    with pytest.raises(NotImplementedError, match="split_large_nuclei"):
        mq.generate_cell_table(seg_dir, tiff_dir, regionprops_base=["area"], split_large_nuclei=True)
    with pytest.raises(NotImplementedError, match="MIBItiff"):
        mq.generate_cell_table(seg_dir, tiff_dir, regionprops_base=["area"], is_mibitiff=True)


def test_bare_call_still_raises(mq, tmp_path):
    fovs, channels, images, segs = morph_cohort(n_fovs=1)
    seg_dir, tiff_dir = write_cohort(str(tmp_path), images, segs, channels)
    with pytest.raises(NotImplementedError, match="fast_extraction=True is what runs"):
        mq.generate_cell_table(seg_dir, tiff_dir)
    with pytest.raises(NotImplementedError, match="fast_extraction=True is what runs"):
        mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=False, nuclear_counts=True)


def test_abi_has_the_region_entries():
    from ark_analysis_amd import _capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "pxsom.h")).read()
    for name in ("pxsom_region_shape_workspace_bytes", "pxsom_region_shape", "pxsom_region_hull"):
        assert name in _capi.SYMBOLS and name + "(" in header
    lib = _capi.lib()
    # bad arguments are refused before any HIP call (no GPU here)
    assert lib.pxsom_region_shape_workspace_bytes(0, 0, 0, 0) == 0
    assert lib.pxsom_region_shape_workspace_bytes(100, 1, 100, 0) == 512
    assert lib.pxsom_region_shape_workspace_bytes(100, 1, 100, 1) == 0
    assert lib.pxsom_region_shape(None, 3, 8, 8, 8, None, 0, 0, 0, None, None, None, None, None, 0, 0, None) < 0
    assert lib.pxsom_region_shape(1, 9, 8, 8, 8, None, 0, 0, 0, None, None, None, None, None, 0, 0, None) < 0
    assert lib.pxsom_region_shape(1, 3, 4, 8, 8, None, 0, 0, 0, None, None, None, None, None, 0, 0, None) < 0
    assert lib.pxsom_region_shape(1, 3, 8, 8, 8, None, 0, 0, 0, None, None, None, None, None, 0, 2, None) < 0
    assert lib.pxsom_region_shape(1, 3, 8, 8, 8, None, 5, 1, 9, None, None, None, None, None, 0, 0, None) < 0
    assert lib.pxsom_region_hull(None, 3, 8, 8, 8, None, 0, None, None, 10.0, 60.0, 150.0, None, None, None) < 0
    assert lib.pxsom_region_hull(1, 3, 8, 8, 8, None, 0, None, None, float("nan"), 60.0, 150.0, None, None, None) < 0
    assert lib.pxsom_region_hull(1, 3, 8, 8, 8, None, 3, None, None, 10.0, 60.0, 150.0, None, None, None) < 0
    assert lib.pxsom_region_shape(1, 3, 8, 8, 8, None, 0, 0, 0, None, None, None, None, None, 0, 0, None) == 0


# ---- two ranks (gloo) ---------------------------------------------------------------------------------------------------
def _worker(rank, world, port, td, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from tests import oracle_backend
    install_host_stand_in(setattr)
    oracle_backend.join_cpu_group(rank, world)
    from ark_analysis_amd import distributed as d
    d.init_from_env()
    from ark_analysis_amd.segmentation import marker_quantification as mq
    norm, asinh = mq.generate_cell_table(os.path.join(td, "seg"), os.path.join(td, "tiffs"), nuclear_counts=True,
                                         regionprops_multi_comp=["nc_ratio"])
    norm.to_pickle(out_path % (rank, "norm"))
    asinh.to_pickle(out_path % (rank, "asinh"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_generate_cell_table_with_morphology(mq, tmp_path):
    import torch.multiprocessing as mp
    fovs, channels, images, segs = morph_cohort(n_fovs=3)
    td = str(tmp_path)
    write_cohort(td, images, segs, channels)
    single = mq.generate_cell_table(os.path.join(td, "seg"), os.path.join(td, "tiffs"), nuclear_counts=True,
                                    regionprops_multi_comp=["nc_ratio"])
    out_path = os.path.join(td, "rank%d_%s.pkl")
    mp.start_processes(_worker, args=(2, _free_port(), td, out_path), nprocs=2, join=True, start_method="spawn")
    for r in range(2):
        pd.testing.assert_frame_equal(pd.read_pickle(out_path % (r, "norm")), single[0], check_exact=True)
        pd.testing.assert_frame_equal(pd.read_pickle(out_path % (r, "asinh")), single[1], check_exact=True)
