"""split_large_nuclei without a GPU: the loop statement, the vectorised statement and the reference's own
outputs (g24) agree; the host choice (som_device.choose_splits) on hand tables and through a numpy stand-in of the two
device passes; generate_cell_table's wiring; every error; and the properties of the planes the GPU tests run on."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import split_nuclei_reference as snr
from tests.test_cell_table import _compare_frames, _fixture_case, install_host_stand_in, write_cohort

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g24():
    return np.load(os.path.join(GOLD, "g24_split_nuclei.npz"), allow_pickle=False)


def split_cases():
    g = _g24()
    for name in g["split_names"]:
        p = "s_%s_" % name
        yield str(name), g[p + "cell"], g[p + "nuc"], g[p + "ids"], int(g[p + "min_size"]), g[p + "out"]


# ---- the numpy stand-in of the device chain: the tables by numpy, the choice by the product's choose_splits ---------
def numpy_apply(cell, nuc, ck, nk, chosen, cell_value, nuc_value):
    """pxsom_split_apply's contract in numpy."""
    ci = np.where(np.isin(cell, ck), np.searchsorted(ck, cell), -1) if ck.size else np.full(cell.shape, -1)
    ni = np.where(np.isin(nuc, nk), np.searchsorted(nk, nuc), -1) if nk.size else np.full(nuc.shape, -1)
    cs, ns = np.clip(ci, 0, max(ck.size - 1, 0)), np.clip(ni, 0, max(nk.size - 1, 0))
    out = nuc.astype(np.int64)
    if nk.size:
        out = np.where(ni >= 0, nuc_value[ns], out)
        if ck.size:
            takes = (ci >= 0) & (ni >= 0) & (chosen[cs] == ni) & (cell_value[cs] >= 0)
            out = np.where(takes, cell_value[cs], out)
    return out.astype(nuc.dtype)


def numpy_split_device(cell, nuc, cell_ids, min_size, small=5):
    from ark_analysis_amd import som_device
    ck, nk, best, inside, area = snr.pair_tables(cell, nuc)
    chosen, cell_value, nuc_value, _ = som_device.choose_splits(ck, nk, best, inside, area, cell_ids, min_size, small,
                                                                dtype=nuc.dtype)
    return numpy_apply(cell, nuc, ck, nk, chosen, cell_value, nuc_value)


@pytest.fixture
def seg_utils(monkeypatch):
    from ark_analysis_amd.segmentation import segmentation_utils
    monkeypatch.setattr(segmentation_utils, "_split_device", numpy_split_device)
    return segmentation_utils


# ---- statements and fixture ---------------------------------------------------------------------------------------
def test_loop_statement_equals_vectorised_statement_equals_fixture():
    n = 0
    for name, cell, nuc, ids, min_size, want in split_cases():
        loop, n_loop = snr.split_loop(cell, nuc, ids, min_size)
        vec, n_vec = snr.split_vec(cell, nuc, ids, min_size)
        assert loop.dtype == vec.dtype == want.dtype == nuc.dtype, name
        np.testing.assert_array_equal(loop, want, err_msg=name)
        np.testing.assert_array_equal(vec, want, err_msg=name)
        assert n_loop == n_vec >= 1, name
        n += 1
    assert n >= 9


def test_statements_agree_on_the_gpu_cases():
    rng = np.random.default_rng(1)
    for h, w, n, seed in ((96, 130, 40, 3), (200, 257, 150, 5)):
        cell, nuc = snr.voronoi_case(h, w, n, seed)
        for kind in snr.ID_KINDS:
            ids = snr.ids_of(kind, cell, rng)
            for min_size in (0, 15):
                a, b = snr.split_loop(cell, nuc, ids, min_size), snr.split_vec(cell, nuc, ids, min_size)
                np.testing.assert_array_equal(a[0], b[0])
                assert a[1] == b[1]


@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference is not on this machine")
def test_regenerated_fixtures_equal_committed(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_split_nuclei.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    a, b = _g24(), np.load(os.path.join(str(tmp_path), "g24_split_nuclei.npz"), allow_pickle=False)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- the host choice ----------------------------------------------------------------------------------------------
def test_choose_splits_on_hand_tables():
    from ark_analysis_amd.som_device import choose_splits
    keys, nuc_keys = [2, 5, 9, 11], [3, 4, 8]
    #        cell 2: nucleus 3, 20 inside of 36;  cell 5: nucleus 3, 12 of 36;  cell 9: nucleus 8, 4 of 40;  cell 11: none
    best, inside, area = [0, 0, 2, -1], [20, 12, 4, 0], [36, 9, 40]
    chosen, cv, nv, n = choose_splits(keys, nuc_keys, best, inside, area, [2, 5, 9, 11])
    assert chosen.dtype == np.int32 and cv.dtype == nv.dtype == np.int64
    assert n == 3 and cv.tolist() == [9, 10, 0, -1]          # cell 9's piece has 4 pixels: numbered (11), then dropped
    assert nv.tolist() == [0, 4, 8]                          # nucleus 3 keeps 36 - 20 - 12 = 4 pixels: dropped
    # the caller's order numbers the labels; a duplicate takes a new number and the last one wins
    chosen, cv, nv, n = choose_splits(keys, nuc_keys, best, inside, area, [5, 2, 5])
    assert n == 3 and cv.tolist() == [10, 11, -1, -1] and nv.tolist() == [0, 4, 8]
    # a subset: nucleus 3 keeps 36 - 12 = 24
    chosen, cv, nv, n = choose_splits(keys, nuc_keys, best, inside, area, [5])
    assert n == 1 and cv.tolist() == [-1, 9, -1, -1] and nv.tolist() == [3, 4, 8]
    # strict compare: 36 - 20 = 16 > 16 is false, 36 - 12 = 24 > 16
    _, cv, _, n = choose_splits(keys, nuc_keys, best, inside, area, [2, 5], min_size=16)
    assert n == 1 and cv.tolist() == [-1, 9, -1, -1]
    # small = 0 keeps everything; first_new moves the numbering
    _, cv, nv, _ = choose_splits(keys, nuc_keys, best, inside, area, [9], small=0, first_new=100)
    assert cv.tolist() == [-1, -1, 100, -1] and nv.tolist() == [3, 4, 8]
    # nothing named, nothing split; an unsplit nucleus below `small` is dropped all the same
    _, cv, nv, n = choose_splits(keys, nuc_keys, best, inside, [36, 4, 40], [])
    assert n == 0 and cv.tolist() == [-1] * 4 and nv.tolist() == [3, 0, 8]
    with pytest.raises(IndexError, match="cell id 7 "):
        choose_splits(keys, nuc_keys, best, inside, area, [2, 7])
    with pytest.raises(IndexError, match="cell id 12 "):
        choose_splits(keys, nuc_keys, best, inside, area, [12])
    with pytest.raises(TypeError):
        choose_splits(keys, nuc_keys, best, inside, area, [2.0])
    # the dtype bound: 8 + 2 = 10 fits, first_new 255 + 2 splits does not
    choose_splits(keys, nuc_keys, best, inside, area, [2, 5], dtype=np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        choose_splits(keys, nuc_keys, best, inside, area, [2, 5], first_new=255, dtype=np.uint8)
    choose_splits(keys, nuc_keys, best, inside, area, [2], first_new=255, dtype=np.uint8)      # 255 itself fits
    # empty tables
    chosen, cv, nv, n = choose_splits([], [], [], [], [], [])
    assert n == 0 and chosen.size == cv.size == nv.size == 0


def test_choice_through_the_numpy_stand_in_equals_the_loop(seg_utils):
    for name, cell, nuc, ids, min_size, want in split_cases():
        got = seg_utils.split_large_nuclei(cell, nuc, ids, min_size=min_size)
        assert got.dtype == want.dtype, name
        np.testing.assert_array_equal(got, want, err_msg=name)
    cell, nuc = snr.voronoi_case(96, 130, 40, 3)
    rng = np.random.default_rng(2)
    for kind in snr.ID_KINDS:
        ids = snr.ids_of(kind, cell, rng)
        np.testing.assert_array_equal(seg_utils.split_large_nuclei(cell, nuc, ids), snr.split_loop(cell, nuc, ids)[0])
    for i in range(0, snr.N_FUZZ, 7):
        c = snr.fuzz_case(i)
        np.testing.assert_array_equal(numpy_split_device(c["cell"], c["nuc"], c["cell_ids"], c["min_size"]),
                                      snr.split_loop(c["cell"], c["nuc"], c["cell_ids"], c["min_size"])[0])


def test_find_nuclear_label_id_and_concatenate_csv(tmp_path):
    import pandas as pd
    from ark_analysis_amd.segmentation import segmentation_utils as su
    nuc = np.array([[0, 7, 7, 3], [3, 3, 7, 0], [0, 0, 0, 0]])
    coords = np.argwhere(np.ones((2, 4), bool))
    assert su.find_nuclear_label_id(nuc, coords) == 3                     # 3 and 7 tie at 3 pixels: the smaller
    assert su.find_nuclear_label_id(nuc, np.array([[2, 0], [2, 1]])) is None
    assert su.find_nuclear_label_id(nuc, np.array([[0, 1], [0, 2], [0, 3]])) == 7
    for name, rows in (("a.csv", [1, 2]), ("b.csv", [3])):
        pd.DataFrame({"x": rows}).to_csv(os.path.join(str(tmp_path), name), index=False)
    su.concatenate_csv(str(tmp_path), ["a.csv", "b.csv"])
    got = pd.read_csv(os.path.join(str(tmp_path), "combined_data.csv"))
    assert got["x"].tolist() == [1, 2, 3] and got["fov"].tolist() == ["a", "a", "b"]
    su.concatenate_csv(str(tmp_path), ["a.csv", "b.csv"], column_name="run", column_values=["r1", "r2"])
    assert pd.read_csv(os.path.join(str(tmp_path), "combined_data.csv"))["run"].tolist() == ["r1", "r1", "r2"]
    with pytest.raises(ValueError, match="different lengths"):
        su.concatenate_csv(str(tmp_path), ["a.csv", "b.csv"], column_values=["r1"])


# ---- errors: all before the device entry is reached ---------------------------------------------------------------
def test_errors_come_before_any_launch(monkeypatch):
    from ark_analysis_amd.segmentation import segmentation_utils as su

    def never(*args, **kwargs):
        raise AssertionError("the device entry was reached")
    monkeypatch.setattr(su, "_split_device", never)
    cell, nuc, _ = snr.hand_plane()
    ids = np.arange(1, 12)
    with pytest.raises(IndexError, match="cell id 40 "):
        su.split_large_nuclei(cell, nuc, [1, 40, 2])
    with pytest.raises(IndexError, match="cell id 0 "):                       # the background is no cell
        su.split_large_nuclei(cell, nuc, [0])
    for bad in (cell.astype(np.int64) * -1, ):
        with pytest.raises(ValueError, match="negative"):
            su.split_large_nuclei(bad, nuc, ids)
        with pytest.raises(ValueError, match="negative"):
            su.split_large_nuclei(cell, np.where(nuc == 11, -11, nuc), ids)
    with pytest.raises(TypeError, match="integer"):
        su.split_large_nuclei(cell, nuc.astype(np.float32), ids)
    with pytest.raises(TypeError, match="integer"):
        su.split_large_nuclei(cell.astype(np.float64), nuc, ids)
    with pytest.raises(TypeError, match="integers"):
        su.split_large_nuclei(cell, nuc, ids.astype(np.float64))
    with pytest.raises(ValueError, match="2147483647"):
        su.split_large_nuclei(cell, np.where(nuc == 19, 2 ** 31, nuc.astype(np.int64)), ids)
    with pytest.raises(ValueError, match="2147483647"):
        su.split_large_nuclei(np.where(cell == 11, 2 ** 32 - 1, cell).astype(np.uint32), nuc, ids)
    with pytest.raises(ValueError, match="one shape"):
        su.split_large_nuclei(cell, nuc[:, :-1], ids)


def test_overflow_of_the_plane_dtype_is_an_error_naming_it(seg_utils):
    cell, nuc, _ = snr.hand_plane()
    ids = np.arange(1, 12)
    high = np.where(nuc == 19, 250, nuc).astype(np.uint8)          # 9 splits from 251 on: 259 does not fit uint8
    with pytest.raises(ValueError, match="uint8"):
        seg_utils.split_large_nuclei(cell, high, ids)
    got = seg_utils.split_large_nuclei(cell, high, ids[:6])        # cells 2 .. 6 split: 251 .. 255 fit
    assert got.dtype == np.uint8 and int(got.max()) == 255
    np.testing.assert_array_equal(got, snr.split_loop(cell, high, ids[:6])[0])
    with pytest.raises(ValueError, match="int16"):
        seg_utils.split_large_nuclei(cell, np.where(nuc == 19, 2 ** 15 - 3, nuc).astype(np.int16), ids)


# ---- generate_cell_table ------------------------------------------------------------------------------------------
@pytest.fixture
def mq(monkeypatch, seg_utils):
    install_host_stand_in(monkeypatch.setattr)
    from ark_analysis_amd.segmentation import marker_quantification
    return marker_quantification


def check_cell_table_fixture(tmp_path):
    """generate_cell_table(split_large_nuclei=True) against the reference's frames; also used on the device."""
    from ark_analysis_amd.segmentation import marker_quantification as mq
    fovs, channels, images, segs, args, want, uninit = _fixture_case(_g24(), 0)
    seg_dir, tiff_dir = write_cohort(os.path.join(str(tmp_path), "g24"), images, segs, channels)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        got = mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=True, split_large_nuclei=True, **args)
        plain = mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=True, **args)
    assert [str(w.message) for w in wl if "found in the following image" in str(w.message)] == []
    for frame, exp in zip(got, want):
        _compare_frames(frame, exp, False, uninit)
    assert not plain[0]["label_nuclear"].equals(got[0]["label_nuclear"])        # the flag changes the table
    assert int(got[0]["label_nuclear"].max()) > max(int(segs[f + "_nuclear.tiff"].max()) for f in fovs)
    return seg_dir, tiff_dir, segs, got


def test_generate_cell_table_host_logic_fixture(mq, tmp_path):
    check_cell_table_fixture(tmp_path)


def test_split_without_nuclear_counts_stays_refused(mq, tmp_path):
    fovs, channels, images, segs, args, _, _ = _fixture_case(_g24(), 0)
    seg_dir, tiff_dir = write_cohort(str(tmp_path), images, segs, channels)
    with pytest.raises(NotImplementedError, match="split_large_nuclei.*nuclear_counts=True"):
        mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=True, split_large_nuclei=True)
    with pytest.raises(NotImplementedError, match="split_large_nuclei.*nuclear_counts=True"):
        mq.generate_cell_table(seg_dir, tiff_dir, regionprops_base=["area"], split_large_nuclei=True)
    # split_large_nuclei=False is the table as before
    a = mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=True, nuclear_counts=True, split_large_nuclei=False)
    b = mq.generate_cell_table(seg_dir, tiff_dir, fast_extraction=True, nuclear_counts=True)
    assert a[0].equals(b[0]) and a[1].equals(b[1])


# ---- the planes of the GPU tests: something happens on every one of them ------------------------------------------
def _facts(cell, nuc, ids=None, **kw):
    if ids is None:
        ids = np.unique(cell)
        ids = ids[ids != 0]
    return snr.facts(cell, nuc, ids, **kw)


def test_hand_plane_puts_every_decision_on_its_edge():
    cell, nuc, notes = snr.hand_plane()
    assert cell.shape == (24, 70)
    ck, nk, best, inside, area = snr.pair_tables(cell, nuc)
    row = {int(c): (int(nk[b]) if b >= 0 else None, int(i), int(area[b] - i) if b >= 0 else None)
           for c, b, i in zip(ck, best, inside)}
    assert row[1] == (11, 20, 15) and row[2] == (12, 20, 16)              # outside == min_size, == min_size + 1
    assert row[3][0] == row[4][0] == row[5][0] == 13 and area[list(nk).index(13)] - 30 - 25 - 21 == 4    # remnant of 4
    assert row[6][0] == row[7][0] == 14 and area[list(nk).index(14)] - 20 - 16 == 5                     # remnant of 5
    assert row[8] == (15, 4, 30) and row[9] == (16, 5, 30)                # new pieces of 4 and of 5
    assert row[10] == (17, 10, 16)                                        # the tie: 17 (16 outside) wins over 18 (3 outside)
    assert int(((cell == 10) & (nuc == 18)).sum()) == 10 and int((nuc == 18).sum()) == 13
    assert row[11] == (None, 0, None)                                     # a cell without a nucleus
    assert int(((nuc == 19) & (cell != 0)).sum()) == 0 and int((nuc == 19).sum()) == 12   # a nucleus over background
    out, n = snr.split_loop(cell, nuc, ck)
    assert n == 9
    labels = set(np.unique(out).tolist())
    assert 11 in labels and int(out[cell == 1].max()) == 11               # cell 1 did not split
    assert 13 not in labels and 14 in labels and int((out == 14).sum()) == 5
    new = {int(c): int(out[(cell == c) & (nuc == row[int(c)][0])].max()) for c in (2, 3, 4, 5, 6, 7, 8, 9, 10)}
    assert new[2] == 20 and new[8] == 0 and new[9] == 27 and new[10] == 28
    assert int((out == 18).sum()) == 13 and int((out == 19).sum()) == 12
    # runs that cross the 64-pixel group and the row end
    flat = np.flatnonzero((nuc == 11).ravel() & (cell == 1).ravel())
    assert flat.min() // 64 != flat.max() // 64 and flat.min() // 70 == flat.max() // 70
    flat = np.flatnonzero((nuc == 12).ravel() & (cell == 2).ravel())
    assert flat.min() // 70 != flat.max() // 70 and flat.max() - flat.min() == 19
    f = _facts(cell, nuc)
    assert f["splits"] == 9 and f["dropped_remnants"] == 1 and f["dropped_new"] == 1 and f["shared_nuclei"] == 2


@pytest.mark.parametrize("h,w,n,seed,splits", [(96, 130, 40, 3, 8), (200, 257, 150, 5, 75)])
def test_voronoi_cases_have_what_they_claim(h, w, n, seed, splits):
    cell, nuc = snr.voronoi_case(h, w, n, seed)
    f = _facts(cell, nuc)
    assert f["splits"] == splits and f["dropped_remnants"] >= 1 and f["cells_without_nucleus"] >= 1
    assert f["shared_nuclei"] >= 1 and f["nuclei"] >= n * 0.9
    if h == 200:
        assert f["dropped_new"] >= 1


def test_field_size_case_has_what_it_claims():
    cell, nuc = snr.voronoi_case(1024, 1024, 20000, 1024)
    f = _facts(cell, nuc)
    assert f["cells"] > 17000 and f["splits"] > 500 and f["dropped_remnants"] >= 1 and f["dropped_new"] >= 1
    assert f["cells_without_nucleus"] >= 1 and f["shared_nuclei"] >= 1


def test_fuzz_generator_covers_every_class_and_every_case_splits():
    seen = {"size": set(), "pair": set(), "layout": set(), "min": set(), "ids": set(), "route": set()}
    for i in range(snr.N_FUZZ):
        c = snr.fuzz_case(i)
        cell, nuc = c["cell"], c["nuc"]
        for plane in (cell, nuc):                                         # the casts lost nothing
            assert plane.min() >= 0 and len(np.unique(plane)) > 5
        out, n = snr.split_vec(cell, nuc, c["cell_ids"], c["min_size"])
        assert n >= 1, i
        assert int(out.max()) <= np.iinfo(nuc.dtype).max and int(nuc.max()) + n <= np.iinfo(nuc.dtype).max, i
        if c["min_kind"] == "edge":                                       # one named cell exactly on the strict compare
            ck, _, best, inside, area = snr.pair_tables(cell, nuc)
            named = np.isin(ck, c["cell_ids"]) & (best >= 0)
            assert ((area[best[named]] - inside[named]) == c["min_size"]).any(), i
        seen["size"].add(cell.shape)
        seen["pair"].add((cell.dtype.name, nuc.dtype.name))
        seen["layout"].add(c["layout"])
        seen["min"].add(c["min_kind"])
        seen["ids"].add(c["id_kind"])
        seen["route"].add(c["force_search"])
    assert seen["size"] == set(snr.FUZZ_SIZES) and len(seen["pair"]) == 36
    assert seen["layout"] == set(snr.FUZZ_LAYOUTS) and seen["min"] == set(snr.FUZZ_MIN_SIZES)
    assert seen["ids"] == set(snr.ID_KINDS) and seen["route"] == {False, True}


# ---- the C entries refuse bad arguments before any HIP call (no GPU needed) ---------------------------------------
def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    p = 4096                                                  # any non-null address: nothing is dereferenced

    def overlaps(cd=3, ldc=70, nd=3, ldn=70, h=24, w=70, n_cells=2, cmin=1, cmax=2, n_nuc=1, area=p, best=p, capacity=10,
                 n=p, ws=p, wsb=1 << 20, flags=0, cell=p, keys=p):
        return lib.pxsom_nuclear_overlaps(cell, cd, ldc, p, nd, ldn, h, w, keys, n_cells, cmin, cmax, p, n_nuc, 7, 7, area,
                                          best, capacity, n, ws, wsb, flags, None)
    for bad, word in ((dict(cd=6), b"dtypes"), (dict(nd=8), b"dtypes"), (dict(ldc=69), b"stride"), (dict(h=0), b"size"),
                      (dict(h=50000, w=50000, ldc=50000, ldn=50000), b"2147483647"), (dict(flags=2), b"flags"),
                      (dict(n_cells=-1), b"key counts"), (dict(cmin=3), b"key_min"), (dict(keys=None), b"null key table"),
                      (dict(cell=None), b"null plane"), (dict(n=None), b"n_dev"), (dict(best=None), b"go together"),
                      (dict(capacity=0), b"capacity"), (dict(capacity=(1 << 27) + 1), b"134217728"),
                      (dict(ws=None), b"workspace"), (dict(wsb=16), b"workspace")):
        assert overlaps(**bad) == -1, bad
        assert word in lib.pxsom_last_error(), (bad, lib.pxsom_last_error())
    assert lib.pxsom_nuclear_overlaps_workspace_bytes(0, 2, 1, 2, 1, 7, 7, 0) == 0
    assert lib.pxsom_nuclear_overlaps_workspace_bytes(10, -1, 1, 2, 1, 7, 7, 0) == 0
    # 64 slots of 12 bytes, one word per cell, two LUTs of 2 and 1 entries: each part rounded up to 256 bytes
    assert lib.pxsom_nuclear_overlaps_workspace_bytes(10, 2, 1, 2, 1, 7, 7, 0) == 256 + 256 + 256 + 512 + 256
    assert lib.pxsom_nuclear_overlaps_workspace_bytes(10, 2, 1, 2, 1, 7, 7, 1) == 256 + 512 + 256
    assert lib.pxsom_split_apply_workspace_bytes(2, 1, 2, 1, 7, 7, 0) == 512
    assert lib.pxsom_split_apply_workspace_bytes(2, 1, 2, 1, 7, 7, 1) == 0

    def apply(cd=0, ldc=70, h=24, ldo=70, out=p, chosen=p, ws=p, wsb=4096, flags=0):
        return lib.pxsom_split_apply(p, cd, ldc, p, 5, 70, h, 70, p, 2, 1, 2, p, 1, 7, 7, chosen, p, p, out, ldo, ws, wsb,
                                     flags, None)
    for bad, word in ((dict(cd=-1), b"dtypes"), (dict(ldc=1), b"stride"), (dict(h=-4), b"size"), (dict(ldo=69), b"output stride"),
                      (dict(out=None), b"null output"), (dict(chosen=None), b"null output or table"), (dict(flags=8), b"flags"),
                      (dict(ws=None), b"workspace"), (dict(wsb=511), b"workspace")):
        assert apply(**bad) == -1, bad
        assert word in lib.pxsom_last_error(), (bad, lib.pxsom_last_error())
