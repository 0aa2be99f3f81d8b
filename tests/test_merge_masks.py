"""Merging object masks into cell masks (K18) without a GPU: the numpy + scipy statement of tests/merge_masks_reference.py
against the g22 fixtures (made by the reference's own merge_masks_single) and against hand-built cases, one quirk each;
the Python mirrors with their device entries swapped for that statement -- signatures, files, dtypes, log, printed
line; the ABI."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ark_analysis_amd.segmentation.ez_seg import merge_masks as mirror  # noqa: F401  (the feature under test)
from tests import merge_masks_reference as mmr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
GE = (lambda x, y: x >= y)
GT = (lambda x, y: x > y)


@pytest.fixture(scope="module")
def g22():
    return np.load(os.path.join(GOLDEN, "g22_merge_masks.npz"))


@pytest.fixture
def statement_backend(monkeypatch):
    """The mirror with its three device entries swapped for the statement on host arrays."""
    from ark_analysis_amd.segmentation.ez_seg import merge_masks as mm
    monkeypatch.setattr(mm, "_to_device", lambda mask: mask)
    monkeypatch.setattr(mm, "_to_host", lambda plane: plane)
    monkeypatch.setattr(mm, "_merge_device", mmr.merge_masks)
    return mm


# ---- the statement against the fixtures and the reference's own case ------------------------------------------------------
def test_statement_equals_the_fixtures(g22):
    cases = json.loads(str(g22["cases"]))
    assert len(cases) == 4
    for c in cases:
        name = c["name"]
        merged, remaining = mmr.merge_masks(g22["objects_" + name], g22["cells_" + name], c["overlap_thresh"],
                                            c["expansion_factor"])
        assert g22["objects_" + name].shape == (96, 96)
        assert merged.dtype == np.int32 and np.array_equal(merged, g22["merged_" + name]), name
        assert remaining.dtype == np.int32 and np.array_equal(remaining, g22["remaining_" + name]), name
        cells = mmr.label_regions(g22["cells_" + name], 2)[0]
        assert 0 < len(np.unique(remaining)) < len(np.unique(cells)), name          # some cells merged, some stayed


def two_disc_case():
    shape = (32, 32)
    objects, cells = np.zeros(shape), np.zeros(shape)                 # float64 planes, as the reference's test passes
    objects[mmr.disc(shape, (7, 7), 25)] = 1
    cells[mmr.disc(shape, (1, 1), 25)] = 1
    cells[mmr.disc(shape, (13, 13), 25)] = 2
    objects[mmr.disc(shape, (25, 25), 25)] = 2
    cells[mmr.disc(shape, (20, 20), 25)] = 3
    cells[mmr.disc(shape, (27, 27), 25)] = 4
    want_merged = objects.copy()
    want_merged[mmr.disc(shape, (27, 27), 25)] = 2
    want_cells = np.where(cells == 4, 0, cells)
    return objects, cells, want_merged, want_cells


def test_statement_on_the_two_disc_case():
    objects, cells, want_merged, want_cells = two_disc_case()
    merged, remaining = mmr.merge_masks(objects, cells, 10, 10)
    assert np.array_equal(merged, want_merged) and np.array_equal(remaining, want_cells)
    # below the threshold: no merge; of two cells over it only the larger overlap
    pairs = {(a, b): c for a, b, c in mmr.pair_overlaps(objects.astype(np.int32), cells.astype(np.int32))}
    area = int((cells == 1).sum())
    assert 0 < pairs[1, 1] / area <= 0.10 and 0 < pairs[1, 2] / area <= 0.10
    assert pairs[2, 4] > pairs[2, 3] > 0.10 * area


@pytest.mark.parametrize("h,w,n_cells,n_objects", [(40, 57, 30, 6), (1, 90, 10, 3), (130, 65, 140, 20), (7, 3, 5, 2)])
def test_windowed_discs_equal_whole_image_discs(h, w, n_cells, n_objects):
    """random_masks_windowed (the field-size GPU tests) paints what random_masks paints, from the same draws: discs cut
    by every border, discs wider than the image, and the generator left in the same state."""
    for radii in (dict(), dict(cell_r=(6, 14), object_r=(10, 30))):
        rs_whole, rs_window = np.random.RandomState(h + w), np.random.RandomState(h + w)
        whole = mmr.random_masks(rs_whole, h, w, n_cells, n_objects, **radii)
        window = mmr.random_masks_windowed(rs_window, h, w, n_cells, n_objects, **radii)
        assert np.array_equal(whole[0], window[0]) and np.array_equal(whole[1], window[1])
        assert whole[0].dtype == window[0].dtype and whole[1].dtype == window[1].dtype
        assert rs_whole.randint(1 << 30) == rs_window.randint(1 << 30)


# ---- hand-built cases, one quirk each ---------------------------------------------------------------------------------------
def quirks():
    """name -> (object mask, cell mask, overlap_thresh, expansion_factor); used by the GPU test too."""
    out = {}
    z = lambda h=8, w=12: np.zeros((h, w), dtype=np.int32)          # noqa: E731
    objects, cells = z(), z()
    cells[2:6, 0:5], cells[2:6, 5:10] = 7, 3                         # touching cells of different value
    objects[3:5, 3:9] = 1                                            # 4 pixels of the left cell, 8 of the right
    out["touching"] = (objects, cells, 10, 20)
    objects, cells = z(), z()
    cells[1:4, 1:4], cells[5:8, 7:10] = 5, 5                         # one value in two pieces
    objects[2:4, 2:6] = 4
    out["pieces"] = (objects, cells, 10, 20)
    objects, cells = z(), z()
    cells[2:4, 1:4], cells[2:4, 6:9] = 2, 1                          # equal overlaps: the raster-first cell keeps it
    objects[3, 2:8] = 1
    out["tie"] = (objects, cells, 10, 20)
    objects, cells = z(), z()
    cells[2:4, 2:4] = 1                                              # area 4, overlap 2: exactly 50 percent
    objects[1:3, 2:4] = 1
    out["threshold"] = (objects, cells, 50, 20)
    for name, last in (("edge_in", 8), ("edge_out", 10)):            # object box cols 2 .. 2 grown by 3: up to col 5
        objects, cells = z(8, 14), z(8, 14)
        objects[5, 2] = 1
        cells[5, 2:last + 1] = 1                                     # centroid col 5 (on the edge) or 6 (one outside)
        out[name] = (objects, cells, 5, 3)
    objects, cells = z(), z()
    cells[3:5, 4:8] = 1
    objects[3:5, 2:6], objects[3:5, 6:10] = 1, 2                     # both objects take the cell: the larger label stays,
    out["shared"] = (objects, cells, 10, 20)                         # and it paints over object 1's pixels
    objects, cells = z(), z()
    cells[1:3, 1:9] = 1                                              # 16 pixels: 2 in object 1 (12.5 %), 6 in object 2
    objects[0:3, 1] = 1
    objects[1:3, 6:9] = 2
    out["overwrite"] = (objects, cells, 20, 20)
    return out


def test_hand_built_cases():
    q = quirks()
    merged, remaining = mmr.merge_masks(*q["touching"])
    assert np.array_equal(np.unique(remaining), [0, 1]) and (merged[2:6, 5:10] == 1).all() and merged[2, 0] == 0
    merged, remaining = mmr.merge_masks(*q["pieces"])
    assert (merged[1:4, 1:4] == 1).all() and not merged[5:8, 7:10].any() and (remaining[5:8, 7:10] == 2).all()
    assert not remaining[1:4, 1:4].any()
    merged, remaining = mmr.merge_masks(*q["tie"])
    assert (merged[2:4, 1:4] == 1).all() and merged[2, 6] == 0 and np.array_equal(np.unique(remaining), [0, 2])
    tied = mmr.merge_masks(*q["tie"], compare=(GE, GT))
    assert np.array_equal(np.unique(tied[1]), [0, 1])                # >= would hand the tie to the later cell
    merged, remaining = mmr.merge_masks(*q["threshold"])
    assert (remaining[2:4, 2:4] == 1).all() and merged[3, 2] == 0
    loose = mmr.merge_masks(*q["threshold"], compare=(GT, GE))
    assert not loose[1].any() and loose[0][3, 2] == 1                # >= would merge at exactly the threshold
    merged, remaining = mmr.merge_masks(*q["edge_in"])
    assert not remaining.any() and (merged[5, 2:9] == 1).all()
    merged, remaining = mmr.merge_masks(*q["edge_out"])
    assert (remaining[5, 2:11] == 1).all() and merged[5, 3] == 0
    merged, remaining = mmr.merge_masks(*q["shared"])
    assert not remaining.any() and (merged[3:5, 4:8] == 2).all() and (merged[3:5, 2:4] == 1).all()
    merged, remaining = mmr.merge_masks(*q["overwrite"])
    assert not remaining.any() and (merged[1:3, 1:9] == 2).all() and merged[0, 1] == 1
    with pytest.raises(ValueError, match="Both masks must have the same shape"):
        mmr.merge_masks(np.zeros((4, 5), np.int32), np.zeros((5, 4), np.int32), 10, 0)


def test_choice_on_the_host_equals_the_statement(g22):
    """som_device.choose_merges (the host half of the device chain) fed from the statement's tables."""
    from ark_analysis_amd import som_device
    sets = [(g22["objects_" + c["name"]], g22["cells_" + c["name"]], c["overlap_thresh"], c["expansion_factor"])
            for c in json.loads(str(g22["cases"]))] + list(quirks().values())
    for objects, cells, thresh, grow in sets:
        ol, n_o, _ = mmr.label_regions(objects, 2)
        cl, n_c, areas = mmr.label_regions(cells, 2)
        _, _, boxes = mmr.region_tables(ol, n_o)
        count, sums, _ = mmr.region_tables(cl, n_c)
        winner, removed = som_device.choose_merges(mmr.pair_overlaps(ol, cl), boxes.astype(np.int32), count, sums, thresh, grow)
        merged = np.where(winner[cl] != 0, winner[cl], ol)
        remaining = np.where(removed[cl] != 0, 0, cl)
        want = mmr.merge_masks(objects, cells, thresh, grow)
        assert np.array_equal(merged, want[0]) and np.array_equal(remaining, want[1])


# ---- the mirrors ------------------------------------------------------------------------------------------------------------
def test_signatures_equal_the_reference(g22):
    recorded = json.loads(str(g22["signatures"]))
    assert set(recorded) == {"merge_masks_seq", "merge_masks_single", "get_bounding_boxes", "filter_labels_in_bbox"}
    for name, params in recorded.items():
        got = [[p.name, repr(p.default)] for p in inspect.signature(getattr(mirror, name)).parameters.values()]
        assert got == params, name


def test_merge_masks_single_files_and_dtypes(statement_backend, tmp_path, g22):
    from ark_analysis_amd import image_io
    mm = statement_backend
    objects, cells, want_merged, want_cells = two_disc_case()
    remaining = mm.merge_masks_single(objects, cells, 10, "merged_mask", str(tmp_path), 10)
    merged = image_io.read_image(str(tmp_path / "merged_mask_merged.tiff"))
    assert merged.dtype == np.int32 and np.array_equal(merged, want_merged)
    assert remaining.dtype == np.int32 and np.array_equal(remaining, want_cells)
    # the relabelled numbers are returned, not the input's values; ".tiff" leaves the name
    objects, cells, thresh, grow = quirks()["pieces"]
    remaining = mm.merge_masks_single(objects.astype(np.uint16), cells.astype(np.int64), thresh, "fov0_obj.tiff", str(tmp_path), grow)
    assert np.array_equal(np.unique(remaining), [0, 2]) and os.path.exists(tmp_path / "fov0_obj_merged.tiff")
    for c in json.loads(str(g22["cases"])):
        name = c["name"]
        remaining = mm.merge_masks_single(g22["objects_" + name], g22["cells_" + name], c["overlap_thresh"], name + ".tiff",
                                          str(tmp_path), c["expansion_factor"])
        assert np.array_equal(remaining, g22["remaining_" + name]), name
        assert np.array_equal(image_io.read_image(str(tmp_path / (name + "_merged.tiff"))), g22["merged_" + name]), name
    with pytest.raises(ValueError, match="Both masks must have the same shape"):
        mm.merge_masks_single(np.zeros((4, 5)), np.zeros((5, 4)), 10, "x", str(tmp_path), 0)
    with pytest.raises(ValueError, match="float64"):
        mm.merge_masks_single(np.full((4, 4), 0.5), np.zeros((4, 4)), 10, "x", str(tmp_path), 0)
    with pytest.raises(ValueError, match="float32"):
        mm.merge_masks_single(np.zeros((4, 4)), np.full((4, 4), 3e9, dtype=np.float32), 10, "x", str(tmp_path), 0)
    with pytest.raises(ValueError, match="complex128"):
        mm.merge_masks_single(np.zeros((4, 4), complex), np.zeros((4, 4)), 10, "x", str(tmp_path), 0)


def run_merge_masks_seq(mm, tmp_path, capsys):
    """merge_masks_seq on two FOVs and two object types at 64 x 80 against the statement chained on the host (used by
    the GPU test too)."""
    from ark_analysis_amd import image_io
    rs = np.random.RandomState(18)
    dirs = {k: tmp_path / k for k in ("ez_seg_dir", "deepcell_output", "merged_masks_dir", "log_dir")}
    for d in dirs.values():
        d.mkdir()
    fovs, kinds, masks = ["fov1", "fov0"], ["plaques", "vessels"], {}
    for fov in fovs:
        objects, cells = mmr.random_masks(rs, 64, 80, 70, 9)
        masks[fov] = cells.astype(np.uint16)
        image_io.write_image(str(dirs["deepcell_output"] / (fov + "_whole_cell.tiff")), masks[fov])
        for kind in kinds:
            masks[fov, kind] = objects if kind == "plaques" else mmr.random_masks(rs, 64, 80, 1, 6)[0]
            image_io.write_image(str(dirs["ez_seg_dir"] / ("%s_%s.tiff" % (fov, kind))), masks[fov, kind])
    capsys.readouterr()
    mm.merge_masks_seq(fovs, kinds, str(dirs["ez_seg_dir"]), str(dirs["deepcell_output"]), "whole_cell", 15, 4,
                       str(dirs["merged_masks_dir"]), str(dirs["log_dir"]))
    out = capsys.readouterr().out
    assert out.endswith("Merged masks built and saved\n") and "Values saved to " in out
    assert sorted(os.listdir(dirs["merged_masks_dir"])) == sorted(
        ["%s_%s_merged.tiff" % (f, k) for f in fovs for k in kinds] + [f + "_final_whole_cell_remaining.tiff" for f in fovs])
    for fov in fovs:
        cells, taken = masks[fov], 0
        for kind in kinds:
            merged, cells_next = mmr.merge_masks(masks[fov, kind], cells, 15, 4)
            taken += len(np.unique(mmr.label_regions(cells, 2)[0])) - len(np.unique(cells_next))
            cells = cells_next
            got = image_io.read_image(str(dirs["merged_masks_dir"] / ("%s_%s_merged.tiff" % (fov, kind))))
            assert got.dtype == np.int32 and np.array_equal(got, merged), (fov, kind)
        got = image_io.read_image(str(dirs["merged_masks_dir"] / (fov + "_final_whole_cell_remaining.tiff")))
        assert got.dtype == np.int32 and np.array_equal(got, cells) and cells.any() and taken > 0, fov
    log = (dirs["log_dir"] / "mask_merge_log.txt").read_text().splitlines()
    assert log == ["fov_list: ['fov1', 'fov0']", "object_list: ['plaques', 'vessels']",
                   "object_mask_dir: " + str(dirs["ez_seg_dir"]), "cell_mask_dir: " + str(dirs["deepcell_output"]),
                   "cell_mask_suffix: whole_cell", "overlap_percent_threshold: 15",
                   "save_path: " + str(dirs["merged_masks_dir"])]


def test_merge_masks_seq_files_and_log(statement_backend, tmp_path, capsys):
    run_merge_masks_seq(statement_backend, tmp_path, capsys)


def test_bounding_boxes_and_filter():
    labels = np.array([[1, 1, 0, 0],
                       [0, 1, 0, 0],
                       [0, 0, 2, 2]])
    boxes = mirror.get_bounding_boxes(labels)
    assert boxes == {1: ((0, 0), (1, 1)), 2: ((2, 2), (2, 3))}
    props = {"label": np.array([1, 2]), "centroid-0": np.array([1 / 3, 2.0]), "centroid-1": np.array([2 / 3, 2.5])}
    assert mirror.filter_labels_in_bbox(boxes[1], props, 0) == [1]
    assert mirror.filter_labels_in_bbox(boxes[2], props, 0) == [2]
    assert mirror.filter_labels_in_bbox(((0, 0), (0, 0)), props, 0) == []
    assert mirror.filter_labels_in_bbox(boxes[1], props, expansion_factor=10) == [1, 2]
    assert mirror.filter_labels_in_bbox(((0, 0), (1, 1)), props, 1) == [1]          # 2.0 <= 1 + 1 but 2.5 > 1 + 1


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols():
    from ark_analysis_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pxsom.h")).read()
    assert _capi.ABI_VERSION == 9 and re.search(r"#define PXSOM_ABI_VERSION 9\b", header)
    for name in ("pxsom_label_regions_workspace_bytes", "pxsom_label_regions", "pxsom_pair_overlaps_workspace_bytes",
                 "pxsom_pair_overlaps", "pxsom_merge_apply"):
        assert name in _capi.SYMBOLS and re.search(r"\b%s\(" % name, header), name
    lib = _capi.lib()       # resolves every symbol; no device needed for the host-side checks below
    assert lib.pxsom_abi_version() == 9
    assert lib.pxsom_label_regions_workspace_bytes(130, 195) == lib.pxsom_label_components_workspace_bytes(130, 195)
    assert lib.pxsom_label_regions_workspace_bytes(0, 5) == 0
    assert lib.pxsom_pair_overlaps_workspace_bytes(1000) >= 2 * 1000 * 12
    assert lib.pxsom_label_regions(None, 3, 4, 4, 4, 1, None, 4, None, None, 17, None, 0, None) == -1
    assert lib.pxsom_pair_overlaps(None, 4, None, 4, 4, 4, 1, 1, None, 0, None, None, 0, None) == -1
    assert lib.pxsom_merge_apply(None, 4, None, 4, 4, 4, None, None, 2, None, 4, None, 4, None) == -1


# ---- the generator reproduces the committed fixture -------------------------------------------------------------------------
def test_generator_reproduces_the_fixture(tmp_path):
    if not os.path.isdir("/root/reference/src/ark"):
        pytest.skip("the reference tree is not on this machine")
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_merge_masks.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / "g22_merge_masks.npz"), np.load(os.path.join(GOLDEN, "g22_merge_masks.npz"))
    assert sorted(new.files) == sorted(old.files)
    for key in old.files:
        assert np.array_equal(new[key], old[key]), key
    assert os.path.getsize(os.path.join(GOLDEN, "g22_merge_masks.npz")) <= 100 * 1024
