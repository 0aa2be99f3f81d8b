"""The marker watershed of fibre segmentation (K28) without a GPU: the two forms of the statement in
tests/watershed_reference.py against each other and against the g31 fixture, the recalled switches, the generator,
watershed_labels, segment_fiber_channel and run_fiber_channel_segmentation with their device entries swapped for the
statement (files, columns, the empty cohort, the refusals, debug off and on), and the ABI: symbols, the header's K28 section,
the C entry's refusals on host pointers."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from ark_analysis_amd import image_io
from ark_analysis_amd.segmentation import fiber_segmentation as fs
from tests import clahe_reference as cr
from tests import fiber_reference as fr
from tests import watershed_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = "g31_watershed.npz"


@pytest.fixture(scope="module")
def g31():
    return np.load(os.path.join(GOLDEN, FIXTURE))


@pytest.fixture(scope="module")
def g30():
    return np.load(os.path.join(GOLDEN, "g30_clahe.npz"))


# ---- the two forms ------------------------------------------------------------------------------------------------------------
def test_the_round_form_equals_the_heap_form_on_random_planes():
    rs = np.random.RandomState(28)
    descents = most_rounds = 0
    for _ in range(3000):
        image, markers = wr.random_case(rs)
        stats = {}
        assert np.array_equal(wr.watershed_rounds(image, markers, shuffle=rs, stats=stats), wr.watershed(image, markers))
        descents += stats["descents"]
        most_rounds = max(most_rounds, stats["rounds"])
        assert stats["labelled"] == (int((markers == 0).sum()) if markers.any() else 0)
    assert descents > 1000 and most_rounds >= 8             # the basin path and several rounds per plane are exercised


def test_both_forms_equal_the_fixture(g31, g30):
    hand = wr.hand_cases()
    assert list(hand) == json.loads(str(g31["hand_names"]))
    for name, (image, markers) in hand.items():
        stats = {}
        assert np.array_equal(wr.watershed(image, markers), g31["labels_" + name]), name
        assert np.array_equal(wr.watershed_rounds(image, markers, stats=stats), g31["labels_" + name]), name
        assert (stats["descents"] > 0) == (name in wr.BASIN_CASES), name
    g28 = np.load(os.path.join(GOLDEN, "g28_fiber_markers.npz"))
    for name in wr.G28_NAMES:
        image, markers = g28["elevation_" + name], g28["markers_" + name]
        stats = {}
        assert np.array_equal(wr.watershed(image, markers), g31["g28_" + name]), name
        assert np.array_equal(wr.watershed_rounds(image, markers, stats=stats), g31["g28_" + name]), name
        assert stats["descents"] == 0 and stats["rounds"] <= 12 and set(np.unique(g31["g28_" + name])) <= {1, 2}, (name, stats)
    assert np.array_equal(wr.watershed(g30["chain_elevation"], g30["chain_markers"]), g31["chain_flooded"])
    assert np.array_equal(wr.filtered_labels(g30["chain_elevation"], g30["chain_markers"], int(g31["chain_min_fiber_size"])),
                          g31["chain_labels"])
    assert g31["chain_labels"].any() and int(g31["chain_largest"]) == np.bincount(g31["chain_labels"].ravel())[1:].max()


def test_what_the_hand_made_planes_show(g31):
    # a tie goes to the marker that is earlier in raster order, whichever label it carries
    assert (g31["labels_flat_two_labels"][:, 4] == 1).all() and (g31["labels_flat_two_labels_swapped"][:, 4] == 2).all()
    # the basin belongs to the label that reaches it first, whole
    for name, first in (("basin_two_labels", 1), ("basin_two_labels_swapped", 2)):
        assert (g31["labels_" + name][2:5, 3:6] == first).all(), name
    # the rim pixel between: through the basin when its parent pops first, directly otherwise -- label 1 both times
    assert g31["labels_rim_basin_first"][2, 4] == 1 and g31["labels_rim_direct_first"][2, 2] == 1
    assert (g31["labels_ring_basin"] == 5).all() and (g31["labels_basin_in_basin"] == 7).all()
    assert set(np.unique(g31["labels_marker_values"])) == {-2 ** 31, -3, 2 ** 31 - 1}
    image, markers = wr.serpentine()
    stats = {}
    assert (wr.watershed_rounds(image, markers, stats=stats) == 1).all() and stats["rounds"] > 2000
    assert not wr.watershed(np.arange(6).reshape(2, 3), np.zeros((2, 3))).any()              # no marker: all zeros


def test_generator_reproduces_the_fixture(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_watershed.py")], check=True, env=env, stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / FIXTURE), np.load(os.path.join(GOLDEN, FIXTURE))
    assert sorted(new.files) == sorted(old.files)
    for key in old.files:
        assert new[key].dtype == old[key].dtype and np.array_equal(new[key], old[key]), key
    assert os.path.getsize(os.path.join(GOLDEN, FIXTURE)) <= 211804 // 4                     # well under g28's size


def test_the_recalled_switches():
    assert set(fs.RECALLED_WATERSHED) == set(fs.WATERSHED_CHOICES) == {"marker_ties", "neighbours"}
    assert all(fs.RECALLED_WATERSHED[k] == v[0] for k, v in fs.WATERSHED_CHOICES.items())
    image, markers = wr.hand_cases()["flat_two_labels"]
    default, reverse = wr.watershed(image, markers), wr.watershed(image, markers, {"marker_ties": "reverse"})
    assert (default[:, 4] == 1).all() and (reverse[:, 4] == 2).all()          # the tie column changes hands
    # The neighbour order is recorded because the statement has to choose one, but under a (value, age) key it can change no
    # label: what one pop pushes carries one label and stays together in every queue.  Shown here on planes with ties,
    # basins and several levels, where any dependence would surface.
    rs = np.random.RandomState(5)
    planes = list(wr.hand_cases().values()) + [wr.random_case(rs) for _ in range(500)]
    for image, markers in planes:
        assert np.array_equal(wr.watershed(image, markers, {"neighbours": "+W,+1,-1,-W"}), wr.watershed(image, markers))
    with pytest.raises(ValueError, match="RECALLED_WATERSHED"):
        wr.watershed(image, markers, {"neighbours": "diagonal"})
    with pytest.raises(ValueError, match="RECALLED_WATERSHED"):
        wr.watershed(image, markers, {"marker_order": "raster"})
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "K28" in design and "RECALLED_WATERSHED" in design


# ---- the host entries over swapped hooks ---------------------------------------------------------------------------------------
def channel_fiber_labels_statement(channel, blur, kernel_size, sigmas, ridge_cutoff, sobel_blur, thresholds, min_fiber_size, planes):
    """The statement with the signature of fiber_segmentation._channel_fiber_labels_device."""
    contrast, ridges, dist, t, markers, elevation = cr.channel_watershed_inputs_device(channel, blur, kernel_size, sigmas,
                                                                                       ridge_cutoff, sobel_blur, thresholds)
    labels = wr.filtered_labels(elevation, markers, min_fiber_size)
    if not planes:
        return labels, None, None, None, t, None, None
    return labels, contrast, ridges, dist, t, markers, elevation


@pytest.fixture
def host(monkeypatch):
    fr.install_stand_ins(monkeypatch.setattr)
    monkeypatch.setattr(fs, "_watershed_device", wr.watershed)
    monkeypatch.setattr(fs, "_channel_fiber_labels_device", channel_fiber_labels_statement)


def chain_arguments(g30, g31):
    channel = cr.chain_channel()
    return channel, dict(blur=float(g30["chain_blur"]), contrast_scaling_divisor=channel.shape[0] / int(g30["chain_k"]),
                         ridge_cutoff=float(g30["cutoff"]), sobel_blur=float(g30["sobel_blur"]),
                         min_fiber_size=int(g31["chain_min_fiber_size"]))


def test_watershed_labels(host, g30, g31):
    got = fs.watershed_labels(g30["chain_elevation"].astype(np.float64), g30["chain_markers"].astype(np.int64))
    assert got.dtype == np.int32 and np.array_equal(got, g31["chain_flooded"])
    seen = {}

    def entry(elevation, markers):
        seen.update(dtypes=(elevation.dtype, markers.dtype), shapes=(elevation.shape, markers.shape))
        return np.zeros(elevation.shape, np.int64)
    monkey = pytest.MonkeyPatch()
    monkey.setattr(fs, "_watershed_device", entry)
    try:
        assert fs.watershed_labels(np.ones((3, 4)) * 2.75, np.ones((3, 4), bool)).dtype == np.int32      # astype, as the reference
    finally:
        monkey.undo()
    assert seen == {"dtypes": (np.int32, np.int32), "shapes": ((3, 4), (3, 4))}
    e, m = np.zeros((3, 4), np.int32), np.zeros((3, 4), np.int32)
    for bad_e, bad_m in ((e[0], m[0]), (e, m[:2]), (e[:0], m[:0]), (e[None], m[None]), (e.astype(object), m),
                         (e + np.nan, m), (e, m + np.inf), (e + 2.0 ** 31, m), (e, m - 2.0 ** 31 - 1)):
        with pytest.raises(ValueError):
            fs.watershed_labels(bad_e, bad_m)


def test_segment_fiber_channel(host, g30, g31, tmp_path):
    channel, kw = chain_arguments(g30, g31)
    quiet = tmp_path / "quiet"
    quiet.mkdir()
    table = fs.segment_fiber_channel(channel, "fov3", str(quiet), **kw)
    assert sorted(os.listdir(quiet)) == ["fiber_object_table.csv", "fov3_fiber_labels.tiff"]           # debug off: no _debug
    labels = image_io.read_image(str(quiet / "fov3_fiber_labels.tiff"))
    assert labels.dtype == np.int32 and np.array_equal(labels, g31["chain_labels"])
    columns = ["fov", "label", "centroid-0", "centroid-1", "major_axis_length", "minor_axis_length", "orientation", "area",
               "eccentricity", "euler_number"]
    assert list(table.columns) == columns and table["fov"].tolist() == ["fov3"] * len(table)
    assert table["label"].tolist() == np.unique(labels[labels != 0]).tolist()
    assert table["area"].tolist() == np.bincount(labels.ravel())[table["label"]].tolist()
    saved = pd.read_csv(quiet / "fiber_object_table.csv")
    assert list(saved.columns) == ["Unnamed: 0"] + columns                                             # written with the index
    loud = tmp_path / "loud"
    loud.mkdir()
    again = fs.segment_fiber_channel(channel.astype(np.float32), "fov3", str(loud), save_csv=False, debug=True, **kw)
    pd.testing.assert_frame_equal(again, table)
    assert sorted(os.listdir(loud)) == ["_debug", "fov3_fiber_labels.tiff"]
    debug = {name: image_io.read_image(str(loud / "_debug" / name)) for name in sorted(os.listdir(loud / "_debug"))}
    assert list(debug) == ["fov3_contrast_adjusted.tiff", "fov3_frangi_filter.tiff", "fov3_ridges_thresholded.tiff",
                           "fov3_thresholded.tiff"]
    assert all(p.dtype == np.float32 and p.shape == channel.shape for p in debug.values())
    assert np.array_equal(debug["fov3_thresholded.tiff"], g30["chain_markers"].astype(np.float32))
    assert np.array_equal(debug["fov3_ridges_thresholded.tiff"], g30["chain_dist"].astype(np.float32))
    assert np.array_equal(debug["fov3_frangi_filter.tiff"], g30["chain_ridges"].astype(np.float32))
    assert np.array_equal(debug["fov3_contrast_adjusted.tiff"], g30["chain_contrast"].astype(np.float32))
    # a subset of the properties, and no fibre at all
    few = fs.segment_fiber_channel(channel, "fov3", str(loud), object_properties=("label", "area"), save_csv=False,
                                   **dict(kw, min_fiber_size=int(g31["chain_largest"]) + 1))
    assert list(few.columns) == ["fov", "label", "area"] and len(few) == 0
    assert not image_io.read_image(str(loud / "fov3_fiber_labels.tiff")).any()


def test_segment_fiber_channel_refuses_before_the_device(monkeypatch, g30, g31, tmp_path):
    def never(*args, **kwargs):
        raise AssertionError("the device entry was reached")
    monkeypatch.setattr(fs, "_channel_fiber_labels_device", never)
    channel, kw = chain_arguments(g30, g31)
    out = str(tmp_path)
    with pytest.raises(FileNotFoundError):
        fs.segment_fiber_channel(channel, "fov3", str(tmp_path / "missing"), **kw)
    with pytest.raises(NotImplementedError, match="object_properties"):
        fs.segment_fiber_channel(channel, "fov3", out, object_properties=("label", "perimeter"), **kw)
    for bad in (channel[0], channel[:0], np.zeros((4, 4)), channel * np.nan, -channel):
        with pytest.raises(ValueError):
            fs.segment_fiber_channel(bad, "fov3", out, **kw)
    for changes, error in ((dict(contrast_scaling_divisor=0), ValueError), (dict(contrast_scaling_divisor=64), ValueError),
                           (dict(contrast_scaling_divisor=0.5), NotImplementedError), (dict(blur=-1), ValueError),
                           (dict(blur=17), NotImplementedError), (dict(sobel_blur=17), NotImplementedError),
                           (dict(fiber_widths=[]), ValueError), (dict(fiber_widths=[-1]), ValueError),
                           (dict(fiber_widths=[100]), NotImplementedError)):
        with pytest.raises(error):
            fs.segment_fiber_channel(channel, "fov3", out, **dict(kw, **changes))
    assert os.listdir(out) == []


def cohort(tmp_path, channel, fovs, sub=""):
    data, out = tmp_path / "data", tmp_path / "out"
    for fov in fovs:
        (data / fov / sub).mkdir(parents=True)
        image_io.write_image(str(data / fov / sub / "Collagen1.tiff"), channel.astype(np.float32))
        image_io.write_image(str(data / fov / sub / "Collagen10.tiff"), np.zeros((4, 4), np.float32))
    out.mkdir()
    return str(data), str(out)


def test_run_fiber_channel_segmentation(host, g30, g31, tmp_path):
    channel, kw = chain_arguments(g30, g31)
    data, out = cohort(tmp_path, channel, ("fov10", "fov2", "fov1"), sub="TIFs")
    table = fs.run_fiber_channel_segmentation(data, "Collagen1", out, img_sub_folder="TIFs", **kw)
    one = fs.fiber_object_props(g31["chain_labels"], "fov1")
    assert table["fov"].tolist() == ["fov1"] * len(one) + ["fov2"] * len(one) + ["fov10"] * len(one)     # natural order
    assert list(table.columns) == list(one.columns) + ["alignment_score"]
    assert sorted(os.listdir(out)) == ["fiber_object_table.csv", "fov10_fiber_labels.tiff", "fov1_fiber_labels.tiff",
                                       "fov2_fiber_labels.tiff"]
    for fov in ("fov1", "fov2", "fov10"):
        assert np.array_equal(image_io.read_image(os.path.join(out, fov + "_fiber_labels.tiff")), g31["chain_labels"])
    saved = pd.read_csv(os.path.join(out, "fiber_object_table.csv"))
    assert list(saved.columns) == list(table.columns) and len(saved) == len(table)                         # no index column
    pd.testing.assert_frame_equal(table.drop(columns="alignment_score").reset_index(drop=True),
                                  pd.concat([fs.fiber_object_props(g31["chain_labels"], f) for f in ("fov1", "fov2", "fov10")])
                                  .reset_index(drop=True))
    # debug on, through kwargs; compression, as the reference passes it on
    fs.run_fiber_channel_segmentation(data, "Collagen1", out, "TIFs", {"method": "gzip"}, debug=True, **kw)
    assert len(os.listdir(os.path.join(out, "_debug"))) == 12
    assert len(pd.read_csv(os.path.join(out, "fiber_object_table.csv"), compression="gzip")) == len(table)


def test_a_cohort_without_a_fibre_gives_the_empty_table(host, g30, g31, tmp_path):
    channel, kw = chain_arguments(g30, g31)
    data, out = cohort(tmp_path, channel, ("fov1", "fov2"))
    table = fs.run_fiber_channel_segmentation(data, "Collagen1", out, **dict(kw, min_fiber_size=int(g31["chain_largest"]) + 1))
    assert len(table) == 0 and list(table.columns) == ["fov"] + list(fs._object_columns(fs.FIBER_OBJECT_PROPS))
    assert list(pd.read_csv(os.path.join(out, "fiber_object_table.csv")).columns) == list(table.columns)
    assert not image_io.read_image(os.path.join(out, "fov2_fiber_labels.tiff")).any()


def test_run_fiber_channel_segmentation_refusals(host, g30, g31, tmp_path):
    channel, kw = chain_arguments(g30, g31)
    data, out = cohort(tmp_path, channel, ("fov1", "fov2"))
    with pytest.raises(FileNotFoundError):
        fs.run_fiber_channel_segmentation(str(tmp_path / "nowhere"), "Collagen1", out)
    with pytest.raises(FileNotFoundError):
        fs.run_fiber_channel_segmentation(data, "Collagen1", str(tmp_path / "nowhere"))
    with pytest.raises(ValueError, match="fiber_channel"):
        fs.run_fiber_channel_segmentation(data, "Collagen", out)
    with pytest.raises(FileNotFoundError):
        fs.run_fiber_channel_segmentation(data, "Collagen1", out, img_sub_folder="TIFs")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no FOV folder"):
        fs.run_fiber_channel_segmentation(str(empty), "Collagen1", out)
    for name in ("save_csv", "fov"):
        with pytest.raises(TypeError):
            fs.run_fiber_channel_segmentation(data, "Collagen1", out, **{name: True})
    os.remove(os.path.join(data, "fov2", "Collagen1.tiff"))
    with pytest.raises(ValueError, match="fov2"):
        fs.run_fiber_channel_segmentation(data, "Collagen1", out, **kw)


def test_the_reference_named_entries_still_refuse_and_the_docstring_names_the_new_ones(tmp_path):
    with pytest.raises(NotImplementedError, match="segment_fibers: the front half of fibre segmentation"):
        fs.segment_fibers(None, "Collagen1", str(tmp_path), "fov1")
    for name in ("watershed_labels", "segment_fiber_channel", "run_fiber_channel_segmentation", "RECALLED_WATERSHED", "K28"):
        assert name in fs.__doc__, name
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "run_fiber_channel_segmentation" in text and "skimage.segmentation.watershed(got" not in text, doc


def test_the_wrappers_are_named_and_refuse_without_a_device():
    import torch
    from ark_analysis_amd import som_device
    from ark_analysis_amd.som_device import planes
    for name in ("watershed", "channel_fiber_labels", "WATERSHED_STATS"):
        assert getattr(som_device, name) is getattr(planes, name)
    assert som_device.WATERSHED_STATS == ("rounds", "levels", "descents", "labelled")
    e = torch.zeros((4, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        som_device.watershed(e, e)
    with pytest.raises(ValueError):
        som_device.channel_fiber_labels(torch.zeros((8, 8), dtype=torch.float64))


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pxsom_watershed_workspace_bytes", "pxsom_watershed")


def test_abi_symbols_and_refusals():
    from ark_analysis_amd import _capi
    header = open(os.path.join(ROOT, "include", "pxsom.h")).read()
    assert _capi.ABI_VERSION == 9 and "#define PXSOM_ABI_VERSION 9" in header
    section = header.split("the marker watershed (K28)", 1)[1]
    for word in ("tests/watershed_reference.py", "parity with skimage itself", "raster order", "-W, -1, +1,", "stats_host"):
        assert word in section, word
    lib = _capi.lib()
    assert lib.pxsom_abi_version() == 9
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and re.search(r"\b%s\(" % name, header) and hasattr(lib, name), name
    invalid, unsupported, workspace = -1, -2, -3
    need = lib.pxsom_watershed_workspace_bytes(6, 8)
    assert need >= 6 * 8 * 40 and lib.pxsom_watershed_workspace_bytes(200, 230) > need
    for h, w in ((0, 8), (8, 0), (-1, 4), (65536, 65536)):
        assert lib.pxsom_watershed_workspace_bytes(h, w) == 0
    assert (lib.pxsom_watershed_workspace_bytes(65536, 65536) == 0) == (lib.pxsom_label_components_workspace_bytes(65536, 65536) == 0)
    # host arrays stand in for the device buffers: every call below is refused before any HIP call
    elev, markers, out = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(64, np.int32)
    ws = np.zeros(need // 8 + 4, np.float64)
    stats = np.full(4, -1, np.int64)
    E, M, O, W = elev.ctypes.data, markers.ctypes.data, out.ctypes.data, (ws.ctypes.data + 15) // 16 * 16
    order = ("elev", "lde", "markers", "ldm", "h", "w", "out", "ldo", "ws", "wsb", "stats", "stream")
    good = [E, 8, M, 8, 6, 8, O, 8, W, need, stats.ctypes.data, None]

    def refused(code, **changes):
        args = list(good)
        for key, value in changes.items():
            args[order.index(key)] = value
        rc = lib.pxsom_watershed(*args)
        assert rc == code and lib.pxsom_last_error().decode().startswith("pxsom_watershed"), (changes, rc)

    for changes in (dict(elev=None), dict(markers=None), dict(out=None), dict(elev=E + 2), dict(markers=M + 1), dict(out=O + 3),
                    dict(h=0), dict(w=0), dict(h=-6), dict(w=-8), dict(lde=7), dict(ldm=7), dict(ldo=7), dict(out=E), dict(out=M),
                    dict(out=E + 4 * 40), dict(out=M - 4 * 40), dict(ws=W + 8)):
        refused(invalid, **changes)
    for changes in (dict(ws=None), dict(wsb=need - 1), dict(wsb=0)):
        refused(workspace, **changes)
    far = 1 << 44
    refused(unsupported, h=65536, w=65536, lde=65536, ldm=65536, ldo=65536, markers=E + far, out=E + 2 * far)
    assert not out.any() and not ws.any() and (stats == -1).all()
