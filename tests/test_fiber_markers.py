"""From the ridge map to the watershed's inputs (K25) without a GPU: the scipy / numpy statement of
tests/fiber_markers_reference.py against the g28 fixtures, fiber_watershed_inputs with its one device entry swapped for that
statement, the multi-Otsu choice on a histogram with every recalled switch, the refusals, the debug files, the ABI."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ark_analysis_amd import image_io
from ark_analysis_amd.segmentation import fiber_segmentation as fs
from tests import fiber_markers_reference as fmr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURE = "g28_fiber_markers.npz"
NEW_SYMBOLS = ("pxsom_distance_transform_edt_workspace_bytes", "pxsom_distance_transform_edt", "pxsom_plane_greater",
               "pxsom_plane_minmax_workspace_bytes", "pxsom_plane_minmax", "pxsom_plane_histogram", "pxsom_sobel_magnitude",
               "pxsom_class_markers")


@pytest.fixture(scope="module")
def g28():
    return np.load(os.path.join(GOLDEN, FIXTURE))


def names(g28):
    return json.loads(str(g28["names"]))


@pytest.fixture
def statement_as_device(monkeypatch):
    monkeypatch.setattr(fs, "_watershed_inputs_device", fmr.watershed_inputs)
    return fs


# ---- the statement and the mirror against the fixtures ----------------------------------------------------------------------
def test_statement_equals_the_fixtures(g28):
    cutoff, sobel_blur = float(g28["cutoff"]), float(g28["sobel_blur"])
    settings = json.loads(str(g28["settings"]))
    assert len(names(g28)) == 8 and len(settings) == 4
    for name in names(g28):
        fg = g28["fg_" + name]
        s = fmr.stages(fmr.ridge_plane(fg, cutoff), cutoff, sobel_blur)
        assert np.array_equal(s["fg"], fg), name
        assert np.array_equal(fmr.squared_distances(fg), g28["sq_" + name]), name
        assert np.array_equal(fmr.distance_transform_edt(fg), np.sqrt(g28["sq_" + name].astype(np.float64))), name
        for key in ("dist", "counts", "markers", "elev", "elevation"):
            assert s[key].dtype == g28[key + "_" + name].dtype and np.array_equal(s[key], g28[key + "_" + name]), (name, key)
        assert s["counts"].sum() == fg.size and s["counts"].shape == (256,)
        for row, recalled in zip(g28["thr_" + name], settings):
            got = fs.threshold_multiotsu_from_histogram(s["counts"], s["edges"], recalled=recalled)
            assert np.array_equal(got, row), (name, recalled)
        assert np.array_equal(g28["thr_" + name][0], [s["t0"], s["t1"]]), name
        assert (np.bincount(g28["markers_" + name].ravel(), minlength=3) > 0).all(), name
    assert {g28["fg_" + n].shape for n in names(g28)} == {(64, 64), (40, 40), (40, 90), (90, 40)}


def test_mirror_equals_the_fixtures(statement_as_device, g28):
    cutoff, sobel_blur = float(g28["cutoff"]), float(g28["sobel_blur"])
    for name in names(g28):
        got = fs.fiber_watershed_inputs(fmr.ridge_plane(g28["fg_" + name], cutoff), cutoff, sobel_blur)
        assert got._fields == ("distance_transformed", "thresholds", "markers", "elevation_map")
        assert got.distance_transformed.dtype == np.float64 and np.array_equal(got.distance_transformed, g28["dist_" + name]), name
        assert got.thresholds.dtype == np.float64 and np.array_equal(got.thresholds, g28["thr_" + name][0]), name
        assert got.markers.dtype == np.int32 and np.array_equal(got.markers, g28["markers_" + name]), name
        assert got.elevation_map.dtype == np.int32 and np.array_equal(got.elevation_map, g28["elevation_" + name]), name
    # the reference's defaults, and a plane of another dtype
    fg = g28["fg_disc"]
    a = fs.fiber_watershed_inputs(fmr.ridge_plane(fg))
    b = fs.fiber_watershed_inputs(fmr.ridge_plane(fg).astype(np.float32), ridge_cutoff=0.1, sobel_blur=1)
    assert np.array_equal(a.markers, g28["markers_disc"]) and np.array_equal(b.markers, a.markers)


def test_the_device_entry_receives_the_host_choice(monkeypatch):
    calls = []

    def entry(ridges, cutoff, sobel_blur, thresholds):
        calls.append((ridges.dtype, ridges.shape, cutoff, sobel_blur, thresholds))
        return np.zeros((3, 4)), (0.5, 1.5), np.zeros((3, 4), np.int64), np.zeros((3, 4), np.int64)

    monkeypatch.setattr(fs, "_watershed_inputs_device", entry)
    got = fs.fiber_watershed_inputs(np.ones((3, 4), np.float32), 0.25, 2)
    assert calls == [(np.float64, (3, 4), 0.25, 2, fs.threshold_multiotsu_from_histogram)]
    assert got.markers.dtype == np.int32 and got.elevation_map.dtype == np.int32 and got.thresholds.tolist() == [0.5, 1.5]


# ---- multi-Otsu on a histogram ----------------------------------------------------------------------------------------------
def edges_of(nbins, lo=0.0, hi=1.0):
    return np.linspace(lo, hi, nbins + 1)


def brute_multiotsu(counts):
    """(best criterion, the pairs that attain it) by the definition: sum over the three classes of S^2 / P in binary64."""
    prob = counts / counts.sum()
    idx = np.arange(counts.size, dtype=np.float64)
    best, pairs = -1.0, []
    for i in range(counts.size - 2):
        for j in range(i + 1, counts.size - 1):
            total = 0.0
            for lo, hi in ((0, i + 1), (i + 1, j + 1), (j + 1, counts.size)):
                p = prob[lo:hi].sum()
                if p > 0:
                    total += (idx[lo:hi] * prob[lo:hi]).sum() ** 2 / p
            if total > best + 1e-12:
                best, pairs = total, [(i, j)]
            elif abs(total - best) <= 1e-12:
                pairs.append((i, j))
    return best, pairs


def test_multiotsu_is_the_maximum_of_the_criterion():
    rs = np.random.RandomState(5)
    for nbins in (4, 9, 24):
        for _ in range(4):
            counts = rs.randint(1, 200, nbins)                 # every bin occupied: a generic histogram has no tie
            edges = edges_of(nbins, -2.0, 5.0)
            centres = (edges[:-1] + edges[1:]) / 2
            _, pairs = brute_multiotsu(counts)
            assert len(pairs) == 1
            got = fs.threshold_multiotsu_from_histogram(counts, edges)
            assert np.array_equal(got, centres[list(pairs[0])])


def test_multiotsu_tie_rule():
    # two modes with empty bins between them and a third class: moving a threshold across the empty bins leaves the
    # criterion bit-equal, and "first" takes the lowest pair in (i, j) order, "last" the highest
    counts = np.zeros(16, np.int64)
    counts[[1, 2]] = 30, 50
    counts[[7, 8]] = 40, 45
    counts[[13, 14]] = 25, 60
    edges = edges_of(16)
    centres = (edges[:-1] + edges[1:]) / 2
    _, pairs = brute_multiotsu(counts)
    assert set(pairs) == {(i, j) for i in range(2, 7) for j in range(8, 13)}
    first = fs.threshold_multiotsu_from_histogram(counts, edges)
    last = fs.threshold_multiotsu_from_histogram(counts, edges, recalled={"tie": "last"})
    assert np.array_equal(first, centres[[2, 8]]) and np.array_equal(last, centres[[6, 12]])
    assert fs.RECALLED_MULTIOTSU["tie"] == "first"
    for prob in ("float32", "float64"):
        assert np.array_equal(fs.threshold_multiotsu_from_histogram(counts, edges, recalled={"prob": prob}), first)


def test_multiotsu_few_values_and_switches():
    edges = edges_of(8)
    centres = (edges[:-1] + edges[1:]) / 2
    two = np.array([0, 5, 0, 0, 0, 9, 0, 0])
    with pytest.raises(ValueError, match="only 2 different values. It cannot be thresholded in 3 classes"):
        fs.threshold_multiotsu_from_histogram(two, edges)
    with pytest.raises(ValueError, match="only 1 different values"):
        fs.threshold_multiotsu_from_histogram(np.array([0, 0, 7, 0, 0, 0, 0, 0]), edges)
    assert fs.threshold_multiotsu_from_histogram(two, edges, recalled={"few_bins": "search"}).shape == (2,)
    # exactly three occupied bins: the first two occupied bins; the search puts the first threshold there too, by the
    # tie rule, and the second on the second occupied bin
    three = np.array([0, 5, 0, 0, 9, 0, 0, 4])
    assert np.array_equal(fs.threshold_multiotsu_from_histogram(three, edges), centres[[1, 4]])
    assert np.array_equal(fs.threshold_multiotsu_from_histogram(three, edges, recalled={"exact_bins": "search"}), centres[[1, 4]])
    got = fs.threshold_multiotsu_from_histogram(three, edges, recalled={"exact_bins": "search", "tie": "last"})
    assert np.array_equal(got, centres[[3, 6]])
    assert fs.RECALLED_MULTIOTSU == {"prob": "float64", "tie": "first", "exact_bins": "occupied", "few_bins": "raise"}
    assert set(fs.MULTIOTSU_CHOICES) == set(fs.RECALLED_MULTIOTSU)
    assert all(fs.RECALLED_MULTIOTSU[k] == v[0] for k, v in fs.MULTIOTSU_CHOICES.items())
    with pytest.raises(ValueError, match="tie='middle'"):
        fs.threshold_multiotsu_from_histogram(three, edges, recalled={"tie": "middle"})
    with pytest.raises(ValueError, match="order"):
        fs.threshold_multiotsu_from_histogram(three, edges, recalled={"order": "first"})
    with pytest.raises(NotImplementedError, match="classes=4"):
        fs.threshold_multiotsu_from_histogram(three, edges, classes=4)
    with pytest.raises(ValueError, match="edges one longer"):
        fs.threshold_multiotsu_from_histogram(three, edges[:-1])
    with pytest.raises(ValueError, match="positive sum"):
        fs.threshold_multiotsu_from_histogram(np.zeros(8, np.int64), edges)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(statement_as_device):
    with pytest.raises(ValueError, match=fmr.NO_BACKGROUND):
        fs.fiber_watershed_inputs(np.full((6, 7), 3.0))                       # every pixel above the cutoff
    with pytest.raises(ValueError, match="only 1 different values"):
        fs.fiber_watershed_inputs(np.zeros((6, 7)))                           # a constant plane: a constant distance map
    with pytest.raises(ValueError, match="only 1 different values"):
        fs.fiber_watershed_inputs(np.full((6, 7), np.nan))                    # NaN > cutoff is False: all background
    with pytest.raises(ValueError):
        fmr.histogram(np.array([[0.0, np.nan], [1.0, 2.0]]))                  # numpy refuses NaN in the histogram's range
    with pytest.raises(NotImplementedError, match="sigma 17"):
        fs.fiber_watershed_inputs(np.zeros((6, 7)), sobel_blur=17)
    for bad in (np.zeros(5), np.zeros((2, 3, 4)), np.zeros((0, 4))):
        with pytest.raises(ValueError, match="non-empty \\[H, W\\]"):
            fs.fiber_watershed_inputs(bad)


def test_plane_histogram_edges_and_nan_rule():
    from ark_analysis_amd.som_device import planes
    assert np.array_equal(planes.histogram_edges(-1.5, 7.25, 256), np.histogram(np.array([-1.5, 7.25]), 256)[1])
    assert np.array_equal(planes.histogram_edges(3.0, 3.0, 4), np.histogram(np.array([3.0]), 4)[1])
    for lo, hi in ((0.0, np.inf), (-np.inf, 0.0), (np.nan, np.nan)):
        with pytest.raises(ValueError, match="not finite"):
            planes.histogram_edges(lo, hi, 8)


# ---- the debug files --------------------------------------------------------------------------------------------------------
def test_debug_files(statement_as_device, g28, tmp_path):
    ridges = fmr.ridge_plane(g28["fg_wide"])
    got = fs.fiber_watershed_inputs(ridges, out_dir=str(tmp_path), fov="fov3", debug=True)
    assert sorted(os.listdir(tmp_path / "_debug")) == ["fov3_ridges_thresholded.tiff", "fov3_thresholded.tiff"]
    threshed = image_io.read_image(str(tmp_path / "_debug" / "fov3_thresholded.tiff"))
    dist = image_io.read_image(str(tmp_path / "_debug" / "fov3_ridges_thresholded.tiff"))
    assert threshed.dtype == np.float32 and np.array_equal(threshed, g28["markers_wide"])
    assert dist.dtype == np.float32 and np.array_equal(dist, g28["dist_wide"].astype(np.float32))
    assert np.array_equal(got.markers, g28["markers_wide"])
    # without debug, or without a folder, nothing is written
    fs.fiber_watershed_inputs(ridges, out_dir=str(tmp_path / "quiet"), fov="fov3", debug=False)
    fs.fiber_watershed_inputs(ridges, debug=True)
    assert not (tmp_path / "quiet").exists()
    with pytest.raises(FileNotFoundError):
        fs.fiber_watershed_inputs(ridges, out_dir=str(tmp_path / "missing"), fov="fov3", debug=True)
    with pytest.raises(ValueError, match="need fov"):
        fs.fiber_watershed_inputs(ridges, out_dir=str(tmp_path), debug=True)


# ---- the generator reproduces the committed fixture ---------------------------------------------------------------------------
def test_generator_reproduces_the_fixture(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_fiber_markers.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / FIXTURE), np.load(os.path.join(GOLDEN, FIXTURE))
    assert sorted(new.files) == sorted(old.files)
    for key in old.files:
        assert new[key].dtype == old[key].dtype and np.array_equal(new[key], old[key]), key
    assert os.path.getsize(os.path.join(GOLDEN, FIXTURE)) <= 256 * 1024


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_refusals():
    from ark_analysis_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pxsom.h")).read()
    assert _capi.ABI_VERSION == 9
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and re.search(r"\b%s\(" % name, header), name
    lib = _capi.lib()
    assert lib.pxsom_abi_version() == 9
    invalid, unsupported, workspace = -1, -2, -3       # PXSOM_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE
    # host arrays stand in for the device planes: every call below is refused before any HIP call
    plane, out = np.zeros(64), np.zeros(64)
    u8, i32, ws = np.zeros(64, np.uint8), np.zeros(64, np.int32), np.zeros(4096 * 8)
    P, O, U, I, W = (a.ctypes.data for a in (plane, out, u8, i32, ws))

    def refused(code, entry, *args):
        rc = getattr(lib, entry)(*args)
        assert rc == code and lib.pxsom_last_error().decode().startswith(entry), (entry, args, rc)

    edt = "pxsom_distance_transform_edt"
    assert lib.pxsom_distance_transform_edt_workspace_bytes(8, 8) == 256 + 64        # g, one band summary
    assert lib.pxsom_distance_transform_edt_workspace_bytes(0, 8) == 0
    assert lib.pxsom_distance_transform_edt_workspace_bytes(46341, 1) == 0
    for args in ((None, 8, 8, 8, O, 8, I, 8, W, 320), (U, 8, 8, 8, None, 8, None, 8, W, 320), (U, 0, 8, 8, O, 8, I, 8, W, 320),
                 (U, 8, -1, 8, O, 8, I, 8, W, 320), (U, 8, 8, 7, O, 8, I, 8, W, 320), (U, 8, 8, 8, O, 7, I, 8, W, 320),
                 (U, 8, 8, 8, O, 8, I, 7, W, 320), (U, 8, 8, 8, O + 4, 8, I, 8, W, 320), (U, 8, 8, 8, O, 8, I + 2, 8, W, 320),
                 (U, 8, 8, 8, O, 8, I, 8, W + 1, 320)):
        refused(invalid, edt, *args, None)
    refused(workspace, edt, U, 8, 8, 8, O, 8, I, 8, W, 319, None)
    refused(workspace, edt, U, 8, 8, 8, O, 8, I, 8, None, 320, None)
    for h, w in ((46341, 1), (1, 46341), (32768, 32768)):       # h^2 + w^2 > INT32_MAX: refused without a launch
        refused(unsupported, edt, U, h, w, w, O, w, I, w, W, 1 << 40, None)

    refused(invalid, "pxsom_plane_greater", None, 8, 8, 8, 0.1, U, 8, None)
    refused(invalid, "pxsom_plane_greater", P, 8, 8, 8, 0.1, None, 8, None)
    refused(invalid, "pxsom_plane_greater", P, 8, 8, 8, float("nan"), U, 8, None)
    refused(invalid, "pxsom_plane_greater", P, 8, 8, 7, 0.1, U, 8, None)
    refused(invalid, "pxsom_plane_greater", P, 8, 8, 8, 0.1, U, 7, None)
    refused(invalid, "pxsom_plane_greater", P + 4, 8, 8, 8, 0.1, U, 8, None)
    refused(unsupported, "pxsom_plane_greater", P, 65536, 65536, 65536, 0.1, U, 65536, None)

    wsb = lib.pxsom_plane_minmax_workspace_bytes()
    assert 0 < wsb <= ws.nbytes
    for args in ((None, 8, 8, 8, O, W, wsb), (P, 8, 8, 8, None, W, wsb), (P, 0, 8, 8, O, W, wsb), (P, 8, 8, 7, O, W, wsb),
                 (P, 8, 8, 8, O + 4, W, wsb), (P, 8, 8, 8, O, W + 4, wsb)):
        refused(invalid, "pxsom_plane_minmax", *args, None)
    refused(workspace, "pxsom_plane_minmax", P, 8, 8, 8, O, W, wsb - 1, None)
    refused(workspace, "pxsom_plane_minmax", P, 8, 8, 8, O, None, wsb, None)
    refused(unsupported, "pxsom_plane_minmax", P, 65536, 65536, 65536, O, W, wsb, None)

    for args in ((None, 8, 8, 8, O, 4, W), (P, 8, 8, 8, None, 4, W), (P, 8, 8, 8, O, 4, None), (P, 8, 8, 8, O, 0, W),
                 (P, 8, 8, 8, O, 1025, W), (P, 8, 0, 8, O, 4, W), (P, 8, 8, 7, O, 4, W), (P, 8, 8, 8, O + 4, 4, W)):
        refused(invalid, "pxsom_plane_histogram", *args, None)
    refused(unsupported, "pxsom_plane_histogram", P, 65536, 65536, 65536, O, 4, W, None)

    for args in ((None, 8, 8, 8, O, 8, I, 8), (P, 8, 8, 8, None, 8, None, 8), (P, 8, 0, 8, O, 8, I, 8), (P, 8, 8, 7, O, 8, I, 8),
                 (P, 8, 8, 8, O, 7, I, 8), (P, 8, 8, 8, O, 8, I, 7), (P, 8, 8, 8, O + 4, 8, I, 8), (P, 8, 8, 8, O, 8, I + 2, 8),
                 (P, 8, 8, 8, P, 8, I, 8), (P, 8, 8, 8, P + 8 * 63, 8, None, 8), (P, 8, 8, 8, None, 8, P + 4 * 60, 8)):
        refused(invalid, "pxsom_sobel_magnitude", *args, None)
    refused(unsupported, "pxsom_sobel_magnitude", P, 65536, 65536, 65536, O + (1 << 44), 65536, None, 65536, None)

    for args in ((None, 8, 8, 8, 0.5, 1.5, I, 8), (P, 8, 8, 8, 0.5, 1.5, None, 8), (P, 8, 8, 8, float("nan"), 1.5, I, 8),
                 (P, 8, 8, 8, 0.5, float("nan"), I, 8), (P, 0, 8, 8, 0.5, 1.5, I, 8), (P, 8, 8, 7, 0.5, 1.5, I, 8),
                 (P, 8, 8, 8, 0.5, 1.5, I, 7), (P, 8, 8, 8, 0.5, 1.5, I + 2, 8)):
        refused(invalid, "pxsom_class_markers", *args, None)
    refused(unsupported, "pxsom_class_markers", P, 65536, 65536, 65536, 0.5, 1.5, I, 65536, None)


def test_the_wrappers_are_on_the_facade():
    from ark_analysis_amd import som_device
    from ark_analysis_amd.som_device import planes
    for name in ("distance_transform_edt", "plane_minmax", "plane_histogram", "sobel_magnitude", "class_markers",
                 "watershed_inputs", "plane_greater"):
        assert getattr(som_device, name) is getattr(planes, name), name


# ---- the reference's three entries still refuse as before -----------------------------------------------------------------------
def test_the_entries_still_refuse(tmp_path):
    assert "equalize_adapthist, frangi, threshold_multiotsu, sobel, watershed" in fs._UNBUILT
    with pytest.raises(NotImplementedError, match="segment_fibers: the front half of fibre segmentation"):
        fs.segment_fibers(None, "Collagen1", str(tmp_path), "fov1")
    (tmp_path / "data" / "fov1").mkdir(parents=True)
    image_io.write_image(str(tmp_path / "data" / "fov1" / "Collagen1.tiff"), np.zeros((4, 4), np.float32))
    with pytest.raises(NotImplementedError, match="run_fiber_segmentation: the front half"):
        fs.run_fiber_segmentation(str(tmp_path / "data"), "Collagen1", str(tmp_path))
    with pytest.raises(NotImplementedError, match="plot_fiber_segmentation_steps: the front half"):
        fs.plot_fiber_segmentation_steps(str(tmp_path / "data"), "fov1", "Collagen1")
