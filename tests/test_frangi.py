"""The Frangi ridge filter of fibre segmentation (K26) without a GPU: the numpy / scipy statement of
tests/frangi_reference.py against the g29 fixture, its own exponential against np.exp, frangi_ridges and
fiber_watershed_inputs_from_contrast with their device entries swapped for that statement, the refusals, the debug
files, the ABI."""
import hashlib
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
from tests import frangi_reference as fr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
FIXTURE = "g29_frangi.npz"
CHAINED, DIGESTED = ("bars", "disc"), ("wide", "tall")


@pytest.fixture(scope="module")
def g29():
    return np.load(os.path.join(GOLDEN, FIXTURE))


def names(g29):
    return json.loads(str(g29["names"]))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture
def statement_as_device(monkeypatch):
    monkeypatch.setattr(fs, "_frangi_device", fr.frangi_device)
    monkeypatch.setattr(fs, "_ridge_watershed_inputs_device", fr.ridge_watershed_inputs_device)
    return fs


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- the statement against the fixture ---------------------------------------------------------------------------------------
def test_statement_equals_the_fixture(g29):
    planes = fr.fixture_planes()
    assert names(g29) == list(planes) and len(planes) == 10
    assert g29["sigmas"].tolist() == [1, 3, 5, 7, 9] and float(g29["beta"]) == 0.5 and float(g29["gamma"]) == 15
    assert float(g29["scale"]) == 10000
    assert {planes[n].shape for n in DIGESTED} == {(40, 90), (90, 40)}
    for name, x in planes.items():
        s = fr.stages(x, g29["sigmas"], float(g29["beta"]), float(g29["gamma"]), float(g29["scale"]))
        assert s["scales"].shape == (5,) + x.shape
        assert same(s["ridges"], g29["ridges_" + name]), name
        if name in DIGESTED:
            assert digest(s["scales"]) == str(g29["sha256_scales_" + name]), name
            assert digest(s["folded"]) == str(g29["sha256_folded_" + name]), name
        else:
            assert same(s["scales"], g29["scales_" + name]) and same(s["folded"], g29["folded_" + name]), name
            assert np.array_equal(g29["ridges_" + name], g29["folded_" + name] * 10000.0), name
        assert np.array_equal(fr.frangi(x, scale=10000), g29["ridges_" + name]), name
    assert not g29["folded_constant"].any()
    assert g29["folded_bars"].max() > 1e-4 and (g29["folded_bars"] == 0).any()
    assert g29["folded_bars_1e6"].max() > 0.999
    # the same bars, dark on bright, are weaker where the bars are, not all zero: the shoulders of a dark bar respond
    on_bars = planes["bars"] >= 1.0
    assert g29["folded_dark_bars"][on_bars].mean() < 0.25 * g29["folded_bars"][on_bars].mean()
    assert g29["folded_dark_bars"].any()


def test_chained_cases_carry_every_k25_stage(g29):
    cutoff, sobel_blur = float(g29["cutoff"]), float(g29["sobel_blur"])
    for name in CHAINED:
        s = fmr.stages(g29["ridges_" + name], cutoff, sobel_blur)
        for key in ("fg", "dist", "counts", "markers", "elev", "elevation"):
            assert same(s[key], g29["%s_%s" % (key, name)]), (name, key)
        assert [s["t0"], s["t1"]] == g29["thr_" + name].tolist(), name
        assert (np.bincount(g29["markers_" + name].ravel(), minlength=3) > 0).all(), name


def test_generator_reproduces_the_fixture(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_frangi.py")], check=True, env=env, stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / FIXTURE), np.load(os.path.join(GOLDEN, FIXTURE))
    assert sorted(new.files) == sorted(old.files)
    for key in old.files:
        assert new[key].dtype == old[key].dtype and np.array_equal(new[key], old[key]), key
    assert os.path.getsize(os.path.join(GOLDEN, FIXTURE)) <= 211804          # g28's size


# ---- exp_neg -----------------------------------------------------------------------------------------------------------------
def test_exp_neg_against_np_exp(g29):
    e = float(g29["exp_gap_e"])
    assert 0.0 < e < 4.0
    grid = fr.exp_neg_grid()
    assert grid.size > 400000 and grid.min() == -708.0 and grid.max() == 0.0
    assert fr.exp_neg_gap(grid) <= e
    assert float(g29["exp_gap_observed"]) <= 2.0 * e + 2.0
    got = fr.exp_neg(np.array([0.0, -0.0, -708.0, np.nextafter(-708.0, -np.inf), -1e4, -np.inf, np.nan]))
    assert got[:2].tolist() == [1.0, 1.0] and got[2] >= 2.0 ** -1022 and got[3:6].tolist() == [0.0, 0.0, 0.0] and np.isnan(got[6])
    assert (fr.exp_neg(grid) >= 2.0 ** -1022).all() and (fr.exp_neg(grid) <= 1.0).all()        # never subnormal, never above 1
    assert fr.exp_neg(np.zeros((3, 4))).shape == (3, 4)


def test_the_figures_are_in_the_design_document(g29):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "E = %.4f" % float(g29["exp_gap_e"]) in text
    assert "%.4f units of 2⁻⁵³" % float(g29["exp_gap_observed"]) in text


def test_the_kernel_states_the_same_constants():
    src = open(os.path.join(ROOT, "ark_analysis_amd", "csrc", "pxsom_frangi.hip")).read()
    for value in (fr.LOG2E, fr.LN2_HI, fr.LN2_LO) + fr.INV_FACTORIAL[3:]:
        assert repr(value) in src, value
    assert "kExpNegFloor = -708.0" in src and "fp contract(off)" in src and "1e-10" in src
    assert not re.search(r"\b(exp|expm1|pow|log)\(", src.split("namespace {", 1)[1])           # no maths-library exponential


# ---- the statement's own rules -----------------------------------------------------------------------------------------------
def test_statement_rules():
    x = fr.patterns(9, 11)["bars"]
    # np.maximum propagates NaN; a NaN pixel spreads as far as the widest blur reaches
    x_nan = x.copy()
    x_nan[4, 5] = np.nan
    got = fr.frangi(x_nan, (1,))
    assert np.isnan(got[4, 5]) and np.isnan(got).sum() > 1
    # alpha does not enter; beta and gamma do
    assert not np.array_equal(fr.frangi(x, (1,), beta=0.5), fr.frangi(x, (1,), beta=0.6))
    assert not np.array_equal(fr.frangi(x, (1,), gamma=15), fr.frangi(x, (1,), gamma=14))
    # the fold is the maximum of the scales, the scale a product after it
    one, three = fr.frangi(x, (1,)), fr.frangi(x, (3,))
    assert np.array_equal(fr.frangi(x, (1, 3), scale=10000), np.maximum(one, three) * 10000.0)
    for shape in ((1, 5), (5, 1), (1, 1)):
        with pytest.raises(ValueError, match=fr.TOO_SMALL):
            fr.frangi(np.zeros(shape))
    assert fr.frangi(np.zeros((2, 2))).shape == (2, 2)


# ---- the host functions over the swapped statement ---------------------------------------------------------------------------
def test_frangi_ridges_equals_the_fixture(statement_as_device, g29):
    for name, x in fr.fixture_planes().items():
        got = fs.frangi_ridges(x)
        assert same(got, g29["ridges_" + name]), name
    x = fr.fixture_planes()["disc"]
    assert np.array_equal(fs.frangi_ridges(x.astype(np.float32), fiber_widths=[1, 3, 5, 7, 9], beta=0.5, gamma=15, scale=10000),
                          g29["ridges_disc"])
    assert np.array_equal(fs.frangi_ridges(x, scale=1), g29["folded_disc"])
    # sigmas are flattened as skimage flattens them
    assert np.array_equal(fs.frangi_ridges(x, fiber_widths=np.array([[1, 3], [5, 7]]), scale=1),
                          fr.frangi(x, (1, 3, 5, 7)))
    assert np.array_equal(fs.frangi_ridges(x, fiber_widths=(s for s in (1, 3)), scale=1), fr.frangi(x, (1, 3)))
    assert np.array_equal(fs.frangi_ridges(x, fiber_widths=3, scale=1), fr.frangi(x, (3,)))


def test_the_device_entries_receive_checked_arguments(monkeypatch):
    calls = []

    def entry(image, sigmas, beta, gamma, scale):
        calls.append((image.dtype, image.shape, sigmas, beta, gamma, scale))
        return np.zeros(image.shape, np.float32)

    monkeypatch.setattr(fs, "_frangi_device", entry)
    got = fs.frangi_ridges(np.ones((3, 4), np.int16), range(1, 4), beta=1, gamma=2, scale=3)
    assert calls == [(np.float64, (3, 4), [1.0, 2.0, 3.0], 1.0, 2.0, 3.0)] and got.dtype == np.float64
    assert all(type(v) is float for v in calls[0][2] + list(calls[0][3:]))

    def chain(contrast, sigmas, ridge_cutoff, sobel_blur, thresholds):
        calls.append((contrast.dtype, sigmas, ridge_cutoff, sobel_blur, thresholds))
        z = np.zeros(contrast.shape)
        return z, z, (0.5, 1.5), z.astype(np.int64), z.astype(np.int64)

    monkeypatch.setattr(fs, "_ridge_watershed_inputs_device", chain)
    inputs, ridges = fs.fiber_watershed_inputs_from_contrast(np.ones((3, 4), np.float32), ridge_cutoff=0.25, sobel_blur=2)
    assert calls[1] == (np.float64, [1.0, 3.0, 5.0, 7.0, 9.0], 0.25, 2, fs.threshold_multiotsu_from_histogram)
    assert inputs.markers.dtype == np.int32 and inputs.thresholds.tolist() == [0.5, 1.5] and ridges.dtype == np.float64


def test_chain_from_contrast_equals_the_fixture(statement_as_device, g29):
    planes = fr.fixture_planes()
    for name in CHAINED:
        inputs, ridges = fs.fiber_watershed_inputs_from_contrast(planes[name], ridge_cutoff=float(g29["cutoff"]),
                                                                 sobel_blur=float(g29["sobel_blur"]))
        assert isinstance(inputs, fs.WatershedInputs)
        assert same(ridges, g29["ridges_" + name]), name
        assert same(inputs.distance_transformed, g29["dist_" + name]) and same(inputs.thresholds, g29["thr_" + name]), name
        assert same(inputs.markers, g29["markers_" + name]) and same(inputs.elevation_map, g29["elevation_" + name]), name
    # the defaults are the reference's; the chain is frangi_ridges followed by fiber_watershed_inputs
    inputs, ridges = fs.fiber_watershed_inputs_from_contrast(planes["bars"])
    assert np.array_equal(inputs.markers, g29["markers_bars"]) and np.array_equal(ridges, fs.frangi_ridges(planes["bars"]))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(statement_as_device):
    x = np.zeros((6, 7))
    for call in (lambda **kw: fs.frangi_ridges(x, **kw), lambda **kw: fs.fiber_watershed_inputs_from_contrast(x, **kw)):
        for empty in ([], (), np.zeros(0), range(0)):
            with pytest.raises(ValueError, match="at least one sigma"):
                call(fiber_widths=empty)
        with pytest.raises(ValueError, match="Sigma values less than zero are not valid"):
            call(fiber_widths=[1, -0.5])
        with pytest.raises(ValueError, match="sigma 0 is not taken"):
            call(fiber_widths=[1, 0])
        with pytest.raises(ValueError, match="finite sigmas"):
            call(fiber_widths=[1, np.inf])
        with pytest.raises(ValueError, match="finite sigmas"):
            call(fiber_widths=[np.nan])
        with pytest.raises(NotImplementedError, match="sigma 16.125 is beyond the radius limit"):
            call(fiber_widths=[1, 16.125])
    assert fs.frangi_ridges(x, fiber_widths=[16.12]).shape == (6, 7)        # the widest radius the blur takes, 64
    with pytest.raises(NotImplementedError, match="black_ridges=True"):
        fs.frangi_ridges(x, black_ridges=True)
    with pytest.raises(NotImplementedError, match="gamma=None"):
        fs.frangi_ridges(x, gamma=None)
    for bad in (0, -1, np.inf, np.nan):
        with pytest.raises(ValueError, match="finite beta and gamma > 0"):
            fs.frangi_ridges(x, beta=bad)
        with pytest.raises(ValueError, match="finite beta and gamma > 0"):
            fs.frangi_ridges(x, gamma=bad)
    with pytest.raises(ValueError, match="scale must be finite"):
        fs.frangi_ridges(x, scale=np.nan)
    for call in (fs.frangi_ridges, fs.fiber_watershed_inputs_from_contrast):
        for shape in ((1, 7), (7, 1), (1, 1)):
            with pytest.raises(ValueError, match=fr.TOO_SMALL):
                call(np.zeros(shape))
        for bad in (np.zeros(5), np.zeros((2, 3, 4)), np.zeros((0, 4))):
            with pytest.raises(ValueError, match="non-empty \\[H, W\\]"):
                call(bad)
    with pytest.raises(NotImplementedError, match="sigma 17"):
        fs.fiber_watershed_inputs_from_contrast(x, sobel_blur=17)
    # what the K25 middle refuses comes through: a ridge map below the cutoff everywhere
    with pytest.raises(ValueError, match="only 1 different values"):
        fs.fiber_watershed_inputs_from_contrast(np.full((6, 7), 0.75))


def test_device_wrapper_refusals_without_a_device():
    from ark_analysis_amd import som_device
    from ark_analysis_amd.som_device import planes
    for name in ("frangi", "ridge_watershed_inputs", "frangi_arguments", "FRANGI_SIGMAS", "GRADIENT_TOO_SMALL"):
        assert getattr(som_device, name) is getattr(planes, name), name
    assert planes.FRANGI_SIGMAS == fr.SIGMAS and planes.GRADIENT_TOO_SMALL.startswith(fr.TOO_SMALL)
    assert planes.frangi_arguments(range(1, 10, 2), 0.5, 15) == ([1.0, 3.0, 5.0, 7.0, 9.0], 0.5, 450.0)
    import torch
    with pytest.raises(ValueError, match="2-D float64 HBM tensor"):
        som_device.frangi(torch.zeros((4, 4), dtype=torch.float64))


# ---- the debug files ---------------------------------------------------------------------------------------------------------
def test_debug_files(statement_as_device, g29, tmp_path):
    x = fr.fixture_planes()["bars"]
    got = fs.frangi_ridges(x, out_dir=str(tmp_path), fov="fov3", debug=True)
    assert os.listdir(tmp_path / "_debug") == ["fov3_frangi_filter.tiff"]
    saved = image_io.read_image(str(tmp_path / "_debug" / "fov3_frangi_filter.tiff"))
    assert saved.dtype == np.float32 and np.array_equal(saved, g29["ridges_bars"].astype(np.float32))
    assert np.array_equal(got, g29["ridges_bars"])
    chain_dir = tmp_path / "chain"
    chain_dir.mkdir()
    inputs, _ = fs.fiber_watershed_inputs_from_contrast(x, out_dir=str(chain_dir), fov="fov4", debug=True)
    assert sorted(os.listdir(chain_dir / "_debug")) == ["fov4_frangi_filter.tiff", "fov4_ridges_thresholded.tiff", "fov4_thresholded.tiff"]
    assert np.array_equal(image_io.read_image(str(chain_dir / "_debug" / "fov4_frangi_filter.tiff")), saved)
    assert np.array_equal(image_io.read_image(str(chain_dir / "_debug" / "fov4_thresholded.tiff")), g29["markers_bars"])
    assert np.array_equal(image_io.read_image(str(chain_dir / "_debug" / "fov4_ridges_thresholded.tiff")),
                          g29["dist_bars"].astype(np.float32))
    # without debug, or without a folder, nothing is written
    for call in (fs.frangi_ridges, fs.fiber_watershed_inputs_from_contrast):
        call(x, out_dir=str(tmp_path / "quiet"), fov="fov3", debug=False)
        call(x, debug=True)
        assert not (tmp_path / "quiet").exists()
        with pytest.raises(FileNotFoundError):
            call(x, out_dir=str(tmp_path / "missing"), fov="fov3", debug=True)
        with pytest.raises(ValueError, match="need fov"):
            call(x, out_dir=str(tmp_path), debug=True)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_symbol_and_refusals():
    from ark_analysis_amd import _capi
    header = open(os.path.join(ROOT, "include", "pxsom.h")).read()
    assert _capi.ABI_VERSION == 9 and "K26" in header
    assert "pxsom_frangi_scale" in _capi.SYMBOLS and re.search(r"\bpxsom_frangi_scale\(", header)
    lib = _capi.lib()
    assert lib.pxsom_abi_version() == 9 and hasattr(lib, "pxsom_frangi_scale")
    invalid, unsupported = -1, -2                       # PXSOM_ERR_INVALID_ARG, PXSOM_ERR_UNSUPPORTED
    # host arrays stand in for the device planes: every call below is refused before any HIP call
    g, out = np.zeros(64), np.zeros(64)
    G, O = g.ctypes.data, out.ctypes.data

    def refused(code, *args):
        rc = lib.pxsom_frangi_scale(*args)
        assert rc == code and lib.pxsom_last_error().decode().startswith("pxsom_frangi_scale"), (args, rc)

    good = [G, 8, 8, 8, 1.0, 0.5, 450.0, 1, 1.0, O, 8, None]

    def but(**changes):
        order = ("g", "ldg", "h", "w", "s2", "bsq", "gsq", "first", "scale", "out", "ldo", "stream")
        args = list(good)
        for key, value in changes.items():
            args[order.index(key)] = value
        return args

    for changes in (dict(g=None), dict(out=None), dict(h=1), dict(w=1), dict(h=0), dict(w=-3), dict(ldg=7), dict(ldo=7),
                    dict(g=G + 4), dict(out=O + 4), dict(out=G), dict(out=G + 8 * 63), dict(g=O + 8)):
        refused(invalid, *but(**changes))
    for key in ("s2", "bsq", "gsq"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(invalid, *but(**{key: bad}))
    refused(unsupported, *but(h=65536, w=65536, ldg=65536, ldo=65536, out=O + (1 << 44)))
    refused(unsupported, *but(h=4 * 65535 + 1, w=2, ldg=2, ldo=2, out=O + (1 << 44)))
    assert not g.any() and not out.any()


# ---- the reference's three entries still refuse as before ----------------------------------------------------------------------
def test_the_entries_still_refuse(tmp_path):
    assert fs._UNBUILT == ("the front half of fibre segmentation (equalize_adapthist, frangi, threshold_multiotsu, sobel, "
                           "watershed) is not implemented; from a segmented mask use fiber_objects, from saved "
                           "<fov>_fiber_labels.tiff files fiber_object_table_from_labels")
    with pytest.raises(NotImplementedError, match="segment_fibers: the front half of fibre segmentation"):
        fs.segment_fibers(None, "Collagen1", str(tmp_path), "fov1")
    (tmp_path / "data" / "fov1").mkdir(parents=True)
    image_io.write_image(str(tmp_path / "data" / "fov1" / "Collagen1.tiff"), np.zeros((4, 4), np.float32))
    with pytest.raises(NotImplementedError, match="run_fiber_segmentation: the front half"):
        fs.run_fiber_segmentation(str(tmp_path / "data"), "Collagen1", str(tmp_path))
    with pytest.raises(NotImplementedError, match="plot_fiber_segmentation_steps: the front half"):
        fs.plot_fiber_segmentation_steps(str(tmp_path / "data"), "fov1", "Collagen1")
