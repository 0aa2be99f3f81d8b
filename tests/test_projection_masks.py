"""Projection object masks (K22) without a GPU: the numpy statement of tests/projection_mask_reference.py against the g25
fixtures (made by the reference's own _create_object_mask(..., "projection") over a Meijering filter restated with
eigvalsh), the opt-in switch of the mirror with its one device entry swapped for that statement, the log line, the ABI."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ark_analysis_amd.segmentation.ez_seg import ez_object_segmentation as ez
from tests import projection_mask_reference as pmr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
IMAGES = ("lines", "discs", "ring", "noise", "quadrant", "mixed", "tiny", "flat")


@pytest.fixture(scope="module")
def g25():
    return np.load(os.path.join(GOLDEN, "g25_projection_masks.npz"))


def cases(g25):
    return json.loads(str(g25["cases"]))


@pytest.fixture
def meijering_on(monkeypatch):
    """The mirror with the switch on and its device entry swapped for the statement."""
    monkeypatch.setattr(ez, "PROJECTION_FILTER", "meijering")
    monkeypatch.setattr(ez, "_object_mask_device", pmr.object_mask)
    return ez


# ---- the statement against the fixtures -----------------------------------------------------------------------------------
def test_statement_equals_the_fixtures(g25):
    for key in IMAGES:
        got = pmr.ridge_sign(g25["img_" + key] > 0)
        assert got.dtype == np.uint8 and np.array_equal(got, g25["ridge_" + key]), key
    kinds = set()
    for c in cases(g25):
        got = pmr.create_projection_mask(g25["img_" + c["image"]], c["sigma"], c["thresh"], c["hole_size"], c["fov_dim"],
                                         c["min_object_area"], c["max_object_area"])
        assert got.dtype == np.int32 and np.array_equal(got, g25["mask_" + c["name"]]), c["name"]
        kinds.add((type(c["thresh"]).__name__, type(c["hole_size"]).__name__))
    assert len(kinds) == 9          # every threshold kind x every hole kind
    assert {c["image"] for c in cases(g25)} == set(IMAGES)
    assert g25["img_tiny"].shape == (3, 5) and g25["img_flat"].shape == (2, 9)
    assert sum(bool(g25["mask_" + c["name"]].any()) for c in cases(g25)) >= 14


def test_statement_flat_planes_edges_and_the_tie():
    for shape in ((2, 2), (5, 7), (40, 33)):
        assert not pmr.ridge_sign(np.zeros(shape, np.uint8)).any() and not pmr.ridge_sign(np.ones(shape, np.uint8)).any()
    # a one-pixel line is a ridge at its own pixels; an int 0 / 1 plane and a bool plane are one input
    line = np.zeros((21, 21), np.uint8)
    line[10] = 1
    got = pmr.ridge_sign(line)
    assert got[10].all() and not got[0].any()
    assert np.array_equal(pmr.ridge_sign(line.astype(np.int64) * 7), got) and np.array_equal(pmr.ridge_sign(line != 0), got)
    # the quadrant corner: on the diagonal through the corner the eigenvalues tie in magnitude and e_lo (negative) is taken
    x = pmr.quadrant(32, 32, 16, 16).astype(np.float64)
    hrr, hrc, hcc = pmr.hessian(x, 2)
    d, t = hrr - hcc, hrr + hcc
    r = np.sqrt(d * d + 4.0 * (hrc * hrc))
    tie = (np.abs((t - r) / 2.0) == np.abs((t + r) / 2.0)) & (r > 0)
    assert tie.any() and pmr.ridge_sign(x, [2])[tie].all()
    with pytest.raises(ValueError, match=pmr.TOO_SMALL):
        pmr.ridge_sign(np.ones((1, 9), np.uint8))


# ---- the mirror -----------------------------------------------------------------------------------------------------------
def test_mirror_equals_the_fixtures(meijering_on, g25):
    for c in cases(g25):
        got = meijering_on._create_object_mask(g25["img_" + c["image"]], "projection", c["sigma"], c["thresh"], c["hole_size"],
                                               c["fov_dim"], c["min_object_area"], c["max_object_area"])
        assert got.dtype == np.int32 and np.array_equal(got, g25["mask_" + c["name"]]), c["name"]


def test_the_switch(monkeypatch):
    img = np.ones((8, 8), np.float32)
    calls = []
    monkeypatch.setattr(ez, "_object_mask_device", lambda *a, **k: calls.append((a, k)) or np.zeros((8, 8), np.int32))
    assert ez.PROJECTION_FILTER is None
    with pytest.raises(NotImplementedError, match="projection.*PROJECTION_FILTER = 'meijering'"):
        ez._create_object_mask(img, "projection")
    monkeypatch.setattr(ez, "PROJECTION_FILTER", "frangi")
    with pytest.raises(ValueError, match="PROJECTION_FILTER must be None or 'meijering', got 'frangi'"):
        ez._create_object_mask(img, "projection")
    assert not calls
    ez._create_object_mask(img, "blob", 1, None, None)          # the blob route does not look at the switch
    assert len(calls) == 1 and calls[0][1] == {} and len(calls[0][0]) == 7
    monkeypatch.setattr(ez, "PROJECTION_FILTER", "meijering")   # read at call time
    ez._create_object_mask(img, "projection", 1, None, 5, 100, 2, 30)
    args, kwargs = calls[1]
    assert args[1:] == (1, None, 5, 2, 30, None) and list(kwargs) == ["ridge"]
    assert list(kwargs["ridge"][0]) == [1, 2, 3, 4] and kwargs["ridge"][1] == 0.5
    ez._create_object_mask(img, "blob", 1, None, None)
    assert calls[2][1] == {}


def test_too_small_planes_and_empty_images(meijering_on, monkeypatch):
    calls = []
    monkeypatch.setattr(ez, "_object_mask_device", lambda *a, **k: calls.append(a))
    for shape in ((1, 9), (9, 1), (1, 1)):
        with pytest.raises(ValueError, match=pmr.TOO_SMALL):
            ez._create_object_mask(np.ones(shape, np.float32), "projection", None, None, None)
    for shape in ((0, 5), (4, 0)):
        got = ez._create_object_mask(np.ones(shape, np.float32), "projection", None, None, None)
        assert got.shape == shape and got.dtype == np.int32
    assert not calls
    with pytest.raises(ValueError, match="must be a 2-D image"):
        ez._create_object_mask(np.ones((2, 3, 4), np.float32), "projection")


def run_create_projection_masks(ez_module, tmp_path):
    """create_object_masks on projections over a two-FOV cohort (80 x 72), as the notebook's first segmentation cell calls
    it; returns the masks' folder and the expected masks by FOV (used by the GPU test too, which hands them on to
    merge_masks_seq)."""
    from ark_analysis_amd import image_io
    rs = np.random.RandomState(8)
    img_dir = tmp_path / "image_data"
    images = {}
    for fov in ("fov0", "fov1"):
        (img_dir / fov).mkdir(parents=True)
        plane = pmr.lines(80, 72, rs) | pmr.discs(80, 72, rs, 2)
        images[fov] = (plane * rs.randint(4, 40, plane.shape)).astype(np.float32)
        image_io.write_image(str(img_dir / fov / "Iba1.tiff"), images[fov])
    masks_dir, log_dir = tmp_path / "masks", tmp_path / "logs"
    masks_dir.mkdir()
    log_dir.mkdir()
    ez_module.create_object_masks(str(img_dir), None, ["fov0", "fov1"], "microglia-projections", "Iba1", str(masks_dir),
                                  str(log_dir), object_shape_type="projection", sigma=1, thresh=None, hole_size=10, fov_dim=100,
                                  min_object_area=5, max_object_area=100000)
    expected = {}
    for fov in ("fov0", "fov1"):
        got = image_io.read_image(str(masks_dir / (fov + "_microglia-projections.tiff")))
        want = expected[fov] = pmr.create_projection_mask(images[fov], 1, None, 10, 100, 5, 100000)
        assert got.dtype == np.int32 and want.any() and np.array_equal(got, want), fov
    log = (log_dir / "microglia-projections_segmentation_log.txt").read_text().splitlines()
    assert log[5:] == ["object_shape_type: projection", "sigma: 1", "thresh: None", "hole_size: 10", "fov_dim: 100",
                       "min_object_area: 5", "max_object_area: 100000", "projection_filter: meijering"]
    return str(masks_dir), expected


def test_create_object_masks_files_and_log(meijering_on, tmp_path):
    run_create_projection_masks(meijering_on, tmp_path)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbol_and_refusals():
    from ark_analysis_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pxsom.h")).read()
    assert _capi.ABI_VERSION == 9 and "pxsom_ridge_sign" in _capi.SYMBOLS and re.search(r"\bpxsom_ridge_sign\(", header)
    lib = _capi.lib()
    assert lib.pxsom_abi_version() == 9
    # host arrays; the two "device" planes are never touched: every call below is refused before any HIP call
    fg, out = np.zeros(64 * 64, np.uint8), np.zeros(64 * 64, np.uint8)
    weights, radii, scales = np.full(35 * 8, 1 / 3.0), np.ones(8, np.int32), np.ones(8)

    def call(fg_p=fg.ctypes.data, h=8, w=8, ld=8, w_p=weights.ctypes.data, r_p=radii.ctypes.data, s_p=scales.ctypes.data, n=1,
             alpha=0.5, out_p=out.ctypes.data, ldo=8):
        rc = lib.pxsom_ridge_sign(fg_p, h, w, ld, w_p, r_p, s_p, n, alpha, out_p, ldo, None)
        return rc, lib.pxsom_last_error().decode() if rc else ""

    invalid, unsupported = -1, -2          # PXSOM_ERR_INVALID_ARG, PXSOM_ERR_UNSUPPORTED
    for kw in (dict(fg_p=None), dict(w_p=None), dict(r_p=None), dict(s_p=None), dict(out_p=None), dict(h=1), dict(w=1), dict(ld=7),
               dict(ldo=7), dict(n=0), dict(n=9), dict(alpha=float("nan")), dict(alpha=float("inf")),
               dict(out_p=fg.ctypes.data), dict(out_p=fg.ctypes.data + 63), dict(out_p=fg.ctypes.data + 16, ld=16, ldo=16)):
        rc, text = call(**kw)
        assert rc == invalid and text.startswith("pxsom_ridge_sign"), kw
    for bad_radius, code in ((0, invalid), (-3, invalid), (17, unsupported)):
        r = np.array([1, bad_radius], np.int32)
        rc, text = call(r_p=r.ctypes.data, n=2)
        assert rc == code and text.startswith("pxsom_ridge_sign"), bad_radius
    for bad_scale in (0.0, -1.0, float("nan"), float("inf")):
        s = np.array([1.0, bad_scale])
        rc, text = call(s_p=s.ctypes.data, n=2)
        assert rc == invalid and text.startswith("pxsom_ridge_sign"), bad_scale
    rc, text = call(h=46341, w=46341, ld=46341, ldo=46341, out_p=fg.ctypes.data + (1 << 40))
    assert rc == unsupported and text.startswith("pxsom_ridge_sign")


# ---- the generator reproduces the committed fixture -------------------------------------------------------------------------
def test_generator_reproduces_the_fixture(tmp_path):
    if not os.path.isdir("/root/reference/src/ark"):
        pytest.skip("the reference tree is not on this machine")
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_projection_masks.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    name = "g25_projection_masks.npz"
    new, old = np.load(tmp_path / name), np.load(os.path.join(GOLDEN, name))
    assert sorted(new.files) == sorted(old.files)
    for key in old.files:
        assert np.array_equal(new[key], old[key]), key
    assert os.path.getsize(os.path.join(GOLDEN, name)) <= 100 * 1024
