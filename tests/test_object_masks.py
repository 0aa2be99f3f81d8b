"""Object masks (K16) without a GPU: the numpy + scipy statement of tests/object_mask_reference.py against the g21 fixtures
(made by the reference's own _create_object_mask / create_cell_mask), and the Python mirrors with their one device entry
swapped for that statement -- signatures, error strings, get_block_size, the files they write, the ABI."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from ark_analysis_amd.segmentation.ez_seg import ez_object_segmentation  # noqa: F401  (the feature under test)
from tests import object_mask_reference as omr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def g21():
    return np.load(os.path.join(GOLDEN, "g21_object_masks.npz"))


@pytest.fixture(scope="module")
def g21_cells():
    return np.load(os.path.join(GOLDEN, "g21_cell_mask.npz"))


def cases(g21):
    return json.loads(str(g21["cases"]))


def g15_table():
    g15 = np.load(os.path.join(GOLDEN, "g15_saved_masks.npz"))
    table = pd.DataFrame({"fov": g15["table_fov"], "label": g15["table_label"], "cell_meta_cluster": g15["table_cluster"]})
    return g15, table


CELL_CASES = [("default", ["cd4", "tumor"], {}), ("small", ["cd8", "Bcell"], dict(sigma=0.6, min_object_area=12, max_hole_area=6)),
              ("none", ["no_such_type"], dict(sigma=1))]


@pytest.fixture
def statement_backend(monkeypatch):
    """The mirrors with their device entries swapped for the statement."""
    from ark_analysis_amd.segmentation.ez_seg import ez_object_segmentation as ez
    from ark_analysis_amd.utils import masking_utils as mu
    monkeypatch.setattr(ez, "_object_mask_device", omr.object_mask)
    monkeypatch.setattr(mu, "_isin_device", lambda seg, labels: np.isin(seg, labels).astype(np.int32))
    return ez, mu


# ---- the statement against the fixtures -----------------------------------------------------------------------------------
def test_statement_equals_the_fixtures(g21):
    kinds = set()
    for c in cases(g21):
        got = omr.create_object_mask(g21["img_" + c["image"]], c["sigma"], c["thresh"], c["hole_size"], c["fov_dim"],
                                     c["min_object_area"], c["max_object_area"])
        assert got.dtype == np.int32 and np.array_equal(got, g21["mask_" + c["name"]]), c["name"]
        kinds.add((type(c["thresh"]).__name__, type(c["hole_size"]).__name__))
    assert len(kinds) == 9          # every threshold kind x every hole kind


def test_statement_cell_masks_equal_the_fixtures(g21_cells):
    g15, table = g15_table()
    for fov in ("fov0", "fov1"):
        for name, types_, kw in CELL_CASES:
            rows = table[(table["fov"] == fov) & table["cell_meta_cluster"].isin(types_)]
            got = omr.cell_mask(g15["seg_" + fov], rows["label"].values, **kw)
            assert np.array_equal(got, g21_cells[name + "_" + fov]), (name, fov)
    assert g21_cells["small_fov0"].any() and not g21_cells["small_fov0"].all()


def test_statement_numbering_fill_and_keep():
    mask = np.array([[0, 0, 1, 0, 1],
                     [1, 0, 1, 0, 0],
                     [1, 1, 1, 0, 1],
                     [0, 0, 0, 1, 0]], dtype=np.uint8)
    labels, n, areas = omr.label_components(mask, 1)
    assert n == 4 and labels[0, 2] == 1 and labels[0, 4] == 2 and labels[2, 4] == 3 and labels[3, 3] == 4
    assert areas.tolist() == [11, 6, 1, 1, 1]
    labels8, n8, _ = omr.label_components(mask, 2)
    assert n8 == 2 and labels8[3, 3] == 1 and labels8[0, 4] == 2
    ring = np.ones((5, 5), np.uint8)
    ring[1:3, 1:3] = 0                      # a hole of 4 pixels
    assert omr.fill_holes(ring, 4)[1, 1] == 0 and omr.fill_holes(ring, 5)[1, 1] == 1      # strict <
    edge = np.ones((4, 4), np.uint8)
    edge[0, 0] = 0                          # a hole that touches the border is a hole like any other
    assert omr.fill_holes(edge, 2).all()
    assert omr.keep_by_area(labels, areas, 1, 1).tolist() == np.where(np.isin(labels, [2, 3, 4]), labels, 0).tolist()


# ---- the mirrors ----------------------------------------------------------------------------------------------------------
def test_signatures_equal_the_reference(g21):
    from ark_analysis_amd.segmentation.ez_seg import ez_object_segmentation as ez
    from ark_analysis_amd.utils import masking_utils as mu
    recorded = json.loads(str(g21["signatures"]))
    assert set(recorded) == {"_create_object_mask", "create_object_masks", "get_block_size", "generate_signal_masks",
                             "create_cell_mask", "generate_cell_masks"}
    for name, params in recorded.items():
        fn = getattr(ez, name, None) or getattr(mu, name)
        got = [[p.name, repr(p.default)] for p in inspect.signature(fn).parameters.values()]
        assert got == params, name


def test_mirror_equals_the_fixtures(statement_backend, g21, g21_cells):
    ez, mu = statement_backend
    for c in cases(g21):
        got = ez._create_object_mask(g21["img_" + c["image"]], "blob", c["sigma"], c["thresh"], c["hole_size"], c["fov_dim"],
                                     c["min_object_area"], c["max_object_area"])
        assert got.dtype == np.int32 and np.array_equal(got, g21["mask_" + c["name"]]), c["name"]
    g15, table = g15_table()
    for fov in ("fov0", "fov1"):
        for name, types_, kw in CELL_CASES:
            got = mu.create_cell_mask(g15["seg_" + fov], table, fov, types_, **kw)
            assert got.dtype == np.int32 and np.array_equal(got, g21_cells[name + "_" + fov]), (name, fov)


def test_block_sizes(g21):
    from ark_analysis_amd.segmentation.ez_seg.ez_object_segmentation import get_block_size
    blocks = json.loads(str(g21["block_sizes"]))
    assert len(blocks) == 40
    for block_type, fov_dim, img_shape, want in blocks:
        assert get_block_size(block_type, fov_dim, img_shape) == want
        assert omr.get_block_size(block_type, fov_dim, img_shape) == want
    assert get_block_size("local_thresh", 400, 2048) == 51 and get_block_size("small_holes", 400, 2048) == 1263
    with pytest.raises(ValueError, match="Not all values given in list block_type were found in list block_types"):
        get_block_size("median", 400, 2048)


def test_errors(statement_backend):
    ez, _ = statement_backend
    img = np.ones((8, 8), np.float32)
    with pytest.raises(ValueError, match=re.escape(
            "Invalid `threshold` value: 0.5. Must be either `auto`, `None` or an integer.")):
        ez._create_object_mask(img, thresh=0.5)
    with pytest.raises(ValueError, match=re.escape(
            "Invalid `hole_size` value: big. Must be either `auto`, `None` or an integer.")):
        ez._create_object_mask(img, hole_size="big")
    with pytest.raises(ValueError, match="Not all values given in list object_shape_type were found in list object_shape_options"):
        ez._create_object_mask(img, object_shape_type="star")
    calls = []
    ez._object_mask_device = lambda *a, **k: calls.append(a)        # (monkeypatch restores the attribute)
    with pytest.raises(NotImplementedError, match="projection"):
        ez._create_object_mask(img, object_shape_type="projection")
    with pytest.raises(NotImplementedError, match="radius limit"):
        ez._create_object_mask(img, sigma=17)
    with pytest.raises(NotImplementedError, match="radius limit"):
        ez._create_object_mask(np.ones((4096, 8), np.float32), thresh="auto", fov_dim=10)   # block 4097: sigma 682
    assert not calls


def _cohort(tmp_path, rs, fovs, channels, size=64):
    img_dir = tmp_path / "image_data"
    images = {}
    for fov in fovs:
        (img_dir / fov).mkdir(parents=True)
        for ch in channels:
            from ark_analysis_amd import image_io
            img = (rs.rand(size, size) < 0.02).astype(np.float32) * rs.uniform(5, 50, (size, size)).astype(np.float32)
            img = np.round(omr.blur(img, 2.0, "nearest") * 8).astype(np.float32)
            image_io.write_image(str(img_dir / fov / (ch + ".tiff")), img)
            images[fov, ch] = img
    return str(img_dir), images


def run_create_object_masks(ez, tmp_path):
    """create_object_masks on a two-FOV cohort; returns what the test compares (used by the GPU test too)."""
    from ark_analysis_amd import image_io
    rs = np.random.RandomState(5)
    fovs = ["fov1", "fov0"]
    img_dir, images = _cohort(tmp_path, rs, fovs, ["CD3", "HH3"])
    masks_dir, log_dir = tmp_path / "masks", tmp_path / "logs"
    masks_dir.mkdir()
    log_dir.mkdir()
    ez.create_object_masks(img_dir, None, fovs, "plaques", "HH3", str(masks_dir), str(log_dir), sigma=1, thresh=40, hole_size=8,
                           fov_dim=100, min_object_area=6, max_object_area=900)
    assert sorted(os.listdir(masks_dir)) == ["fov0_plaques.tiff", "fov1_plaques.tiff"]
    for fov in fovs:
        got = image_io.read_image(str(masks_dir / (fov + "_plaques.tiff")))
        want = omr.create_object_mask(images[fov, "HH3"], 1, 40, 8, 100, 6, 900)
        assert got.dtype == np.int32 and want.any() and np.array_equal(got, want), fov
    log = (log_dir / "plaques_segmentation_log.txt").read_text().splitlines()
    assert log[0] == "image_data_dir: " + img_dir and log[1] == "fov_list: ['fov1', 'fov0']"
    assert log[2:5] == ["mask_name: plaques", "channel_to_segment: HH3", "masks_dir: " + str(masks_dir)]
    assert log[5:] == ["object_shape_type: blob", "sigma: 1", "thresh: 40", "hole_size: 8", "fov_dim: 100",
                       "min_object_area: 6", "max_object_area: 900"]


def run_generate_signal_masks(mu, tmp_path):
    from ark_analysis_amd import image_io
    rs = np.random.RandomState(6)
    fovs = ["fov0", "fov1"]
    img_dir, images = _cohort(tmp_path, rs, fovs, ["CD3", "CD4", "HH3"])
    mask_dir = tmp_path / "signal_masks"
    mask_dir.mkdir()
    mu.generate_signal_masks(img_dir, str(mask_dir), ["CD3", "HH3"], "signal", intensity_thresh_perc=30, sigma=1,
                             min_object_area=20, max_hole_area=10)
    for fov in fovs:
        got = image_io.read_image(str(mask_dir / fov / "signal.tiff"))
        total = images[fov, "CD3"] + images[fov, "HH3"]
        want = omr.create_object_mask(total, 1, 30, 10, 400, 20, 64 * 64)
        assert want.any() and np.array_equal(got, want), fov
    with pytest.raises(ValueError, match="Not all values given in list input_channels were found in list all_channels"):
        mu.generate_signal_masks(img_dir, str(mask_dir), ["CD8"], "signal")


def run_generate_cell_masks(mu, tmp_path):
    from ark_analysis_amd import image_io
    rs = np.random.RandomState(7)
    seg_dir, mask_dir = tmp_path / "seg", tmp_path / "cell_masks"
    seg_dir.mkdir()
    rows, segs = [], {}
    for fov in ("fov0", "fov1"):
        seg = np.kron(rs.permutation(64).reshape(8, 8) + 1, np.ones((8, 8), dtype=np.int64)).astype(np.int32)
        seg[rs.rand(64, 64) < 0.1] = 0
        image_io.write_image(str(seg_dir / (fov + "_whole_cell.tiff")), seg)
        segs[fov] = seg
        rows += [(fov, lab, ["tumor", "cd4", "cd8"][lab % 3]) for lab in range(1, 65)]
    table = pd.DataFrame(rows, columns=["fov", "label", "cell_meta_cluster"])
    mu.generate_cell_masks(str(seg_dir), str(mask_dir), table, ["tumor"], "tumor_mask", sigma=0.5, min_object_area=70,
                           max_hole_area=4)
    for fov in ("fov0", "fov1"):
        got = image_io.read_image(str(mask_dir / fov / "tumor_mask.tiff"))
        want = omr.cell_mask(segs[fov], [lab for lab in range(1, 65) if lab % 3 == 0], 0.5, 70, 4)
        assert want.any() and not want.all() and np.array_equal(got.astype(np.int32), want), fov


def test_create_object_masks_files(statement_backend, tmp_path, capsys):
    run_create_object_masks(statement_backend[0], tmp_path)
    out = capsys.readouterr().out
    assert out.endswith("ez masks built and saved\n") and "Values saved to " in out


def test_generate_signal_masks_files(statement_backend, tmp_path):
    run_generate_signal_masks(statement_backend[1], tmp_path)


def test_generate_cell_masks_files(statement_backend, tmp_path):
    run_generate_cell_masks(statement_backend[1], tmp_path)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols():
    from ark_analysis_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pxsom.h")).read()
    assert _capi.ABI_VERSION == 9 and re.search(r"#define PXSOM_ABI_VERSION 9\b", header)
    for name in ("pxsom_label_components_workspace_bytes", "pxsom_label_components", "pxsom_components_select",
                 "pxsom_gaussian_blur_plane_mode", "pxsom_binarize_plane"):
        assert name in _capi.SYMBOLS and re.search(r"\b%s\(" % name, header), name
    lib = _capi.lib()       # resolves every symbol; no device needed for the host-side checks below
    assert lib.pxsom_abi_version() == 9
    assert lib.pxsom_label_components_workspace_bytes(130, 195) >= 130 * 195 * 4
    assert lib.pxsom_label_components_workspace_bytes(0, 5) == 0
    assert lib.pxsom_label_components(None, 4, 4, 4, 1, 0, None, 4, None, None, 9, None, 0, None) == -1
    assert lib.pxsom_components_select(2, None, 0, None, 4, None, 1, 4, 4, 0, 0, None, 4, None) == -1
    assert lib.pxsom_gaussian_blur_plane_mode(None, None, None, 4, 4, 7, None, 1, 0, None) == -1
    assert lib.pxsom_binarize_plane(None, 7, 4, 4, 0, 0.0, None, None, 4, None) == -1


# ---- the generator reproduces the committed fixtures ------------------------------------------------------------------------
def test_generator_reproduces_the_fixtures(tmp_path):
    if not os.path.isdir("/root/reference/src/ark"):
        pytest.skip("the reference tree is not on this machine")
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_object_masks.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    for name in ("g21_object_masks.npz", "g21_cell_mask.npz"):
        new, old = np.load(tmp_path / name), np.load(os.path.join(GOLDEN, name))
        assert sorted(new.files) == sorted(old.files)
        for key in old.files:
            assert np.array_equal(new[key], old[key]), (name, key)
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 100 * 1024
