"""Projection object masks on the GPU (K22): som_device.ridge_sign equal, pixel for pixel, to the numpy statement of
tests/projection_mask_reference.py over the sizes at which the kernel's cases differ (np.gradient's one-sided rule at n = 2,
3, 4, planes smaller than every radius, one tile, tile seams, padded rows), flat planes, single pixels, the checkerboard,
the quadrant corner on a tile seam, lines, discs and noise, five scale lists and two alphas; then the whole chain of
_create_object_mask(..., "projection") under the switch against every g25 case, and the cohort function whose masks
merge_masks_seq consumes."""
import json

import numpy as np
import pytest
import torch

from tests import merge_masks_reference as mmr
from tests import projection_mask_reference as pmr
from tests import test_projection_masks as tpm

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (2, 70), (70, 2), (3, 5), (4, 4), (5, 7), (63, 65), (64, 64), (65, 129), (130, 67), (200, 230), (2, 300)]
EIGHT = [0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4]                     # radii 2, 4, ..., 16
SCALES = [[1], [4], [1, 2, 3, 4], [1.5, 2.5], EIGHT]
PADDED = (130, 67)                                           # this shape runs on row-padded fg and out planes


def patterns(h, w):
    """name -> uint8 plane.  A tile seam is row 63 / 64 and column 63 / 64; a plane without one takes its middle."""
    rs = np.random.RandomState(h * 1000 + w)
    sy, sx = (63 if h > 64 else h // 2), (64 if w > 64 else w // 2)
    cy, cx = (64 if h > 64 else h // 2), (64 if w > 64 else w // 2)
    return {"zeros": np.zeros((h, w), np.uint8), "ones": np.ones((h, w), np.uint8),
            "pixel_corner": pmr.single_pixel(h, w, 0, 0), "pixel_edge": pmr.single_pixel(h, w, h - 1, w // 2),
            "pixel_seam": pmr.single_pixel(h, w, sy, sx), "checkerboard": (np.indices((h, w)).sum(0) % 2 == 0).astype(np.uint8),
            "quadrant": pmr.quadrant(h, w, cy, cx), "lines": pmr.lines(h, w, rs), "discs": pmr.discs(h, w, rs),
            "noise": pmr.noise(h, w, rs)}


def on_device(plane, gpu, padded):
    if not padded:
        return torch.from_numpy(plane).to(gpu), None
    h, w = plane.shape
    buf = torch.zeros((h, w + 13), dtype=torch.uint8, device=gpu)
    buf[:, :w] = torch.from_numpy(plane).to(gpu)
    out = torch.full((h, w + 29), 7, dtype=torch.uint8, device=gpu)
    return buf[:, :w], out


@pytest.mark.parametrize("alpha", [0.5, 1 / 3], ids=["half", "third"])
@pytest.mark.parametrize("sigmas", SCALES, ids=["s1", "s4", "s1234", "s1.5_2.5", "eight"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ridge_sign_equals_the_statement(gpu, shape, sigmas, alpha):
    from ark_analysis_amd import som_device
    h, w = shape
    for name, plane in patterns(h, w).items():
        fg, out = on_device(plane, gpu, shape == PADDED)
        got = som_device.ridge_sign(fg, sigmas, alpha, out=None if out is None else out[:, :w])
        want = pmr.ridge_sign(plane, sigmas, alpha)
        assert got.dtype == torch.uint8 and got.shape == (h, w)
        diff = int((got.cpu().numpy() != want).sum())
        assert diff == 0, (name, diff)
        if name in ("zeros", "ones"):
            assert not want.any()
        if out is not None:
            assert got.data_ptr() == out.data_ptr() and bool((out[:, w:] == 7).all())


def test_ridge_sign_inputs(gpu):
    from ark_analysis_amd import _capi, som_device
    plane = pmr.lines(40, 50, np.random.RandomState(3))
    want = pmr.ridge_sign(plane)
    t = torch.from_numpy(plane).to(gpu)
    assert np.array_equal(som_device.ridge_sign(t).cpu().numpy(), want)                         # the reference's defaults
    assert np.array_equal(som_device.ridge_sign(t != 0, range(1, 5, 1), 0.5).cpu().numpy(), want)   # a bool plane
    assert np.array_equal(som_device.ridge_sign(t * 200).cpu().numpy(), want)                   # any non-zero byte is 1
    with pytest.raises(ValueError, match=pmr.TOO_SMALL):
        som_device.ridge_sign(t[:1])
    with pytest.raises(ValueError, match="1 to 8 scales"):
        som_device.ridge_sign(t, [1] * 9)
    with pytest.raises(ValueError, match="1 to 8 scales"):
        som_device.ridge_sign(t, [])
    for bad in ([0], [-1.0], [float("inf")], [1, float("nan")]):
        with pytest.raises(ValueError, match="finite sigmas > 0"):
            som_device.ridge_sign(t, bad)
    with pytest.raises(ValueError, match="finite alpha"):
        som_device.ridge_sign(t, [1], float("nan"))
    with pytest.raises(NotImplementedError, match="radius 17"):
        som_device.ridge_sign(t, [4.2])
    with pytest.raises(NotImplementedError, match="radius 0"):
        som_device.ridge_sign(t, [0.1])
    with pytest.raises(_capi.PxsomError, match="out overlaps fg"):
        som_device.ridge_sign(t, out=t)
    with pytest.raises(ValueError):
        som_device.ridge_sign(t.to(torch.int32))


@pytest.fixture(scope="module")
def g25():
    return np.load(tpm.GOLDEN + "/g25_projection_masks.npz")


def test_projection_chain_equals_every_fixture(gpu, g25, monkeypatch):
    from ark_analysis_amd import som_device
    from ark_analysis_amd.segmentation.ez_seg import ez_object_segmentation as ez
    for key in tpm.IMAGES:
        got = som_device.ridge_sign(torch.from_numpy(g25["img_" + key] > 0).to(gpu)).cpu().numpy()
        assert np.array_equal(got, g25["ridge_" + key]), key
    monkeypatch.setattr(ez, "PROJECTION_FILTER", "meijering")
    for c in json.loads(str(g25["cases"])):
        img, want = g25["img_" + c["image"]], g25["mask_" + c["name"]]
        got = ez._create_object_mask(img, "projection", c["sigma"], c["thresh"], c["hole_size"], c["fov_dim"],
                                     c["min_object_area"], c["max_object_area"])
        assert got.dtype == np.int32 and np.array_equal(got, want), c["name"]
    # ridge=None leaves the blob route as it was
    img = g25["img_mixed"]
    t = torch.from_numpy(img).to(gpu)
    blob = som_device.object_mask(t, 1, None, 15, 10, 100000)
    assert np.array_equal(blob.cpu().numpy(), som_device.object_mask(t, 1, None, 15, 10, 100000, None, ridge=None).cpu().numpy())
    assert np.array_equal(blob.cpu().numpy(), pmr.object_mask(img, 1, None, 15, 10, 100000))


def test_projection_cohort_and_merge(gpu, tmp_path, monkeypatch):
    """The notebook's projection cell, then merge_masks_seq on the masks it wrote."""
    from ark_analysis_amd import image_io
    from ark_analysis_amd.segmentation.ez_seg import ez_object_segmentation as ez
    from ark_analysis_amd.segmentation.ez_seg import merge_masks as mm
    monkeypatch.setattr(ez, "PROJECTION_FILTER", "meijering")
    masks_dir, expected = tpm.run_create_projection_masks(ez, tmp_path)
    rs = np.random.RandomState(19)
    cell_dir, merged_dir = tmp_path / "deepcell_output", tmp_path / "merged"
    cell_dir.mkdir()
    merged_dir.mkdir()
    cells = {}
    for fov in expected:
        cells[fov] = mmr.random_masks(rs, 80, 72, 60, 1)[1].astype(np.int32)
        image_io.write_image(str(cell_dir / (fov + "_whole_cell.tiff")), cells[fov])
    mm.merge_masks_seq(list(expected), ["microglia-projections"], masks_dir, str(cell_dir), "whole_cell", 10, 3, str(merged_dir),
                       str(tmp_path / "logs"))
    for fov, objects in expected.items():
        want_merged, want_cells = mmr.merge_masks(objects, cells[fov], 10, 3)
        got = image_io.read_image(str(merged_dir / (fov + "_microglia-projections_merged.tiff")))
        assert np.array_equal(got, want_merged) and want_merged.any(), fov
        got = image_io.read_image(str(merged_dir / (fov + "_final_whole_cell_remaining.tiff")))
        assert np.array_equal(got, want_cells), fov
