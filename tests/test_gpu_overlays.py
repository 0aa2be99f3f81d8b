"""K29 on the device: pxsom_overlay_rgb, pxsom_percentile_f32_listq, the channel sums of generate_deepcell_input and
pxsom_colorize against the numpy statement (tests/overlay_reference.py).  Every result is array_equal to the statement:
no tolerance."""
import os

import numpy as np
import pytest
import torch

from tests import overlay_reference as ovr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLANE_DTYPES = (np.uint8, np.int16, np.uint16, np.int32, np.float32)
LABEL_DTYPES = (np.uint8, np.int32, np.int64)
# 1-pixel and 1-line images; one below, at and one above the wave's 4 rows and 256 columns; the block's 16 rows; widths
# that are no multiple of 4 (the ragged RGB tail, rows that start off a 4-byte boundary); an odd mid-size plane
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 255), (4, 256), (5, 257), (17, 258), (16, 513), (67, 131))


def _up(a, gpu, shift=0):
    """The array in HBM, contiguous; with ``shift`` that many elements into its allocation (a base off 16 bytes)."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    if shift:
        flat = torch.empty(t.numel() + shift, dtype=t.dtype, device=gpu)
        flat[shift:] = t.reshape(-1)
        t = flat[shift:].view(t.shape)
    return t


def _cells(h, w, seed, dtype, big=False):
    return ovr.cells(h, w, seed, dtype, big=big and np.dtype(dtype).itemsize >= 4)


def _check(gpu, planes, seg, alt=None, shift=0):
    """overlay_rgb with and without the border plane against the statement; with ``shift`` every input plane (an
    ``[H, W, c]`` image as its c planes) starts that many elements into its allocation."""
    from ark_analysis_amd import som_device as sd
    want = ovr.overlay(planes, seg, alt)
    dev_planes = [_up(planes[..., i], gpu, shift) for i in range(planes.shape[2])] if shift else _up(planes, gpu)
    seg_d, alt_d = _up(seg, gpu, shift), None if alt is None else _up(alt, gpu, shift)
    got, borders = sd.overlay_rgb(dev_planes, seg_d, alt_d, want_borders=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == seg.shape + (3,)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(borders.cpu().numpy(), ovr.borders(seg))
    assert np.array_equal(sd.overlay_rgb(dev_planes, seg_d, alt_d).cpu().numpy(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_overlay_shapes(gpu, shape):
    h, w = shape
    for n, pdt in enumerate(PLANE_DTYPES):
        seed = 1000 * h + 10 * w + n
        planes = np.stack([ovr.signal(h, w, seed + i, pdt) for i in range(1 + n % 3)], axis=-1)
        if h * w < 50:                      # (a few pixels, all negative, would be the refusal of test_overlay_refusals)
            planes = np.abs(planes)
        seg = _cells(h, w, seed, LABEL_DTYPES[n % 3], big=True)
        alt = _cells(h, w, seed + 7, LABEL_DTYPES[(n + 1) % 3]) if n % 2 == 0 else None
        _check(gpu, planes, seg, alt)


def test_overlay_unaligned_base(gpu):
    """Widths that are a multiple of 4, so that only the base pointer decides between the 4-element and the element
    loads: every plane and label plane one and three elements off its allocation."""
    h, w = 5, 256
    for n, pdt in enumerate(PLANE_DTYPES):
        planes = np.stack([ovr.signal(h, w, 300 + n + i, pdt) for i in range(2)], axis=-1)
        seg = _cells(h, w, 310 + n, LABEL_DTYPES[n % 3], big=True)
        alt = _cells(h, w, 320 + n, LABEL_DTYPES[(n + 1) % 3])
        for shift in (1, 3):
            assert _up(seg, gpu, shift).data_ptr() % (4 * seg.dtype.itemsize) != 0
            _check(gpu, planes, seg, alt, shift=shift)


@pytest.mark.parametrize("ldt", LABEL_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("pdt", PLANE_DTYPES, ids=lambda d: np.dtype(d).name)
def test_overlay_dtypes(gpu, pdt, ldt):
    """Every plane dtype x label dtype; 1, 2 and 3 channels and the 2-D form; the alternate segmentation in another dtype,
    present and absent; int32 / int64 labels above 2^15."""
    h, w = 21, 261
    seg = _cells(h, w, 5, ldt, big=True)
    if np.dtype(ldt).itemsize >= 4:
        assert seg.max() > 2 ** 15
    alt = _cells(h, w, 6, np.int16 if ldt != np.int16 else np.uint16)
    planes = np.stack([ovr.signal(h, w, 50 + i, pdt) for i in range(3)], axis=-1)
    _check(gpu, planes[..., 0], seg, alt)
    _check(gpu, planes[..., :1], seg, None)
    _check(gpu, planes[..., :2], seg, alt)
    _check(gpu, planes, seg, None)
    _check(gpu, planes, seg, _cells(h, w, 8, np.uint16))


@pytest.mark.parametrize("pdt", PLANE_DTYPES, ids=lambda d: np.dtype(d).name)
def test_overlay_plane_kinds(gpu, pdt):
    """An all-zero plane (mode 0), a plane with one positive value and one whose positive pixels are all equal (lo == hi:
    mode 2), negative values and values above the 95th percentile (mode 1), side by side in one image."""
    h, w = 19, 67
    seg = _cells(h, w, 11, np.int32)
    zero, one, equal, plain = (ovr.signal(h, w, 70 + i, pdt, kind) for i, kind in enumerate(("zero", "one", "equal", "plain")))
    lo, hi = ovr.percentiles_positive(plain)
    assert (plain > hi).any() and (np.dtype(pdt).kind == "u" or (plain < 0).any())
    for trio in ((zero, one, plain), (equal, zero, zero), (plain, equal, one), (zero, zero, zero)):
        _check(gpu, np.stack(trio, axis=-1), seg, _cells(h, w, 12, np.uint8))
    _check(gpu, one, seg)


def test_overlay_float32_top_of_range(gpu):
    """A float32 plane whose pixels at and above the 95th percentile come out as 254: the quotient falls one ulp short
    of 1 (tests/test_overlays.py shows the plane)."""
    plane = ovr.signal(16, 16, 4, np.float32)
    lo, hi = ovr.percentiles_positive(plane)
    assert ovr.rescale_intensity_uint8(plane, lo, hi)[plane >= hi].max() == 254
    _check(gpu, plane, _cells(16, 16, 4, np.int32))


def test_borders_only_and_labels(gpu):
    """Borders-only calls in every label dtype the device reads; cells touching the image edge, single-pixel cells and
    two cells adjacent without background are what ovr.cells builds."""
    from ark_analysis_amd import som_device as sd
    for n, ldt in enumerate((np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64)):
        for h, w in ((1, 1), (5, 257), (33, 300)):
            seg = _cells(h, w, 20 + n, ldt, big=True)
            got = sd.overlay_rgb(None, _up(seg, gpu))
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ovr.borders(seg)), (ldt, h, w)
    seg = np.zeros((6, 9), dtype=np.int32)
    seg[0:3, 0:4], seg[0:3, 4:9], seg[4, 4] = 1, 2, 3         # at the edge, adjacent without background, a single pixel
    want = ovr.borders(seg)
    assert want[0, 0] == 0 and want[0, 3] == 255 and want[0, 4] == 255 and want[4, 4] == 255 and want[2, 0] == 255
    assert np.array_equal(sd.overlay_rgb(None, _up(seg, gpu)).cpu().numpy(), want)


def test_overlay_refusals(gpu):
    from ark_analysis_amd import som_device as sd
    seg = _up(_cells(8, 9, 1, np.int32), gpu)
    negative = _up(-np.ones((8, 9), dtype=np.float32), gpu)
    with pytest.raises(ValueError, match="channel dsDNA has a non-zero maximum but no positive pixel"):
        sd.overlay_rgb([negative], seg, channel_names=["dsDNA"])
    with pytest.raises(ValueError, match="max 3 channels"):
        sd.overlay_rgb(torch.zeros((8, 9, 4), dtype=torch.uint8, device=gpu), seg)
    with pytest.raises(ValueError):
        sd.overlay_rgb(torch.zeros((8, 9), dtype=torch.float64, device=gpu), seg)
    with pytest.raises(ValueError):
        sd.overlay_rgb(torch.zeros((8, 8), dtype=torch.uint8, device=gpu), seg)


# ---- percentiles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdt", PLANE_DTYPES, ids=lambda d: np.dtype(d).name)
def test_percentiles_positive(gpu, pdt):
    """The float32 list-q entry and the integer route against np.percentile: 1, 2, 3 and about 1 000 kept values among
    zeros (and negative values where the dtype has them), and a plane whose kept values are all equal."""
    from ark_analysis_amd import som_device as sd
    rs = np.random.RandomState(40)
    for kept in (1, 2, 3, 1000):
        for rep in range(3):
            total = kept + 30 + kept % 2
            if np.dtype(pdt).kind == "f":
                values = (rs.gamma(2.0, 3.0, size=kept) * 10.0 ** rs.randint(-3, 4)).astype(pdt) + np.float32(1e-6)
            else:
                values = rs.randint(1, min(np.iinfo(pdt).max, 5000), size=kept).astype(pdt)
            plane = np.zeros(total, dtype=pdt)
            plane[rs.permutation(total)[:kept]] = values
            if np.dtype(pdt).kind != "u":
                free = np.flatnonzero(plane == 0)[:7]
                plane[free] = -3
            plane = plane.reshape(1, total) if rep % 2 else plane.reshape(total // 2, 2)
            assert (plane > 0).sum() == kept
            got = sd.percentiles_positive(_up(plane, gpu), (5, 95))
            assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), ovr.percentiles_positive(plane)), (kept, rep)
    equal = ovr.signal(9, 11, 3, pdt, "equal")
    assert np.array_equal(sd.percentiles_positive(_up(equal, gpu)).cpu().numpy(), np.array([9.0, 9.0]))
    other = sd.percentiles_positive(_up(ovr.signal(13, 17, 5, pdt), gpu), (0, 50, 100, 37.5))
    assert np.array_equal(other.cpu().numpy(), ovr.percentiles_positive(ovr.signal(13, 17, 5, pdt), (0, 50, 100, 37.5)))
    assert torch.isnan(sd.percentiles_positive(_up(np.zeros((3, 3), dtype=pdt), gpu))).all()


# ---- the public functions on the device ------------------------------------------------------------------------------
def test_overlay_image_and_saved_files_on_the_device(gpu, tmp_path):
    from ark_analysis_amd import image_io
    from ark_analysis_amd.segmentation import segmentation_utils
    from ark_analysis_amd.utils import plot_utils
    with np.load(os.path.join(HERE, "golden", "g32_overlays.npz")) as g:
        for name in (str(n) for n in g["overlay_names"]):
            p = "o_%s_" % name
            chans = [str(c) for c in g[p + "chans"]]
            folder = tmp_path / name
            folder.mkdir()
            image_io.write_stack(str(folder / "fov0.tiff"), g[p + "pages"])
            image_io.write_image(str(folder / "fov0_whole_cell.tiff"), g[p + "cell"])
            image_io.write_image(str(folder / "fov0_nuclear.tiff"), g[p + "nuc"])
            alt = g[p + "alt"] if p + "alt" in g.files else None
            got = plot_utils.create_overlay("fov0", str(folder), str(folder), chans, str(g[p + "comp"]), alternate_segmentation=alt)
            assert np.array_equal(got, g[p + "overlay"]), name
            segmentation_utils.save_segmentation_labels(str(folder), str(folder), str(folder), ["fov0"], channels=chans)
            assert np.array_equal(image_io.read_image(str(folder / "fov0_segmentation_borders.tiff")), g[p + "borders"])
            assert np.array_equal(image_io.read_image(str(folder / "_".join(["fov0", *chans, "overlay.tiff"]))),
                                  g[p + "saved_overlay"])


def test_generate_deepcell_input_on_the_device(gpu, tmp_path):
    """int16 and uint16 sums that wrap, float32 sums of 1, 2, 7 and 9 channels (numpy's pairwise order from 8 on)."""
    from ark_analysis_amd import image_io
    from ark_analysis_amd.utils import deepcell_service_utils
    with np.load(os.path.join(HERE, "golden", "g32_overlays.npz")) as g:
        names = [str(n) for n in g["deepcell_names"]]
        assert {"i16_wrap", "f32_1", "f32_2", "f32_7", "f32_9"} <= set(names)
        for name in names:
            p = "d_%s_" % name
            stack = g[p + "stack"]
            chans = ["chan%d" % i for i in range(stack.shape[2])]
            tiff_dir, data_dir = tmp_path / name / "tiffs", tmp_path / name / "input"
            (tiff_dir / "fov0" / "TIFs").mkdir(parents=True)
            data_dir.mkdir()
            for i, ch in enumerate(chans):
                image_io.write_image(str(tiff_dir / "fov0" / "TIFs" / (ch + ".tiff")), stack[:, :, i])
            nuc, mem = [int(i) for i in g[p + "nuc"]], [int(i) for i in g[p + "mem"]]
            deepcell_service_utils.generate_deepcell_input(str(data_dir), str(tiff_dir), [chans[i] for i in nuc],
                                                           [chans[i] for i in mem], ["fov0"])
            got = image_io.read_stack(str(data_dir / "fov0.tiff"))
            assert got.dtype == stack.dtype and np.array_equal(got, ovr.deepcell_pages(stack, nuc, mem)), name
            assert np.array_equal(got, g[p + "pages"]), name


# ---- the colour gather -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", (3, 4))
@pytest.mark.parametrize("mdt", (np.uint8, np.int16, np.uint16, np.int32), ids=lambda d: np.dtype(d).name)
def test_colorize(gpu, mdt, ncol):
    from ark_analysis_amd import som_device as sd
    rs = np.random.RandomState(60 + ncol)
    colors = rs.rand(23, ncol)
    table = ovr.color_table(colors)
    table_d = _up(table, gpu)
    for h, w in ((1, 1), (2, 3), (3, 5), (4, 257), (1, 1030)):
        mask = rs.randint(0, 23, size=(h, w)).astype(mdt)
        got, status = sd.colorize(_up(mask, gpu), table_d)
        assert status == 0 and got.dtype == torch.uint8 and tuple(got.shape) == (h, w, ncol)
        assert np.array_equal(got.cpu().numpy(), ovr.colored_mask(mask, colors)), (h, w)
    bad_values = (23, 200) if np.dtype(mdt).kind == "u" else (23, -1)
    for value in bad_values:
        for h, w in ((3, 5), (4, 257)):
            mask = rs.randint(0, 23, size=(h, w)).astype(mdt)
            mask[h - 1, w - 1] = value
            got, status = sd.colorize(_up(mask, gpu), table_d)
            assert status == sd.COLORIZE_BAD_INDEX
            keep = np.ones((h, w), dtype=bool)
            keep[h - 1, w - 1] = False
            assert np.array_equal(got.cpu().numpy()[keep], table[mask[keep]]) and not got.cpu().numpy()[h - 1, w - 1].any()


def test_save_colored_masks_on_the_device(gpu, tmp_path):
    from ark_analysis_amd import image_io
    from ark_analysis_amd.utils import plot_utils
    with np.load(os.path.join(HERE, "golden", "g32_overlays.npz")) as g:
        path = str(tmp_path / "names.csv")
        with open(path, "w") as f:
            f.write(str(g["c_names_text"]))
        colors = {int(k): tuple(float(x) for x in v) for k, v in zip(g["c_color_keys"], g["c_color_values"])}
        for fov in ("fov0", "fov1"):
            image_io.write_image(str(tmp_path / (fov + "_cell_mask.tiff")), g["c_mask_" + fov])
        plot_utils.save_colored_masks(["fov0", "fov1"], str(tmp_path), str(tmp_path / "colored"), path, colors, "cell")
        for fov in ("fov0", "fov1"):
            got = image_io.read_image(str(tmp_path / "colored" / (fov + "_cell_mask_colored.tiff")))
            assert np.array_equal(got, g["c_colored_" + fov])
        bad = g["c_mask_fov0"].copy()
        bad[0, 0] = -1
        with pytest.raises(IndexError):
            plot_utils.colored_mask(bad, g["c_mc_colors"])
