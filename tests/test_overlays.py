"""K29 on the CPU: the numpy statement (tests/overlay_reference.py) against the outputs of the reference's own functions
(tests/golden/g32_overlays.npz), what each recalled detail changes, the public functions with their device entries swapped
for the statement, the TIFF stack and RGB files, every refusal, and the ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from tests import overlay_reference as ovr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "g32_overlays.npz")
PAGE_NAMES = ["nuclear_channel", "membrane_channel"]
NEW_SYMBOLS = ("pxsom_percentile_f32_listq", "pxsom_overlay_rgb", "pxsom_colorize")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def _overlay_case(g, name):
    p = "o_%s_" % name
    chans = [str(c) for c in g[p + "chans"]]
    comp = str(g[p + "comp"])
    tif = np.stack([g[p + "pages"][PAGE_NAMES.index(c)] for c in chans], axis=-1)
    return p, chans, comp, tif, g[p + ("cell" if comp == "whole_cell" else "nuc")], g.get(p + "alt")


# ---- the statement equals the reference's outputs --------------------------------------------------------------------
def test_statement_equals_the_reference_overlays(golden):
    names = [str(n) for n in golden["overlay_names"]]
    assert len(names) == 6
    for name in names:
        p, chans, comp, tif, seg, alt = _overlay_case(golden, name)
        assert np.array_equal(ovr.overlay(tif, seg, alt), golden[p + "overlay"]), name
        assert np.array_equal(ovr.borders(golden[p + "cell"]), golden[p + "borders"]), name
        assert np.array_equal(ovr.overlay(tif, golden[p + "cell"]), golden[p + "saved_overlay"]), name
        assert set(np.unique(golden[p + "borders"])) <= {0, 255} and golden[p + "borders"].dtype == np.uint8
    assert np.array_equal(ovr.borders(golden["b_cell"]), golden["b_borders"])
    # the fixture meets both compositing colours, a skipped channel and the lo == hi branch
    p = "o_f32_both_alt_"
    red = (golden[p + "overlay"] == (255, 0, 0)).all(axis=2)
    assert red.any() and np.array_equal(red, ovr.inner_boundaries(golden[p + "alt"]))
    assert not golden["o_u8_zero_and_one_pages"][0].any()
    lo, hi = ovr.percentiles_positive(golden["o_f32_one_pages"][0])
    assert lo == hi == 300.5


def test_statement_equals_the_reference_sums_and_colours(golden):
    for name in (str(n) for n in golden["deepcell_names"]):
        p = "d_%s_" % name
        got = ovr.deepcell_pages(golden[p + "stack"], golden[p + "nuc"], golden[p + "mem"])
        assert got.dtype == golden[p + "pages"].dtype and np.array_equal(got, golden[p + "pages"]), name
    wrapped = golden["d_i16_wrap_stack"][:, :, [0, 1, 2]].astype(np.int64).sum(axis=2)
    assert (wrapped > 32767).all() and np.array_equal(wrapped.astype(np.int16), golden["d_i16_wrap_pages"][0])
    assert not golden["d_u16_wrap_pages"][1].any() and not golden["d_f32_2_pages"][0].any()      # an empty list: zeros
    for fov in ("fov0", "fov1"):
        mask = golden["c_mask_" + fov]
        assert np.array_equal(ovr.colored_mask(mask, golden["c_mc_colors"]), golden["c_colored_" + fov])
        assert np.array_equal(ovr.color_table(golden["c_mc_colors"])[mask], golden["c_colored_" + fov])


def test_list_q_percentile_arithmetic():
    """np.percentile with a list q on a float32 vector is the mix of pxsom_percentile_f32_listq, not float32 arithmetic
    throughout and not float64 values throughout."""
    rs = np.random.RandomState(29)
    differs32 = differs64 = 0
    for n in (1, 2, 3, 4, 5, 17, 100, 1001):
        for _ in range(40):
            v = (rs.gamma(2.0, 3.0, size=n) * 10.0 ** rs.randint(-3, 4)).astype(np.float32)
            want = np.percentile(v, [5, 95])
            assert want.dtype == np.float64 and np.array_equal(ovr.percentile_listq_f32(v, [5, 95]), want)
            differs32 += not np.array_equal(np.array([np.percentile(v, 5), np.percentile(v, 95)], dtype=np.float64), want)
            differs64 += not np.array_equal(np.percentile(v.astype(np.float64), [5, 95]), want)
    assert differs32 > 0 and differs64 > 0


# ---- what each recalled detail changes -------------------------------------------------------------------------------
def test_every_recalled_switch_changes_a_result(golden):
    assert set(ovr.RECALLED_OVERLAY) == {"clip_then_scale", "equal_range_branch", "truncating_cast"}
    assert all(ovr.RECALLED_OVERLAY.values())
    _, _, _, tif, seg, alt = _overlay_case(golden, "u16_both")
    assert not np.array_equal(ovr.overlay(tif, seg, alt, {"truncating_cast": False}), ovr.overlay(tif, seg, alt))
    _, _, _, tif, seg, alt = _overlay_case(golden, "f32_one")
    assert not np.array_equal(ovr.overlay(tif, seg, alt, {"equal_range_branch": False}), ovr.overlay(tif, seg, alt))
    # clip-then-scale against scale-then-clip.  In binary64 (every integer plane) the two agree on every pixel: the clip is
    # monotone, a pixel at or above hi gives (hi - lo) / (hi - lo) = 1 exactly, one at or below lo gives 0.  In binary32
    # they differ at the top: clip(x) - float32(lo) is rounded on its own, the divisor float32(hi - lo) is rounded from
    # the binary64 difference, and the quotient may fall one ulp short of 1 -- 254 where scaling first and clipping to
    # 255 gives 255.
    for name in ("u16_both", "i16_one", "i32_equal", "u8_zero_and_one"):
        _, _, _, tif, seg, alt = _overlay_case(golden, name)
        assert np.array_equal(ovr.overlay(tif, seg, alt, {"clip_then_scale": False}), ovr.overlay(tif, seg, alt)), name
    plane = ovr.signal(16, 16, 4, np.float32)
    lo, hi = ovr.percentiles_positive(plane)
    first, after = ovr.rescale_intensity_uint8(plane, lo, hi), ovr.rescale_intensity_uint8(plane, lo, hi, {"clip_then_scale": False})
    assert first[plane >= hi].max() == 254 and after[plane >= hi].min() == 255
    assert np.array_equal(first[plane < hi], after[plane < hi])


# ---- the public functions over the statement -------------------------------------------------------------------------
@pytest.fixture
def statement(monkeypatch):
    """The device entries of the three modules swapped for the numpy statement; counts the calls."""
    from ark_analysis_amd.utils import deepcell_service_utils, plot_utils
    calls = {"overlay": 0, "colorize": 0, "sums": 0}

    def overlay(channels, seg, alt, want_rgb, want_borders, channel_names):
        calls["overlay"] += 1
        assert seg.dtype.name in plot_utils._DEVICE_LABEL_DTYPES and all(c.dtype.name in plot_utils._DEVICE_PLANE_DTYPES
                                                                         for c in channels)
        if want_rgb:
            for i, c in enumerate(channels):
                if np.max(c) != 0 and not (c > 0).any():
                    raise ValueError("channel %s has a non-zero maximum but no positive pixel" % (channel_names[i],))
        rgb = ovr.overlay(np.stack(channels, axis=-1), seg, alt) if want_rgb else None
        return rgb, ovr.borders(seg) if want_borders else None

    def colorize(mask, table):
        calls["colorize"] += 1
        bad = mask.min() < 0 or mask.max() >= table.shape[0]
        return table[np.clip(mask, 0, table.shape[0] - 1)], int(bad)

    def sums(planar, groups):
        calls["sums"] += 1
        stack = np.moveaxis(planar, 0, -1)
        return [ovr.deepcell_pages(stack, g, [])[0] for g in groups]

    monkeypatch.setattr(plot_utils, "_overlay_device", overlay)
    monkeypatch.setattr(plot_utils, "_colorize_device", colorize)
    monkeypatch.setattr(deepcell_service_utils, "_channel_sums_device", sums)
    return calls


def _write_overlay_inputs(g, p, folder, fov):
    from ark_analysis_amd import image_io
    image_io.write_stack(os.path.join(folder, fov + ".tiff"), g[p + "pages"])
    image_io.write_image(os.path.join(folder, fov + "_whole_cell.tiff"), g[p + "cell"])
    image_io.write_image(os.path.join(folder, fov + "_nuclear.tiff"), g[p + "nuc"])


def test_create_overlay_and_save_segmentation_labels_write_the_reference_files(golden, statement, tmp_path):
    from ark_analysis_amd import image_io
    from ark_analysis_amd.segmentation import segmentation_utils
    from ark_analysis_amd.utils import plot_utils
    for name in (str(n) for n in golden["overlay_names"]):
        p, chans, comp, tif, seg, alt = _overlay_case(golden, name)
        folder = tmp_path / name
        out_dir = folder / "out"
        out_dir.mkdir(parents=True)
        _write_overlay_inputs(golden, p, str(folder), "fov0")
        got = plot_utils.create_overlay("fov0", str(folder), str(folder), chans, comp, alternate_segmentation=alt)
        assert got.dtype == np.uint8 and np.array_equal(got, golden[p + "overlay"]), name
        assert np.array_equal(plot_utils.overlay_image(tif, seg, alt), golden[p + "overlay"]), name
        segmentation_utils.save_segmentation_labels(str(folder), str(folder), str(out_dir), ["fov0"], channels=chans)
        assert sorted(os.listdir(out_dir)) == sorted(["fov0_segmentation_borders.tiff", "_".join(["fov0", *chans, "overlay.tiff"])])
        assert np.array_equal(image_io.read_image(str(out_dir / "fov0_segmentation_borders.tiff")), golden[p + "borders"])
        assert np.array_equal(image_io.read_image(str(out_dir / "_".join(["fov0", *chans, "overlay.tiff"]))),
                              golden[p + "saved_overlay"])
    assert statement["overlay"] > 0
    # borders alone
    folder = tmp_path / "borders"
    folder.mkdir()
    image_io.write_image(str(folder / "fovb_whole_cell.tiff"), golden["b_cell"])
    segmentation_utils.save_segmentation_labels(str(folder), str(folder), str(folder), ["fovb"])
    assert sorted(os.listdir(folder)) == ["fovb_segmentation_borders.tiff", "fovb_whole_cell.tiff"]
    assert np.array_equal(image_io.read_image(str(folder / "fovb_segmentation_borders.tiff")), golden["b_borders"])


def test_tif_overlay_preprocess(golden):
    from ark_analysis_amd.utils import plot_utils
    seg = np.zeros((4, 5), dtype=np.int32)
    rs = np.random.RandomState(3)
    for c in (1, 2, 3):
        tif = rs.randint(0, 100, size=(4, 5, c)).astype(np.uint16)
        got = plot_utils.tif_overlay_preprocess(seg, tif)
        assert got.dtype == tif.dtype and got.shape == (4, 5, 3) and np.array_equal(got, ovr.tif_overlay_preprocess(tif))
        for i in range(c):
            assert np.array_equal(got[..., 2 - i], tif[..., i])
    flat = plot_utils.tif_overlay_preprocess(seg, tif[..., 0])
    assert np.array_equal(flat[..., 2], tif[..., 0]) and not flat[..., :2].any()
    with pytest.raises(ValueError, match="plotting_tif and segmentation_labels array dimensions not equal."):
        plot_utils.tif_overlay_preprocess(seg, np.zeros((4, 6)))
    with pytest.raises(ValueError, match="max 3 channels of overlay supported, got"):
        plot_utils.tif_overlay_preprocess(seg, np.zeros((4, 5, 4)))
    with pytest.raises(ValueError, match="plotting tif must be 2D or 3D array, got"):
        plot_utils.tif_overlay_preprocess(seg, np.zeros((4, 5, 1, 1)))


def test_host_path_for_dtypes_the_device_does_not_read(golden, statement):
    """float64 planes and int8 / uint64 labels take the same statement on the host: no device entry is called."""
    from ark_analysis_amd.utils import plot_utils
    _, _, _, tif, seg, alt = _overlay_case(golden, "f32_both_alt")
    before = statement["overlay"]
    got = plot_utils.overlay_image(tif.astype(np.float64), seg, alt)
    assert np.array_equal(got, ovr.overlay(tif.astype(np.float64), seg, alt))
    small = (seg % 100).astype(np.int8)
    assert np.array_equal(plot_utils.overlay_image(tif, small, alt), ovr.overlay(tif, small, alt))
    assert np.array_equal(plot_utils.segmentation_borders(seg.astype(np.uint64)), ovr.borders(seg))
    assert statement["overlay"] == before
    assert np.array_equal(plot_utils.overlay_image(tif, seg, alt), ovr.overlay(tif, seg, alt)) and statement["overlay"] == before + 1


def test_generate_deepcell_input_writes_the_reference_pages(golden, statement, tmp_path):
    from ark_analysis_amd import image_io
    from ark_analysis_amd.utils import deepcell_service_utils
    for name in (str(n) for n in golden["deepcell_names"]):
        p = "d_%s_" % name
        stack = golden[p + "stack"]
        chans = ["chan%d" % i for i in range(stack.shape[2])]
        tiff_dir, data_dir = tmp_path / name / "tiffs", tmp_path / name / "input"
        (tiff_dir / "fov0" / "TIFs").mkdir(parents=True)
        data_dir.mkdir()
        for i, ch in enumerate(chans):
            image_io.write_image(str(tiff_dir / "fov0" / "TIFs" / (ch + ".tiff")), stack[:, :, i])
        deepcell_service_utils.generate_deepcell_input(str(data_dir), str(tiff_dir), [chans[i] for i in golden[p + "nuc"]],
                                                       [chans[i] for i in golden[p + "mem"]], ["fov0"])
        assert os.listdir(data_dir) == ["fov0.tiff"]
        got = image_io.read_stack(str(data_dir / "fov0.tiff"))
        assert got.dtype == stack.dtype and np.array_equal(got, golden[p + "pages"]), name
    assert statement["sums"] == len(golden["deepcell_names"])


def _colormap_inputs(golden, folder):
    path = os.path.join(folder, "names.csv")
    with open(path, "w") as f:
        f.write(str(golden["c_names_text"]))
    colors = {int(k): tuple(float(x) for x in v) for k, v in zip(golden["c_color_keys"], golden["c_color_values"])}
    return path, colors


def test_metacluster_colormap_and_save_colored_masks(golden, statement, tmp_path):
    from ark_analysis_amd import image_io
    from ark_analysis_amd.utils import plot_utils
    path, colors = _colormap_inputs(golden, str(tmp_path))
    mcc = plot_utils.MetaclusterColormap(cluster_type="cell", cluster_id_to_name_path=path, metacluster_colors=colors)
    assert np.array_equal(mcc.mc_colors, golden["c_mc_colors"])
    assert mcc.metacluster_id_to_name.drop(columns="color").to_csv(index=False) == str(golden["c_table_text"])
    assert list(colors.keys()) == list(golden["c_updated_keys"])                 # the caller's dict gains two colours
    assert np.array_equal(np.array([colors[k] for k in colors]), golden["c_updated_values"])
    assert mcc.unassigned_color == (0.9, 0.9, 0.9, 1.0) and mcc.background_color == (0.0, 0.0, 0.0, 1.0)
    assert np.array_equal(np.asarray(mcc.cmap.colors), golden["c_cmap_colors"])
    assert np.array_equal(mcc.norm.boundaries, golden["c_norm_boundaries"]) and mcc.norm.Ncmap == int(golden["c_norm_ncolors"])
    names = list(mcc.metacluster_id_to_name["cell_meta_cluster_rename"])
    assert names[0] == "Empty" and names[-1] == "Unassigned"

    fovs = ["fov0", "fov1"]
    for fov in fovs:
        image_io.write_image(str(tmp_path / (fov + "_cell_mask.tiff")), golden["c_mask_" + fov])
    path, colors = _colormap_inputs(golden, str(tmp_path))
    plot_utils.save_colored_masks(fovs, str(tmp_path), str(tmp_path / "new" / "colored"), path, colors, "cell")
    for fov in fovs:
        got = image_io.read_image(str(tmp_path / "new" / "colored" / (fov + "_cell_mask_colored.tiff")))
        assert got.dtype == np.uint8 and np.array_equal(got, golden["c_colored_" + fov])
    assert statement["colorize"] == 2
    # three colour columns, and a mask dtype the device does not read (the host path)
    rgb = golden["c_mc_colors"][:, :3]
    mask = golden["c_mask_fov0"]
    assert np.array_equal(plot_utils.colored_mask(mask, rgb), ovr.colored_mask(mask, rgb))
    assert np.array_equal(plot_utils.colored_mask(mask.astype(np.int64), rgb), ovr.colored_mask(mask, rgb))
    assert statement["colorize"] == 3


# ---- the files -------------------------------------------------------------------------------------------------------
def test_stack_and_rgb_tiffs_round_trip_and_pillow_reads_them(tmp_path):
    from PIL import Image
    from ark_analysis_amd import image_io
    rs = np.random.RandomState(8)
    path = str(tmp_path / "stack.tiff")
    for dtype in ("uint8", "uint16", "int16", "int32", "uint32", "float32"):
        for shape in ((2, 5, 7), (1, 3, 3), (3, 1, 1), (2, 7, 5)):
            pages = (rs.rand(*shape) * 200 - (50 if dtype[0] != "u" else 0)).astype(dtype)
            image_io.write_stack(path, pages)
            got = image_io.read_stack(path)
            assert got.dtype == pages.dtype and np.array_equal(got, pages), (dtype, shape)
            with Image.open(path) as im:
                assert im.n_frames == shape[0]
                for i in range(shape[0]):
                    im.seek(i)
                    if dtype != "uint32":               # (Pillow has no unsigned 32-bit mode)
                        assert np.array_equal(np.array(im).astype(dtype), pages[i]), (dtype, shape, i)
    # the single-image readers keep refusing what they refused
    image_io.write_stack(path, np.zeros((2, 4, 4), dtype=np.int16))
    with pytest.raises(NotImplementedError, match="multi-page"):
        image_io.read_tiff_shaped(path)
    image_io.write_image(path, np.arange(12, dtype=np.int32).reshape(3, 4))
    assert np.array_equal(image_io.read_stack(path), np.arange(12, dtype=np.int32).reshape(1, 3, 4))
    # compressed pages fall back to Pillow
    frames = [Image.fromarray(rs.randint(0, 255, size=(6, 4)).astype(np.uint8)) for _ in range(3)]
    frames[0].save(path, save_all=True, append_images=frames[1:], compression="tiff_lzw")
    assert np.array_equal(image_io.read_stack(path), np.stack([np.array(f) for f in frames]))
    for c, mode in ((3, "RGB"), (4, "RGBA")):
        for hw in ((1, 1), (5, 7), (4, 3)):
            image = rs.randint(0, 256, size=hw + (c,)).astype(np.uint8)
            image_io.write_rgb(path, image)
            with Image.open(path) as im:
                assert im.mode == mode and np.array_equal(np.array(im), image)
            assert np.array_equal(image_io.read_image(path), image)
    for bad in (np.zeros((2, 3)), np.zeros((2, 3, 4), dtype=np.float64), np.zeros((0, 3, 4), dtype=np.uint8)):
        with pytest.raises(ValueError):
            image_io.write_stack(path, bad)
    for bad in (np.zeros((2, 3), dtype=np.uint8), np.zeros((2, 3, 2), dtype=np.uint8), np.zeros((2, 3, 3), dtype=np.uint16)):
        with pytest.raises(ValueError):
            image_io.write_rgb(path, bad)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_file(golden, statement, tmp_path):
    from ark_analysis_amd import image_io
    from ark_analysis_amd.segmentation import segmentation_utils
    from ark_analysis_amd.utils import deepcell_service_utils, plot_utils
    p = "o_i16_one_"
    folder, out_dir = tmp_path / "in", tmp_path / "out"
    folder.mkdir()
    out_dir.mkdir()
    _write_overlay_inputs(golden, p, str(folder), "fov0")
    with pytest.raises(ValueError, match="Not all values given in list provided_channels"):
        plot_utils.create_overlay("fov0", str(folder), str(folder), ["dsDNA"], "whole_cell")
    with pytest.raises(ValueError, match="Not all values given in list provided_compartments"):
        plot_utils.create_overlay("fov0", str(folder), str(folder), ["nuclear_channel"], "cytoplasm")
    with pytest.raises(ValueError, match="segmentation_labels and alternate_segmentation array dimensions not equal."):
        plot_utils.create_overlay("fov0", str(folder), str(folder), ["nuclear_channel"], "whole_cell",
                                  alternate_segmentation=np.zeros((3, 3), dtype=np.int32))
    seg = golden[p + "cell"]
    with pytest.raises(ValueError, match="plotting_tif and segmentation_labels array dimensions not equal."):
        plot_utils.overlay_image(np.zeros((5, 5), dtype=np.uint8), seg)
    with pytest.raises(ValueError, match="max 3 channels of overlay supported"):
        plot_utils.overlay_image(np.zeros(seg.shape + (4,), dtype=np.uint8), seg)
    with pytest.raises(ValueError, match="plotting tif must be 2D or 3D array"):
        plot_utils.overlay_image(np.zeros(seg.shape + (1, 1), dtype=np.uint8), seg)
    # a non-zero maximum without a positive pixel: the channel is named, on the device route and on the host route, and
    # save_segmentation_labels leaves no file of that FOV
    negative = -np.abs(golden[p + "pages"]) - 1
    image_io.write_stack(str(folder / "fov0.tiff"), negative)
    with pytest.raises(ValueError, match="channel membrane_channel has a non-zero maximum but no positive pixel"):
        segmentation_utils.save_segmentation_labels(str(folder), str(folder), str(out_dir), ["fov0"],
                                                    channels=["nuclear_channel", "membrane_channel"][::-1])
    assert os.listdir(out_dir) == []
    with pytest.raises(ValueError, match="channel 0 has a non-zero maximum but no positive pixel"):
        plot_utils.overlay_image(negative[0].astype(np.float64), seg)
    # a single-page file where the two pages are expected
    image_io.write_image(str(folder / "fov0.tiff"), negative[0])
    with pytest.raises(ValueError, match="must hold the two pages"):
        plot_utils.create_overlay("fov0", str(folder), str(folder), ["nuclear_channel"], "whole_cell")

    with pytest.raises(ValueError, match="Either nuc_channels or mem_channels should be non-empty."):
        deepcell_service_utils.generate_deepcell_input(str(out_dir), str(folder), [], None, ["fov0"])
    with pytest.raises(NotImplementedError):
        deepcell_service_utils.generate_deepcell_input(str(out_dir), str(folder), ["a"], None, ["fov0"], is_mibitiff=True)
    assert os.listdir(out_dir) == []

    # coloured masks: an index outside the table, negative ones included; a wrong cluster type; missing columns
    path, colors = _colormap_inputs(golden, str(tmp_path))
    table = golden["c_mc_colors"]
    for dtype in (np.int16, np.int64):
        for value in (-1, table.shape[0]):
            mask = np.zeros((3, 4), dtype=dtype)
            mask[1, 2] = value
            with pytest.raises(IndexError, match="outside the colour table"):
                plot_utils.colored_mask(mask, table)
    image_io.write_image(str(tmp_path / "fov9_cell_mask.tiff"), np.full((3, 3), 99, dtype=np.int16))
    with pytest.raises(IndexError):
        plot_utils.save_colored_masks(["fov9"], str(tmp_path), str(tmp_path / "colored"), path, dict(colors), "cell")
    assert os.listdir(tmp_path / "colored") == []
    with pytest.raises(ValueError, match="provided_cluster_type"):
        plot_utils.save_colored_masks(["fov9"], str(tmp_path), str(tmp_path / "colored"), path, dict(colors), "tissue")
    pd.read_csv(path).drop(columns="cluster_id").to_csv(path, index=False)
    with pytest.raises(ValueError, match="required_cols"):
        plot_utils.MetaclusterColormap(cluster_type="cell", cluster_id_to_name_path=path, metacluster_colors=dict(colors))


def test_library_refuses_bad_arguments_before_any_hip_call():
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    modes, ranges = (ctypes.c_int32 * 3)(0, 0, 1), (ctypes.c_double * 6)(0, 0, 0, 0, 1.0, 2.0)
    p = ctypes.c_void_p(4096)                  # never dereferenced: every call below is refused first

    def overlay(r=None, g=None, b=p, pdt=7, modes=modes, ranges=ranges, seg=p, sdt=3, alt=None, adt=0, h=4, w=4, rgb=p, borders=None):
        return lib.pxsom_overlay_rgb(r, g, b, pdt, modes, ranges, seg, sdt, alt, adt, h, w, rgb, borders, None)

    assert overlay(h=0) == -1 and b"bad sizes" in lib.pxsom_last_error()
    assert overlay(seg=None) == -1 and overlay(sdt=7) == -1 and overlay(alt=p, adt=9) == -1
    assert overlay(rgb=None) == -1 and b"no output" in lib.pxsom_last_error()
    assert overlay(b=None) == -1 and b"without a plane" in lib.pxsom_last_error()
    assert overlay(pdt=5) == -1 and b"plane_dtype" in lib.pxsom_last_error()
    assert overlay(modes=(ctypes.c_int32 * 3)(0, 0, 3)) == -1 and b"bad mode" in lib.pxsom_last_error()
    assert overlay(modes=(ctypes.c_int32 * 3)(0, 0, 2)) == -1 and b"does not fit mode" in lib.pxsom_last_error()
    assert overlay(ranges=(ctypes.c_double * 6)(0, 0, 0, 0, 2.0, 2.0)) == -1
    assert overlay(ranges=(ctypes.c_double * 6)(0, 0, 0, 0, 1.0, float("inf"))) == -1
    assert overlay(rgb=ctypes.c_void_p(4096 + 8)) == -1 and b"overlaps" in lib.pxsom_last_error()
    status = ctypes.c_void_p(8192)
    assert lib.pxsom_colorize(p, 3, 0, 4, p, 5, 3, p, status, None) == -1
    assert lib.pxsom_colorize(p, 5, 4, 4, p, 5, 3, p, status, None) == -1 and b"mask_dtype" in lib.pxsom_last_error()
    assert lib.pxsom_colorize(p, 3, 4, 4, p, 5, 2, p, status, None) == -1 and b"bad table" in lib.pxsom_last_error()
    assert lib.pxsom_colorize(p, 3, 4, 4, None, 5, 3, p, status, None) == -1
    q = (ctypes.c_double * 2)(0.05, 1.5)
    assert lib.pxsom_percentile_f32_listq(p, 10, 1, 1, q, 2, 1, p, p, 1 << 20, None) == -1
    assert b"outside [0, 1]" in lib.pxsom_last_error()
    assert lib.pxsom_percentile_f32_listq(p, 10, 1, 1, None, 2, 1, p, p, 1 << 20, None) == -1


def test_abi_stays_9_with_the_new_symbols():
    from ark_analysis_amd import _capi, som_device as sd
    lib = _capi.lib()
    header = open(os.path.join(ROOT, "include", "pxsom.h")).read()
    assert _capi.ABI_VERSION == 9 and re.search(r"#define PXSOM_ABI_VERSION 9\b", header) and "K29" in header
    assert lib.pxsom_abi_version() == 9
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and re.search(r"\b%s\(" % name, header) and hasattr(lib, name), name
    for name, value in (("PXSOM_OVERLAY_ZERO", sd.OVERLAY_ZERO), ("PXSOM_OVERLAY_RESCALE", sd.OVERLAY_RESCALE),
                        ("PXSOM_OVERLAY_CLIP", sd.OVERLAY_CLIP), ("PXSOM_COLORIZE_BAD_INDEX", sd.COLORIZE_BAD_INDEX)):
        assert re.search(r"^#define %s %d$" % (name, value), header, flags=re.M), name
    assert os.path.exists(os.path.join(ROOT, "ark_analysis_amd", "csrc", "pxsom_overlay.hip"))


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/ark"), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_committed_fixture(golden, tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_overlays.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with np.load(tmp_path / "g32_overlays.npz") as g:
        assert sorted(g.files) == sorted(golden)
        for k in g.files:
            assert g[k].dtype == golden[k].dtype and np.array_equal(g[k], golden[k]), k
