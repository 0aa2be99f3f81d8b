#!/usr/bin/env python
"""Generates tests/golden/g32_overlays.npz: the outputs of the REFERENCE's own ark.utils.plot_utils.create_overlay,
ark.segmentation.segmentation_utils.save_segmentation_labels, ark.utils.deepcell_service_utils.generate_deepcell_input,
ark.utils.plot_utils.MetaclusterColormap and save_colored_masks, imported from /root/reference/src with
tests/golden/_shims, as the other generators do.  The file holds inputs and recorded outputs only.

scikit-image, xarray, alpineer and tifffile are absent from this image.  The stand-ins below are installed from this
generator (the files under _shims stay as they are); each is a restatement, so parity with the missing library itself
is unpinned:
  - skimage.exposure.rescale_intensity: scikit-image 0.19's body as recalled, for a numeric in_range and a dtype-name
    out_range -- clip to in_range; if the range is not empty (image - imin) / (imax - imin) and
    np.asarray(image * (omax - omin) + omin, dtype=out_dtype); else np.clip(image, omin, omax).astype(out_dtype).
    skimage.util.img_as_ubyte is imported only.
  - skimage.segmentation.find_boundaries, mode "inner": dilation != erosion of scipy.ndimage with the footprint
    generate_binary_structure(ndim, connectivity) under scipy's reflect border, and image != background
    (as make_golden_cell_masks.py states it).  skimage.measure / skimage.morphology are imported only.
  - xarray.DataArray: label indexing (.loc) axis by axis, .values, coordinates and dims as attributes -- what
    create_overlay, save_segmentation_labels and generate_deepcell_input touch.  A list of labels on the last axis gives
    a C-contiguous [H, W, c] array: the layout the real xarray hands to np.sum is unpinned.
  - alpineer.load_utils.load_imgs_from_dir / load_imgs_from_tree: the TIFFs read with ark_analysis_amd.image_io; a
    multi-page file is taken channels first and moved to [H, W, C], as alpineer does.  alpineer.image_utils.save_image
    records the array it is given and writes nothing.
  - requests, tifffile, tqdm.notebook: imported only (network code).

    python tests/golden/make_golden_overlays.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed file.
"""
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")

import scipy.ndimage as ndi  # noqa: E402

from ark_analysis_amd import image_io  # noqa: E402
from tests import overlay_reference as ovr  # noqa: E402  (only its input builders: cells, signal)

OUT_DIR = os.environ.get("PXSOM_GOLDEN_OUT", HERE)


# ---- skimage ------------------------------------------------------------------------------------------------------
_DTYPE_RANGE = {"uint8": (0, 255), "uint16": (0, 65535), "int16": (-32768, 32767)}


def rescale_intensity(image, in_range="image", out_range="dtype"):
    if isinstance(in_range, str) or not isinstance(out_range, str):
        raise NotImplementedError("rescale_intensity stand-in: numeric in_range and a dtype-name out_range only")
    out_dtype = np.dtype(out_range)
    imin, imax = map(float, in_range)
    omin, omax = map(float, _DTYPE_RANGE[out_range])
    if imin >= 0:
        omin = 0.0                                  # clip_negative
    image = np.clip(image, imin, imax)
    if imin != imax:
        image = (image - imin) / (imax - imin)
        return np.asarray(image * (omax - omin) + omin, dtype=out_dtype)
    return np.clip(image, omin, omax).astype(out_dtype)


def find_boundaries(label_img, connectivity=1, mode="thick", background=0):
    img = np.asarray(label_img)
    fp = ndi.generate_binary_structure(img.ndim, connectivity)
    edges = ndi.grey_dilation(img, footprint=fp) != ndi.grey_erosion(img, footprint=fp)
    if mode != "inner":
        raise NotImplementedError(mode)
    return edges & (img != background)


def _module(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


import skimage  # noqa: E402  (the _shims package)
skimage.exposure = _module("skimage.exposure", rescale_intensity=rescale_intensity)
skimage.util = _module("skimage.util", img_as_ubyte=None)
skimage.measure = _module("skimage.measure", regionprops_table=None, regionprops=None, label=None, moments=None)
skimage.morphology = _module("skimage.morphology", remove_small_objects=None)
_module("tifffile", imread=None)
for _name in ("requests", "tqdm.notebook"):
    try:
        __import__(_name)
    except ImportError:
        _module(_name, tqdm=None)


# ---- xarray.DataArray ---------------------------------------------------------------------------------------------
class _Coord:
    def __init__(self, values):
        self.values = np.asarray(values)


class DataArray:
    def __init__(self, data, coords=None, dims=None):
        self.values = np.asarray(data)
        self.dims = tuple(dims)
        self._coords = {d: np.asarray(c.values if isinstance(c, _Coord) else c) for d, c in zip(self.dims, coords)}

    def __getattr__(self, name):
        coords = self.__dict__.get("_coords", {})
        if name in coords:
            return _Coord(coords[name])
        raise AttributeError(name)

    @property
    def shape(self):
        return self.values.shape

    @property
    def dtype(self):
        return self.values.dtype

    @property
    def loc(self):
        return self

    def squeeze(self):
        return np.squeeze(self.values)          # (used as an index only)

    def __getitem__(self, key):
        values, dims, coords = self.values, [], []
        for axis in reversed(range(len(self.dims))):
            k, c = key[axis], self._coords[self.dims[axis]]
            if isinstance(k, slice):
                assert k == slice(None)
                dims.insert(0, self.dims[axis])
                coords.insert(0, c)
            elif isinstance(k, (list, np.ndarray)):
                idx = [int(np.flatnonzero(c == v)[0]) for v in k]
                values = np.take(values, idx, axis=axis)
                dims.insert(0, self.dims[axis])
                coords.insert(0, c[idx])
            else:
                values = np.take(values, int(np.flatnonzero(c == k)[0]), axis=axis)
        return DataArray(np.ascontiguousarray(values), coords, dims)


xarray = _module("xarray", DataArray=DataArray)


# ---- alpineer -----------------------------------------------------------------------------------------------------
def load_imgs_from_dir(data_dir, files=None, xr_dim_name="compartments", xr_channel_names=None, trim_suffix=None, **kwargs):
    imgs = []
    for f in files:
        pages = image_io.read_stack(os.path.join(str(data_dir), f))
        imgs.append(np.moveaxis(pages, 0, -1))
    arr = np.stack(imgs, axis=0)
    names = [os.path.splitext(f)[0] for f in files]
    if trim_suffix:
        names = [n.split(trim_suffix)[0] for n in names]
    chans = list(xr_channel_names) if xr_channel_names is not None else list(range(arr.shape[3]))
    return DataArray(arr, [names, range(arr.shape[1]), range(arr.shape[2]), chans], ["fovs", "rows", "cols", xr_dim_name])


def load_imgs_from_tree(data_dir, img_sub_folder=None, fovs=None, channels=None, **kwargs):
    stacks = [np.ascontiguousarray(image_io.read_channels(data_dir, f, channels, img_sub_folder or "")) for f in fovs]
    arr = np.stack(stacks, axis=0).astype(stacks[0].dtype, copy=False)
    return DataArray(arr, [list(fovs), range(arr.shape[1]), range(arr.shape[2]), list(channels)],
                     ["fovs", "rows", "cols", "channels"])


SAVED = {}


def save_image(fname, data, compression_level=6):
    SAVED[os.path.basename(str(fname))] = np.array(data)


from alpineer import image_utils, load_utils  # noqa: E402  (the _shims modules)
load_utils.load_imgs_from_dir = load_imgs_from_dir
load_utils.load_imgs_from_tree = load_imgs_from_tree
image_utils.save_image = save_image

from ark.segmentation import segmentation_utils as ref_seg  # noqa: E402
from ark.utils import deepcell_service_utils as ref_deepcell  # noqa: E402
from ark.utils import plot_utils as ref_plot  # noqa: E402

ref_plot.find_boundaries = find_boundaries
ref_seg.find_boundaries = find_boundaries
ref_plot.xr = xarray
assert ref_plot.rescale_intensity is rescale_intensity


# ---- cases --------------------------------------------------------------------------------------------------------
# (name, (h, w), plane dtype, label dtype, nuclear page kind, membrane page kind, channels, compartment, alt dtype)
OVERLAY_CASES = [
    ("u16_both", (37, 41), np.uint16, np.int32, "plain", "plain", ["nuclear_channel", "membrane_channel"], "whole_cell", None),
    ("f32_both_alt", (33, 64), np.float32, np.int32, "plain", "plain", ["membrane_channel", "nuclear_channel"], "nuclear",
     np.uint8),
    ("i16_one", (24, 29), np.int16, np.uint16, "plain", "plain", ["membrane_channel"], "whole_cell", None),
    ("u8_zero_and_one", (17, 23), np.uint8, np.uint8, "zero", "one", ["nuclear_channel", "membrane_channel"], "whole_cell",
     np.int32),
    ("i32_equal", (20, 20), np.int32, np.int32, "equal", "plain", ["nuclear_channel", "membrane_channel"], "nuclear", None),
    ("f32_one", (9, 13), np.float32, np.int32, "one", "plain", ["nuclear_channel"], "whole_cell", None),
]


def overlay_cases(out):
    out["overlay_names"] = np.array([c[0] for c in OVERLAY_CASES])
    for n, (name, (h, w), pdt, ldt, knuc, kmem, chans, comp, adt) in enumerate(OVERLAY_CASES):
        pages = np.stack([ovr.signal(h, w, 100 + 2 * n, pdt, knuc), ovr.signal(h, w, 101 + 2 * n, pdt, kmem)])
        cell, nuc = ovr.cells(h, w, 200 + n, ldt), ovr.cells(h, w, 300 + n, ldt, big=np.dtype(ldt).itemsize >= 4)
        alt = None if adt is None else ovr.cells(h, w, 400 + n, adt)
        with tempfile.TemporaryDirectory() as td:
            image_io.write_stack(os.path.join(td, "fov0.tiff"), pages)
            image_io.write_image(os.path.join(td, "fov0_whole_cell.tiff"), cell)
            image_io.write_image(os.path.join(td, "fov0_nuclear.tiff"), nuc)
            got = ref_plot.create_overlay("fov0", td, td, chans, comp, alternate_segmentation=alt)
            SAVED.clear()
            ref_seg.save_segmentation_labels(td, td, td, ["fov0"], channels=chans)
            saved = dict(SAVED)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        p = "o_%s_" % name
        out[p + "pages"], out[p + "cell"], out[p + "nuc"] = pages, cell, nuc
        out[p + "chans"], out[p + "comp"] = np.array(chans), np.array(comp)
        if alt is not None:
            out[p + "alt"] = alt
        out[p + "overlay"] = got
        out[p + "borders"] = saved["fov0_segmentation_borders.tiff"]
        out[p + "saved_overlay"] = saved["_".join(["fov0", *chans, "overlay.tiff"])]
    # borders alone
    cell = ovr.cells(31, 35, 555, np.int32, big=True)
    with tempfile.TemporaryDirectory() as td:
        image_io.write_image(os.path.join(td, "fovb_whole_cell.tiff"), cell)
        SAVED.clear()
        ref_seg.save_segmentation_labels(td, td, td, ["fovb"])
        assert list(SAVED) == ["fovb_segmentation_borders.tiff"]
        out["b_cell"], out["b_borders"] = cell, SAVED["fovb_segmentation_borders.tiff"]


# (name, dtype, channel count, nuclear channel positions, membrane channel positions)
DEEPCELL_CASES = [
    ("i16_wrap", np.int16, 4, [0, 1, 2], [3, 1]),
    ("u16_wrap", np.uint16, 3, [0, 1, 2], []),
    ("f32_1", np.float32, 2, [1], [0]),
    ("f32_2", np.float32, 3, [], [2, 0]),
    ("f32_7", np.float32, 8, [0, 1, 2, 3, 4, 5, 6], [7]),
    ("f32_9", np.float32, 10, [9, 0, 1, 2, 3, 4, 5, 6, 7], [8, 3]),
]


def deepcell_cases(out):
    out["deepcell_names"] = np.array([c[0] for c in DEEPCELL_CASES])
    for n, (name, dtype, c, nuc, mem) in enumerate(DEEPCELL_CASES):
        rs = np.random.RandomState(600 + n)
        h, w = 19 + n, 23
        if np.dtype(dtype).kind == "f":
            stack = (rs.gamma(2.0, 50.0, size=(h, w, c)) * 10.0 ** rs.randint(-3, 4, size=(h, w, c))).astype(dtype)
        else:
            info = np.iinfo(dtype)
            stack = rs.randint(info.max // 2, info.max, size=(h, w, c)).astype(dtype)     # sums past the dtype's range
        chans = ["chan%d" % i for i in range(c)]
        with tempfile.TemporaryDirectory() as td:
            os.makedirs(os.path.join(td, "fov0", "TIFs"))
            for i, ch in enumerate(chans):
                image_io.write_image(os.path.join(td, "fov0", "TIFs", ch + ".tiff"), stack[:, :, i])
            SAVED.clear()
            ref_deepcell.generate_deepcell_input(td, td, [chans[i] for i in nuc], [chans[i] for i in mem], ["fov0"])
            got = SAVED["fov0.tiff"]
        assert got.shape == (2, h, w) and got.dtype == np.dtype(dtype)
        p = "d_%s_" % name
        out[p + "stack"], out[p + "nuc"], out[p + "mem"], out[p + "pages"] = stack, np.array(nuc, dtype=np.int64), \
            np.array(mem, dtype=np.int64), got


def color_cases(out):
    """MetaclusterColormap and save_colored_masks: a GUI CSV whose cluster ids are not in the order of its rows, RGBA
    colours, int16 masks holding every id, the unassigned one included."""
    rs = np.random.RandomState(700)
    gui = pd.DataFrame({"cell_som_cluster": np.arange(1, 9), "cell_meta_cluster": [3, 1, 1, 2, 4, 5, 5, 2],
                        "cell_meta_cluster_rename": ["cd8", "cd4", "cd4", "Bcell", "macro", "tumor", "tumor", "Bcell"],
                        "cluster_id": [3, 1, 1, 2, 4, 5, 5, 2]})
    colors = {m: tuple(float(v) for v in np.round(rs.rand(4), 3)) for m in range(1, 6)}
    fovs = ["fov0", "fov1"]
    masks = [rs.randint(0, 7, size=(21 + 5 * i, 30 - 3 * i)).astype(np.int16) for i in range(2)]
    with tempfile.TemporaryDirectory() as td:
        gui.to_csv(os.path.join(td, "names.csv"), index=False)
        given = dict(colors)
        mcc = ref_plot.MetaclusterColormap(cluster_type="cell", cluster_id_to_name_path=os.path.join(td, "names.csv"),
                                           metacluster_colors=given)
        for fov, mask in zip(fovs, masks):
            image_io.write_image(os.path.join(td, fov + "_cell_mask.tiff"), mask)
        SAVED.clear()
        ref_plot.save_colored_masks(fovs, td, os.path.join(td, "colored"), os.path.join(td, "names.csv"), dict(colors), "cell")
        saved = dict(SAVED)
    out["c_names_text"] = np.array(gui.to_csv(index=False))
    out["c_color_keys"] = np.array(sorted(colors), dtype=np.int64)
    out["c_color_values"] = np.array([colors[k] for k in sorted(colors)])
    out["c_updated_keys"] = np.array(list(given.keys()), dtype=np.int64)
    out["c_updated_values"] = np.array([given[k] for k in given])
    out["c_mc_colors"] = mcc.mc_colors
    out["c_table_text"] = np.array(mcc.metacluster_id_to_name.drop(columns="color").to_csv(index=False))
    out["c_cmap_colors"] = np.asarray(mcc.cmap.colors)
    out["c_norm_boundaries"] = np.asarray(mcc.norm.boundaries)
    out["c_norm_ncolors"] = np.int64(mcc.norm.Ncmap)
    for fov, mask in zip(fovs, masks):
        out["c_mask_" + fov] = mask
        out["c_colored_" + fov] = saved["%s_cell_mask_colored.tiff" % fov]


if __name__ == "__main__":
    arrays = {}
    overlay_cases(arrays)
    deepcell_cases(arrays)
    color_cases(arrays)
    path = os.path.join(OUT_DIR, "g32_overlays.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", os.path.relpath(path, ROOT), len(arrays), "arrays,", os.path.getsize(path), "bytes")
