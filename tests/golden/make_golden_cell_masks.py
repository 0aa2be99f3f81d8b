#!/usr/bin/env python
"""Generates tests/golden/g15_*.npz: the cell cluster masks of the REFERENCE's ark.utils.data_utils (erode_mask,
label_cells_by_cluster, map_segmentation_labels, generate_and_save_cell_cluster_masks,
generate_and_save_neighborhood_cluster_masks), imported from /root/reference/src with tests/golden/_shims, as
make_golden.py does.

scikit-image and numba are absent from this image, so three module attributes the reference looks up are patched here
(the shims under _shims stay as they are):
  - data_utils.find_boundaries: a restatement of skimage.segmentation.find_boundaries, modes "thick" and "inner" --
    dilation != erosion of scipy.ndimage with the footprint generate_binary_structure(ndim, connectivity), scipy's
    default reflect border, "inner" excluding `background`.  Parity with skimage itself is therefore unpinned (as for
    pyFlowSOM): every fixture that erodes carries this one restated call.
  - data_utils.nb: numba's int32-keyed typed dict as a Python dict that wraps keys and values to their numba types;
    relabel_segmentation's njit is already a pass-through in the numba shim.
  - data_utils.load_utils.load_imgs_from_dir: reads the one requested segmentation TIFF with Pillow and returns it as the
    [H, W, 1] array behind `.loc[fov, ...]`.

    python tests/golden/make_golden_cell_masks.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed files.
"""
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")

import scipy.ndimage as ndi  # noqa: E402
from PIL import Image  # noqa: E402

from ark.utils import data_utils  # noqa: E402

from ark_analysis_amd import image_io  # noqa: E402  (writes the int32 segmentation TIFFs the fixtures read)

OUT_DIR = os.environ.get("PXSOM_GOLDEN_OUT", HERE)


def save(name, **arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", os.path.relpath(path, ROOT), {k: getattr(v, "shape", None) for k, v in arrays.items()})


# ---- the patched lookups ------------------------------------------------------------------------------------------
def find_boundaries(label_img, connectivity=1, mode="thick", background=0):
    """skimage.segmentation.find_boundaries, modes thick / inner, restated with scipy.ndimage."""
    img = np.asarray(label_img)
    if img.dtype == bool:
        img = img.astype(np.uint8)
    fp = ndi.generate_binary_structure(img.ndim, connectivity)
    edges = ndi.grey_dilation(img, footprint=fp) != ndi.grey_erosion(img, footprint=fp)
    if mode == "inner":
        edges &= img != background
    elif mode != "thick":
        raise NotImplementedError(mode)
    return edges


class _Int32Dict(dict):
    """numba.typed.Dict.empty(key_type=int32, value_type=...): keys (and lookups) wrap to int32, values to their type."""

    def __init__(self, value_type):
        super().__init__()
        self._vt = value_type

    def __setitem__(self, k, v):
        super().__setitem__(int(np.array(k).astype(np.int64).astype(np.int32)), self._vt(v))

    def get(self, k, default=None):
        return super().get(int(np.array(k).astype(np.int64).astype(np.int32)), default)


class _Nb:
    prange = range

    class types:
        int32 = np.int32
        float64 = np.float64

    class typed:
        class Dict:
            @staticmethod
            def empty(key_type, value_type):
                return _Int32Dict(value_type)


class _Stack:
    def __init__(self, planes):
        self._planes = planes

    @property
    def loc(self):
        return self

    def __getitem__(self, key):
        return self._planes[key[0] if isinstance(key, tuple) else key]


def load_imgs_from_dir(data_dir, files=None, trim_suffix=None, **kwargs):
    planes = {}
    for f in files:
        with Image.open(os.path.join(data_dir, f)) as im:
            planes[f.split(trim_suffix)[0] if trim_suffix else os.path.splitext(f)[0]] = np.array(im)[..., None]
    return _Stack(planes)


def patch():
    import tqdm
    data_utils.find_boundaries = find_boundaries
    data_utils.nb = _Nb
    data_utils.load_utils.load_imgs_from_dir = load_imgs_from_dir
    data_utils.tqdm = tqdm.tqdm                   # the notebook bar needs ipywidgets (absent here)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def blocks(rs, h, w, n, lo=1, dtype=np.int32):
    """A label image of rectangular cells of random sparse labels, with some background 0."""
    yy = np.sort(rs.choice(np.arange(1, h), size=n - 1, replace=False))
    xx = np.sort(rs.choice(np.arange(1, w), size=n - 1, replace=False))
    ry, rx = np.searchsorted(yy, np.arange(h), side="right"), np.searchsorted(xx, np.arange(w), side="right")
    ids = rs.randint(lo, lo + 4 * n * n, size=(n, n))
    ids[rs.rand(n, n) < 0.15] = 0
    return ids[ry[:, None], rx[None, :]].astype(dtype)


def g15_erode():
    """erode_mask: defaults (connectivity 1, thick), connectivity 2 thick on [H, W, 1], inner with background 0 and 7,
    a uint16 and a uint8 image."""
    rs = np.random.RandomState(151)
    seg = blocks(rs, 23, 31, 6)
    seg[3:6, 4:9] = 7
    seg16 = blocks(rs, 19, 17, 5, lo=60000, dtype=np.int64).astype(np.uint16)
    seg8 = blocks(rs, 9, 40, 4, dtype=np.int64).astype(np.uint8)
    out = {"seg": seg, "seg16": seg16, "seg8": seg8,
           "default": data_utils.erode_mask(seg),
           "c2_thick_hw1": data_utils.erode_mask(seg[..., None], connectivity=2, mode="thick", background=0),
           "c1_inner": data_utils.erode_mask(seg, connectivity=1, mode="inner", background=0),
           "c2_inner_bg7": data_utils.erode_mask(seg, connectivity=2, mode="inner", background=7),
           "u16_c2_thick": data_utils.erode_mask(seg16, connectivity=2, mode="thick"),
           "u8_default": data_utils.erode_mask(seg8)}
    save("g15_erode", **out)


def _cell_table(rs, fovs, segs, cluster_names):
    """One row per cell label of every FOV, some labels left out, some extra labels absent from the image."""
    rows = []
    for fov, seg in zip(fovs, segs):
        labels = [int(v) for v in np.unique(seg) if v != 0]
        keep = [v for v in labels if rs.rand() > 0.1]
        extra = [int(v) for v in rs.randint(10 ** 6, 2 * 10 ** 6, size=3)]
        for v in keep + extra:
            rows.append((fov, v, cluster_names[rs.randint(len(cluster_names))]))
    return pd.DataFrame(rows, columns=["fov", "label", "cell_meta_cluster"])


def g15_label_cells():
    """label_cells_by_cluster: string cluster names, labels missing from the table, table labels missing from the image,
    a table row with label 0, a (fov, label) listed twice with different clusters; and a table of 40 000 integer
    clusters (ids past 32 767 wrap in the int16 mask)."""
    rs = np.random.RandomState(152)
    fovs = ["fov2", "fov10", "fov1"]
    segs = [blocks(rs, 21 + i, 27, 6) for i in range(3)]
    table = _cell_table(rs, fovs, segs, ["b_cell", "A_type", "mono", "t_cell"])
    lab0 = int(np.unique(segs[0])[3])
    extra = pd.DataFrame([("fov2", 0, "mono"), ("fov2", lab0, "t_cell"), ("fov2", lab0, "b_cell")],
                         columns=table.columns)
    table = pd.concat([table, extra], ignore_index=True)
    cmd = data_utils.ClusterMaskData(table, "fov", "label", "cell_meta_cluster")
    out = {"table_fov": table["fov"].values.astype(str), "table_label": table["label"].values,
           "table_cluster": table["cell_meta_cluster"].values.astype(str),
           "mapping_text": np.array(cmd.mapping.to_csv(index=False)),
           "cluster_names": np.array(cmd.cluster_names).astype(str), "unassigned_id": np.int64(cmd.unassigned_id),
           "n_clusters": np.int64(cmd.n_clusters), "unique_fovs": np.array(cmd.unique_fovs)}
    for fov, seg in zip(fovs, segs):
        out["seg_" + fov] = seg
        out["mask_" + fov] = data_utils.label_cells_by_cluster(fov, cmd, seg)

    # > 32 767 clusters: ids wrap in int16
    h, w = 160, 300
    big = np.arange(1, h * w + 1, dtype=np.int32).reshape(h, w)
    big[rs.rand(h, w) < 0.05] = 0
    labels = np.arange(1, h * w + 1)
    clusters = rs.permutation(40000)[labels % 40000]
    wide = pd.DataFrame({"fov": "fovw", "label": labels[:-50], "k": clusters[:-50]})
    cmd_w = data_utils.ClusterMaskData(wide, "fov", "label", "k")
    out.update(wide_seg=big, wide_label=wide["label"].values, wide_cluster=wide["k"].values,
               wide_unassigned_id=np.int64(cmd_w.unassigned_id),
               wide_mask=data_utils.label_cells_by_cluster("fovw", cmd_w, big))
    save("g15_label_cells", **out)


def g15_map_values():
    """map_segmentation_labels: a Series of values with NaN / +inf / -inf (replaced by 0), the default unassigned 0 and
    an explicit one; an ndarray of values with NaN (kept), a repeated label (the later value wins)."""
    rs = np.random.RandomState(153)
    seg = blocks(rs, 25, 22, 6)
    labels = np.array([int(v) for v in np.unique(seg) if v != 0][:-3] + [999999])
    values = rs.rand(labels.size) * 10
    values[[1, 4, 6]] = [np.nan, np.inf, -np.inf]
    arr_labels = np.concatenate([labels, labels[:2]])
    arr_values = np.concatenate([values, [5.5, 6.5]])
    out = {"seg": seg, "labels": labels, "values": values, "arr_labels": arr_labels, "arr_values": arr_values,
           "series": data_utils.map_segmentation_labels(pd.Series(labels), pd.Series(values), seg),
           "series_unassigned": data_utils.map_segmentation_labels(pd.Series(labels), pd.Series(values), seg[None],
                                                                   unassigned_id=-2.5),
           "ndarray": data_utils.map_segmentation_labels(arr_labels, arr_values, seg)}
    save("g15_map_values", **out)


def g15_saved_masks():
    """generate_and_save_cell_cluster_masks (sub_dir, name_suffix, a GUI CSV with a stale cluster_id column) and
    generate_and_save_neighborhood_cluster_masks on three small FOVs of int32 segmentations."""
    rs = np.random.RandomState(154)
    fovs = ["fov0", "fov1", "fov2"]
    segs = [blocks(rs, 26 + 3 * i, 33 - 2 * i, 7) for i in range(3)]
    names = ["cd4", "Bcell", "cd8", "macro", "tumor"]
    table = _cell_table(rs, fovs, segs, names)
    table = table.rename(columns={"cell_meta_cluster": "cell_meta_cluster_rename"})
    table["kmeans_neighborhood"] = rs.randint(1, 6, size=len(table))
    gui = pd.DataFrame({"cell_som_cluster": np.arange(1, 8), "cell_meta_cluster": [1, 2, 2, 3, 4, 5, 5],
                        "cell_meta_cluster_rename": ["cd4", "Bcell", "Bcell", "cd8", "macro", "tumor", "tumor"],
                        "cluster_id": 77})
    out = {"names_text": np.array(gui.to_csv(index=False)), "table_fov": table["fov"].values.astype(str),
           "table_label": table["label"].values, "table_cluster": table["cell_meta_cluster_rename"].values.astype(str),
           "table_kmeans": table["kmeans_neighborhood"].values}
    with tempfile.TemporaryDirectory() as td:
        seg_dir = os.path.join(td, "deepcell_output")
        os.makedirs(seg_dir)
        os.makedirs(os.path.join(td, "masks"))
        for fov, seg in zip(fovs, segs):
            image_io.write_image(os.path.join(seg_dir, fov + "_whole_cell.tiff"), seg)
            out["seg_" + fov] = seg
        gui.to_csv(os.path.join(td, "names.csv"), index=False)
        data_utils.generate_and_save_cell_cluster_masks(
            fovs=fovs, save_dir=os.path.join(td, "masks"), seg_dir=seg_dir, cell_data=table,
            cluster_id_to_name_path=os.path.join(td, "names.csv"), fov_col="fov", label_col="label",
            cell_cluster_col="cell_meta_cluster_rename", seg_suffix="_whole_cell.tiff", sub_dir="cell_masks",
            name_suffix="_cell_mask")
        out["names_after_text"] = np.array(open(os.path.join(td, "names.csv")).read())
        data_utils.generate_and_save_neighborhood_cluster_masks(
            fovs=fovs, save_dir=os.path.join(td, "masks"), seg_dir=seg_dir, neighborhood_data=table, fov_col="fov",
            label_col="label", cluster_col="kmeans_neighborhood", sub_dir="neighborhood_masks",
            name_suffix="_neighborhood_mask")
        for fov in fovs:
            for kind, suffix in (("cell", "_cell_mask"), ("neighborhood", "_neighborhood_mask")):
                with Image.open(os.path.join(td, "masks", kind + "_masks", fov + suffix + ".tiff")) as im:
                    saved = np.array(im)        # Pillow hands the int16 TIFF back in a wider container
                assert np.array_equal(saved.astype(np.int16), saved)
                out[kind + "_" + fov] = saved.astype(np.int16)
    save("g15_saved_masks", **out)


if __name__ == "__main__":
    patch()
    steps = {"erode": g15_erode, "label_cells": g15_label_cells, "map_values": g15_map_values,
             "saved_masks": g15_saved_masks}
    for name in (sys.argv[1:] or list(steps)):
        steps[name]()
