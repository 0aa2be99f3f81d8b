#!/usr/bin/env python
"""Generates tests/golden/g24_split_nuclei.npz: the planes of the REFERENCE's
ark.segmentation.segmentation_utils.split_large_nuclei and the cell tables of its
marker_quantification.generate_cell_table(nuclear_counts=True, split_large_nuclei=True, fast_extraction=True), imported
from /root/reference/src with the stand-ins of make_golden_cell_table.py (see there: regionprops_table for label and
coords in raster order, xarray.DataArray, the alpineer loaders).

One more stand-in is installed here: skimage.morphology.remove_small_objects restated for an INTEGER array, as
scikit-image 0.19 documents and implements it -- ``component_sizes = np.bincount(ar.ravel())``, every pixel whose label
has ``component_sizes < min_size`` set to 0, no connected components taken -- so parity with skimage itself is unpinned.

The inputs come from tests/split_nuclei_reference.py (the hand-built 24 x 70 plane, Voronoi cells with shifted nuclei);
the file holds inputs and recorded outputs only.

    python tests/golden/make_golden_split_nuclei.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed file.
"""
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_cell_table as base  # noqa: E402  (installs the stand-ins and imports the reference)

from ark.segmentation import segmentation_utils as ref_utils  # noqa: E402
from tests import split_nuclei_reference as snr  # noqa: E402

OUT_DIR = os.environ.get("PXSOM_GOLDEN_OUT", HERE)


def remove_small_objects(ar, min_size=64, **kwargs):
    if ar.dtype.kind not in "iu":
        raise TypeError("Only bool or integer image types are supported. Got %s." % ar.dtype)
    out = ar.copy()
    component_sizes = np.bincount(out.ravel())
    out[(component_sizes < min_size)[out]] = 0
    return out


ref_utils.remove_small_objects = remove_small_objects

# (name, plane source, dtype, cell_ids kind, min_size)
SPLIT_CASES = [("hand_%s" % kind, "hand", np.int32, kind, 15) for kind in snr.ID_KINDS] + [
    ("hand_min0", "hand", np.int32, "ascending", 0),
    ("hand_u8", "hand", np.uint8, "reversed", 15),
    ("voronoi_64x96", (64, 96, 20, 2), np.int32, "ascending", 15),
    ("voronoi_64x96_dup_u16", (64, 96, 20, 2), np.uint16, "duplicates", 15),
    ("voronoi_48x64_min3", (48, 64, 14, 9), np.int16, "subset", 3),
]


def planes(source, dtype):
    cell, nuc = snr.hand_plane()[:2] if source == "hand" else snr.voronoi_case(*source)
    return cell.astype(dtype), nuc.astype(dtype)


def split_cases(out):
    out["split_names"] = np.array([c[0] for c in SPLIT_CASES])
    for name, source, dtype, kind, min_size in SPLIT_CASES:
        cell, nuc = planes(source, dtype)
        ids = snr.ids_of(kind, cell, np.random.default_rng(24))
        got = ref_utils.split_large_nuclei(cell, nuc, ids, min_size=min_size)
        assert got.dtype == nuc.dtype and int(got.max()) > int(nuc.max()), name        # every case splits something
        p = "s_%s_" % name
        out[p + "cell"], out[p + "nuc"], out[p + "ids"] = cell, nuc, ids
        out[p + "min_size"], out[p + "out"] = np.array(min_size), got


def table_case(out):
    """Case 0 in the layout of g17_cases.npz (make_golden_cell_table.run_case): two FOVs of 40 x 70, uint16 x 2."""
    rs = np.random.RandomState(24)
    h, w, c = 40, 70, 2
    fovs, channels = ["fov0", "fov1"], ["chan0", "chan1"]
    images = {f: base._image(rs, h, w, c, np.uint16) for f in fovs}
    hand_cell, hand_nuc, _ = snr.hand_plane()
    cell0, nuc0 = np.zeros((h, w), np.int32), np.zeros((h, w), np.int32)
    cell0[:hand_cell.shape[0]], nuc0[:hand_nuc.shape[0]] = hand_cell, hand_nuc
    cell1, nuc1 = snr.voronoi_case(h, w, 12, 5)
    segs = {"fov0_whole_cell.tiff": cell0, "fov0_nuclear.tiff": nuc0, "fov1_whole_cell.tiff": cell1.astype(np.int32),
            "fov1_nuclear.tiff": nuc1.astype(np.int32)}
    with tempfile.TemporaryDirectory() as td:
        tiff_dir, seg_dir = os.path.join(td, "tiffs"), os.path.join(td, "seg")
        for fov, img in images.items():
            os.makedirs(os.path.join(tiff_dir, fov, "TIFs"))
            for k, ch in enumerate(channels):
                base._write_tiff(os.path.join(tiff_dir, fov, "TIFs", ch + ".tiff"), np.ascontiguousarray(img[:, :, k]))
        os.makedirs(seg_dir)
        for name, seg in segs.items():
            base.image_io.write_image(os.path.join(seg_dir, name), seg)
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter("always")
            norm, asinh = base.mq.generate_cell_table(seg_dir, tiff_dir, fovs=None, extraction="total_intensity",
                                                      nuclear_counts=True, split_large_nuclei=True, fast_extraction=True,
                                                      mask_types=["whole_cell"], add_underscore=True)
            plain, _ = base.mq.generate_cell_table(seg_dir, tiff_dir, fovs=None, extraction="total_intensity",
                                                   nuclear_counts=True, fast_extraction=True, mask_types=["whole_cell"],
                                                   add_underscore=True)
    assert not np.array_equal(norm["label_nuclear"].to_numpy(), plain["label_nuclear"].to_numpy())   # the flag acts
    p = "c0_"
    out["n_cases"] = np.array(1)
    out[p + "fovs"], out[p + "channels"] = np.array(fovs), np.array(channels)
    for fov in fovs:
        out[p + "img_" + fov] = images[fov]
    out[p + "seg_names"] = np.array(sorted(segs))
    for name, seg in segs.items():
        out[p + "seg_" + name] = seg
    out[p + "extraction"], out[p + "threshold"] = np.array("total_intensity"), np.array(0.0)
    out[p + "nuclear_counts"], out[p + "mask_types"] = np.array(True), np.array(["whole_cell"])
    out[p + "add_underscore"] = np.array(True)
    out[p + "warnings"] = np.array([str(x.message) for x in wl if "found in the following image" in str(x.message)])
    uninit = np.asarray(norm["cell_size_nuclear"] == 0)
    out[p + "uninit"] = uninit
    for tag, df in (("norm", norm), ("asinh", asinh)):
        cols = list(df.columns)
        assert cols[-2:] == ["fov", "mask_type"], cols
        vals = df[cols[:-2]].to_numpy(dtype=np.float64)
        nuc_ch = [k for k, col in enumerate(cols[:-2]) if col.endswith("_nuclear") and col not in (
            "cell_size_nuclear", "label_nuclear", "centroid-0_nuclear", "centroid-1_nuclear")]
        vals[np.ix_(uninit, nuc_ch)] = 0        # the reference leaves these uninitialised: 0 here, excluded by the tests
        out[p + tag + "_columns"] = np.array(cols)
        out[p + tag + "_dtypes"] = np.array([str(t) for t in df.dtypes])
        out[p + tag + "_values"] = vals
        out[p + tag + "_fov"] = df["fov"].to_numpy().astype(str)
        out[p + tag + "_mask_type"] = df["mask_type"].to_numpy().astype(str)
        out[p + tag + "_index"] = np.asarray(df.index, dtype=np.int64)


def main():
    out = {}
    split_cases(out)
    table_case(out)
    path = os.path.join(OUT_DIR, "g24_split_nuclei.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, base.ROOT), len(out), "arrays")


if __name__ == "__main__":
    main()
