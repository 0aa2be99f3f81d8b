#!/usr/bin/env python
"""Generates tests/golden/g22_merge_masks.npz: merged and remaining masks of the REFERENCE's
ark.segmentation.ez_seg.merge_masks.merge_masks_single, imported from /root/reference/src with tests/golden/_shims, as
make_golden_object_masks.py does.

scikit-image is absent from this image, so the two skimage functions the reference calls are restated here under their
documented semantics and injected as modules before the import:
  - morphology.label(image, return_num=True): regions of equal non-zero value under the full (8-) neighbourhood, numbered
    in raster order of their first pixel -- a flood fill written out here, independent of the scipy statement the tests use
  - measure.regionprops_table(labels, properties=('label', 'centroid')) / ('label', 'bbox'): the labels present,
    ascending; centroid = the mean of the pixel coordinates; bbox half-open (min row, min col, max row + 1, max col + 1)
Parity with skimage itself is therefore UNPINNED (as for g21).  The reference's TIFF writer (alpineer's save_image) is
captured instead of writing a file.  The fixture holds inputs, parameters, both outputs and the signatures as text -- no
reference text.

    python tests/golden/make_golden_merge_masks.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed file.
"""
import inspect
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")

OUT_DIR = os.environ.get("PXSOM_GOLDEN_OUT", HERE)


# ---- the restated skimage functions -------------------------------------------------------------------------------------
def label(label_image, background=None, return_num=False, connectivity=None):
    image = np.asarray(label_image)
    assert image.ndim == 2 and background is None and connectivity is None
    h, w = image.shape
    out = np.zeros((h, w), dtype=np.int64)
    n = 0
    for y in range(h):
        for x in range(w):
            if image[y, x] == 0 or out[y, x]:
                continue
            n += 1
            out[y, x] = n
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for ny in range(max(cy - 1, 0), min(cy + 2, h)):
                    for nx in range(max(cx - 1, 0), min(cx + 2, w)):
                        if not out[ny, nx] and image[ny, nx] == image[y, x]:
                            out[ny, nx] = n
                            stack.append((ny, nx))
    return (out, n) if return_num else out


def regionprops_table(label_image, intensity_image=None, properties=("label", "bbox"), *, cache=True, separator="-"):
    labels = np.asarray(label_image)
    present = np.unique(labels[labels != 0])
    coords = [np.argwhere(labels == lab) for lab in present]
    table = {"label": present}
    if tuple(properties) == ("label", "centroid"):
        means = np.array([c.mean(axis=0) for c in coords], dtype=np.float64).reshape(-1, 2)
        table["centroid-0"], table["centroid-1"] = means[:, 0], means[:, 1]
    else:
        assert tuple(properties) == ("label", "bbox")
        lo = np.array([c.min(axis=0) for c in coords], dtype=np.int64).reshape(-1, 2)
        hi = np.array([c.max(axis=0) + 1 for c in coords], dtype=np.int64).reshape(-1, 2)
        table["bbox-0"], table["bbox-1"], table["bbox-2"], table["bbox-3"] = lo[:, 0], lo[:, 1], hi[:, 0], hi[:, 1]
    return table


def inject():
    """Registers skimage.morphology / .measure beside the shim package, and imports the reference's module."""
    import skimage
    for name, members in (("morphology", dict(label=label)), ("measure", dict(regionprops_table=regionprops_table))):
        mod = types.ModuleType("skimage." + name)
        mod.__dict__.update(members)
        sys.modules["skimage." + name] = mod
        setattr(skimage, name, mod)
    import ark.segmentation
    pkg = types.ModuleType("ark.segmentation.ez_seg")      # (the package's own __init__ pulls in matplotlib)
    pkg.__path__ = [os.path.join(os.path.dirname(ark.segmentation.__file__), "ez_seg")]
    sys.modules["ark.segmentation.ez_seg"] = pkg
    from ark.segmentation.ez_seg import merge_masks
    return merge_masks


# ---- inputs -------------------------------------------------------------------------------------------------------------
def discs(rs, n, radii, values):
    yy, xx = np.mgrid[:96, :96]
    out = np.zeros((96, 96), dtype=np.int32)
    for i in range(n):
        cy, cx, r = rs.randint(0, 96), rs.randint(0, 96), rs.randint(radii[0], radii[1] + 1)
        out[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = values(i)
    return out


CASES = [  # (name, cells, objects, cell radii, object radii, overlap threshold, expansion factor, dtype)
    ("sparse", 40, 8, (3, 6), (5, 10), 10, 5, "int32"),
    ("dense", 160, 25, (2, 5), (4, 9), 30, 2, "uint16"),        # cells paint over cells: pieces, touching values
    ("float", 60, 12, (3, 7), (6, 12), 50, 0, "float64"),       # the reference's own test passes float planes
    ("wide", 90, 30, (2, 4), (3, 6), 0, 40, "int64"),           # threshold 0, a box that takes in half the image
]


def g22(mm):
    rs = np.random.RandomState(221)
    out, meta, saved = {}, [], {}
    mm.image_utils.save_image = lambda fname, data: saved.update({os.path.basename(str(fname)): np.asarray(data)})
    for name, n_cells, n_objects, cell_r, object_r, thresh, grow, dtype in CASES:
        cells = discs(rs, n_cells, cell_r, lambda i: rs.randint(1, n_cells // 2 + 1)).astype(dtype)    # values repeat
        objects = discs(rs, n_objects, object_r, lambda i: 3 * i + 2).astype(dtype)
        remaining = mm.merge_masks_single(objects.copy(), cells.copy(), thresh, name + ".tiff", "unused", grow)
        merged = saved.pop(name + "_merged.tiff")
        assert not saved and merged.shape == (96, 96) and (merged != label(objects)).any()
        out["cells_" + name], out["objects_" + name] = cells, objects
        out["merged_" + name], out["remaining_" + name] = merged.astype(np.int32), np.asarray(remaining).astype(np.int32)
        meta.append(dict(name=name, overlap_thresh=thresh, expansion_factor=grow))
    out["cases"] = np.array(json.dumps(meta))
    out["signatures"] = np.array(json.dumps({
        fn: [[p.name, repr(p.default)] for p in inspect.signature(getattr(mm, fn)).parameters.values()]
        for fn in ("merge_masks_seq", "merge_masks_single", "get_bounding_boxes", "filter_labels_in_bbox")}))
    path = os.path.join(OUT_DIR, "g22_merge_masks.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, ROOT), {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    g22(inject())
