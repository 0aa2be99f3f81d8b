#!/usr/bin/env python
"""Generates tests/golden/g21_*.npz: object masks of the REFERENCE's
ark.segmentation.ez_seg.ez_object_segmentation._create_object_mask and ark.utils.masking_utils.create_cell_mask, imported
from /root/reference/src with tests/golden/_shims, as make_golden_cell_masks.py does.

scikit-image is absent from this image, so the six skimage functions the reference calls are restated here with
scipy.ndimage and numpy, under their documented semantics, and injected as modules before the import (the shims under
_shims stay as they are):
  - filters.gaussian(image, sigma, preserve_range=True): float32 / float64 stay, any other dtype becomes float64;
    scipy's gaussian_filter with mode="nearest", truncate 4.0
  - filters.threshold_local(image, block_size): the default method "gaussian", offset 0, mode "reflect":
    gaussian_filter(image, (block_size - 1) / 6) in the image's float dtype
  - morphology.remove_small_holes(ar, area_threshold): connectivity 1; background components of fewer than
    area_threshold pixels become True; a boolean result
  - measure.label(image, connectivity): scipy.ndimage.label with generate_binary_structure(2, connectivity)
  - measure.regionprops_table(label_image, properties=["label", "area"]): the labels present, ascending, and their pixels
  - util.map_array(input, input_vals, output_vals): a lookup, 0 where a value is not listed
Parity with skimage itself is therefore UNPINNED (as for pyFlowSOM and find_boundaries): every fixture carries these
restated calls.  The fixtures hold inputs, parameters, expected int32 masks and the two signatures as text -- no reference
text.

    python tests/golden/make_golden_object_masks.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed files.
"""
import inspect
import json
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")

import scipy.ndimage as ndi  # noqa: E402

OUT_DIR = os.environ.get("PXSOM_GOLDEN_OUT", HERE)


def save(name, **arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", os.path.relpath(path, ROOT), {k: getattr(v, "shape", None) for k, v in arrays.items()})


# ---- the restated skimage functions -------------------------------------------------------------------------------------
def _float_plane(image):
    image = np.asarray(image)
    return image if image.dtype in (np.float32, np.float64) else image.astype(np.float64)


def gaussian(image, sigma=1, *, mode="nearest", cval=0, preserve_range=False, truncate=4.0):
    assert preserve_range
    image = _float_plane(image)
    output = np.empty_like(image)
    ndi.gaussian_filter(image, sigma, output=output, mode=mode, cval=cval, truncate=truncate)
    return output


def threshold_local(image, block_size=3, method="gaussian", offset=0, mode="reflect", param=None, cval=0):
    assert method == "gaussian" and param is None and block_size % 2 == 1
    image = _float_plane(image)
    thresh_image = np.zeros(image.shape, dtype=image.dtype)
    ndi.gaussian_filter(image, (block_size - 1) / 6.0, output=thresh_image, mode=mode, cval=cval)
    return thresh_image - offset


def remove_small_holes(ar, area_threshold=64, connectivity=1):
    out = np.logical_not(np.asarray(ar).astype(bool))
    ccs, _ = ndi.label(out, structure=ndi.generate_binary_structure(out.ndim, connectivity))
    too_small = np.bincount(ccs.ravel()) < area_threshold
    out[too_small[ccs]] = False
    return np.logical_not(out)


def label(label_image, background=None, return_num=False, connectivity=None):
    image = np.asarray(label_image)
    assert image.dtype == bool or set(np.unique(image)) <= {0, 1}
    conn = image.ndim if connectivity is None else connectivity
    return ndi.label(image != 0, structure=ndi.generate_binary_structure(image.ndim, conn))[0]


def regionprops_table(label_image, intensity_image=None, properties=("label", "bbox"), *, cache=True, separator="-"):
    assert list(properties) == ["label", "area"]
    counts = np.bincount(np.asarray(label_image).ravel())
    labels = np.nonzero(counts[1:])[0] + 1
    return {"label": labels, "area": counts[labels].astype(np.float64)}


def map_array(input_arr, input_vals, output_vals, out=None):
    lut = np.zeros(int(max(input_arr.max(), input_vals.max() if len(input_vals) else 0)) + 1, dtype=output_vals.dtype)
    lut[input_vals] = output_vals
    return lut[input_arr]


def inject():
    """Registers skimage.filters / .morphology / .measure / .util beside the shim package, and imports the reference."""
    import skimage
    for name, members in (("filters", dict(gaussian=gaussian, threshold_local=threshold_local)),
                          ("morphology", dict(remove_small_holes=remove_small_holes)),
                          ("measure", dict(label=label, regionprops_table=regionprops_table)),
                          ("util", dict(map_array=map_array))):
        mod = types.ModuleType("skimage." + name)
        mod.__dict__.update(members)
        sys.modules["skimage." + name] = mod
        setattr(skimage, name, mod)
    # the package's own __init__ pulls in its display and merge modules (matplotlib, more of skimage): a bare package
    # module in its place lets the two modules wanted here import on their own
    import ark.segmentation
    pkg = types.ModuleType("ark.segmentation.ez_seg")
    pkg.__path__ = [os.path.join(os.path.dirname(ark.segmentation.__file__), "ez_seg")]
    sys.modules["ark.segmentation.ez_seg"] = pkg
    from ark.segmentation.ez_seg import ez_object_segmentation
    from ark.utils import masking_utils
    return ez_object_segmentation, masking_utils


# ---- inputs -------------------------------------------------------------------------------------------------------------
def blob_image(rs, h, w, n_blobs, dtype):
    """Bumps of several sizes on a background of exact zeros, some with a dent in the middle (holes after the
    threshold), multiplicative noise."""
    yy, xx = np.mgrid[:h, :w]
    img = np.zeros((h, w))
    for _ in range(n_blobs):
        cy, cx, r = rs.randint(0, h), rs.randint(0, w), rs.uniform(2.0, 9.0)
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        bump = np.where(d2 < r * r, 40.0 * (1.0 - d2 / (r * r)) + 5.0, 0.0)
        if rs.rand() < 0.5:
            bump[d2 < (0.4 * r) ** 2] = 0.0
        img += bump
    img *= rs.uniform(0.7, 1.3, size=img.shape)
    return np.round(img).astype(dtype) if np.dtype(dtype).kind in "iu" else img.astype(dtype)


CASES = [  # (name, image, sigma, thresh, hole_size, fov_dim, min_object_area, max_object_area)
    ("none_none", "f32", 1, None, None, 100, 10, 100000),
    ("none_int", "f32", 1, None, 20, 100, 10, 100000),
    ("none_auto", "f32", 1, None, "auto", 100, 10, 100000),
    ("pct_none", "f32", 1, 60, None, 100, 10, 100000),
    ("pct_int", "f32", 2, 35, 12, 100, 5, 100000),
    ("pct_auto", "f32", 1, 60, "auto", 100, 10, 100000),
    ("auto_none", "f32", 1, "auto", None, 100, 10, 100000),
    ("auto_int", "f32", 2, "auto", 15, 100, 4, 100000),
    ("auto_auto", "f32", 1, "auto", "auto", 100, 10, 100000),
    ("no_blur", "f32", None, None, 6, 100, 1, 100000),
    ("area_range", "f32", 1, "auto", None, 100, 104, 205),      # drops the first, the last and middle labels
    ("f64_pct", "f64", 1.5, 50, 10, 200, 8, 100000),
    ("f64_auto", "f64", 1, "auto", "auto", 200, 8, 100000),
    ("u16_pct", "u16", 1, 40, 10, 100, 8, 100000),
    ("u16_auto", "u16", 1, "auto", None, 100, 8, 5000),
    ("odd_shape", "odd", 1, 55, 9, 77, 3, 100000),
    ("empty", "zeros", 1, None, "auto", 100, 10, 100000),
    ("empty_auto", "zeros", 1, "auto", 5, 100, 10, 100000),
    # (an all-zero image under a percentile threshold: the reference's np.percentile of nothing raises IndexError)
]


def g21_object_masks(ez, mu):
    rs = np.random.RandomState(211)
    images = {"f32": blob_image(rs, 96, 128, 40, np.float32), "f64": blob_image(rs, 80, 72, 25, np.float64),
              "u16": blob_image(rs, 64, 90, 25, np.uint16), "odd": blob_image(rs, 37, 53, 12, np.float32),
              "zeros": np.zeros((24, 31), np.float32)}
    out = {"img_" + k: v for k, v in images.items()}
    meta = []
    for name, key, sigma, thresh, hole, fov_dim, lo, hi in CASES:
        mask = ez._create_object_mask(images[key].copy(), "blob", sigma, thresh, hole, fov_dim, lo, hi)
        assert mask.dtype == np.int32
        out["mask_" + name] = mask
        meta.append(dict(name=name, image=key, sigma=sigma, thresh=thresh, hole_size=hole, fov_dim=fov_dim,
                         min_object_area=lo, max_object_area=hi))
    out["cases"] = np.array(json.dumps(meta))
    out["signatures"] = np.array(json.dumps({
        "_create_object_mask": [[p.name, repr(p.default)] for p in inspect.signature(ez._create_object_mask).parameters.values()],
        "create_object_masks": [[p.name, repr(p.default)] for p in inspect.signature(ez.create_object_masks).parameters.values()],
        "get_block_size": [[p.name, repr(p.default)] for p in inspect.signature(ez.get_block_size).parameters.values()],
        "generate_signal_masks": [[p.name, repr(p.default)] for p in inspect.signature(mu.generate_signal_masks).parameters.values()],
        "create_cell_mask": [[p.name, repr(p.default)] for p in inspect.signature(mu.create_cell_mask).parameters.values()],
        "generate_cell_masks": [[p.name, repr(p.default)] for p in inspect.signature(mu.generate_cell_masks).parameters.values()],
    }))
    blocks = [(bt, fd, n, ez.get_block_size(bt, fd, n)) for bt in ("small_holes", "local_thresh")
              for fd in (400, 800, 100, 77) for n in (2048, 1024, 512, 96, 37)]
    out["block_sizes"] = np.array(json.dumps(blocks))
    save("g21_object_masks", **out)


def g21_cell_mask(ez, mu):
    """create_cell_mask on the segmentations of g15_saved_masks: the default sigma 10, and a small sigma with small holes
    and a minimum area, so that the mask is not simply everything."""
    g15 = np.load(os.path.join(HERE, "g15_saved_masks.npz"))
    table = pd.DataFrame({"fov": g15["table_fov"], "label": g15["table_label"],
                          "cell_meta_cluster": g15["table_cluster"]})
    out = {}
    for fov in ("fov0", "fov1"):
        seg = g15["seg_" + fov]
        out["default_" + fov] = mu.create_cell_mask(seg, table, fov, ["cd4", "tumor"])
        out["small_" + fov] = mu.create_cell_mask(seg, table, fov, ["cd8", "Bcell"], sigma=0.6, min_object_area=12,
                                                  max_hole_area=6)
        out["none_" + fov] = mu.create_cell_mask(seg, table, fov, ["no_such_type"], sigma=1)
    save("g21_cell_mask", **out)


if __name__ == "__main__":
    ez, mu = inject()
    steps = {"object_masks": g21_object_masks, "cell_mask": g21_cell_mask}
    for name in (sys.argv[1:] or list(steps)):
        steps[name](ez, mu)
