"""``ark.segmentation.ez_seg.merge_masks``: merging ez_seg object masks into the cell segmentation.  Every object takes
the cell it overlaps most -- among the cells whose centroid lies in the object's bounding box grown by
``expansion_factor`` and of which more than ``overlap_thresh`` percent lie inside the object -- and the cells taken leave
the cell mask.  Both relabellings, the overlap counts and the write pass run on the device (som_device.merge_masks:
pxsom_label_regions, pxsom_pair_overlaps, pxsom_merge_apply); the choice over the few thousand overlapping pairs is made
on the host in the reference's float64 statements; paths, the TIFFs and the log stay on the host.

``skimage.morphology.label`` and ``regionprops_table`` are taken by their documented semantics (regions of equal value
under the 8-neighbourhood, numbered in raster order of their first pixel; centroid = mean of the pixel coordinates;
half-open bounding boxes); parity with skimage itself is unpinned.  The merged TIFF is int32 here."""
import os
import pathlib

import numpy as np

from ... import distributed, image_io
from .ez_seg_utils import log_creator


# ---- the device entries (the CPU tests swap these three for the numpy statement of the same contract) -------------------
def _to_device(mask: np.ndarray):
    """A host mask, checked by :func:`_label_plane`, as an HBM plane."""
    import torch
    from ... import _capi
    return torch.from_numpy(mask if mask.flags.writeable else mask.copy()).to(_capi.require_gpu())


def _merge_device(object_plane, cell_plane, overlap_thresh, expansion_factor):
    """som_device.merge_masks on two HBM planes -> (merged, remaining) int32 HBM planes."""
    from ... import som_device
    return som_device.merge_masks(object_plane, cell_plane, overlap_thresh, expansion_factor)


def _to_host(plane) -> np.ndarray:
    return plane.cpu().numpy()


_LABEL_DTYPES = ("uint8", "int16", "uint16", "int32", "uint32", "int64")


def _label_plane(mask, what: str) -> np.ndarray:
    """``mask`` as a contiguous array of a dtype the device labels.  Integer masks go as they are (bool, int8 and
    uint64 widened where the values allow); a mask of another dtype is accepted when every value is integral and fits
    int32 (the reference's own test passes float64 planes) and becomes int32."""
    mask = np.asarray(mask)
    if mask.dtype.name in _LABEL_DTYPES:
        return np.ascontiguousarray(mask)
    if mask.dtype == np.bool_:
        return np.ascontiguousarray(mask, dtype=np.uint8)
    if mask.dtype.kind in "iu":
        if mask.size == 0 or (mask.min() >= -2 ** 63 and mask.max() <= 2 ** 63 - 1):
            return np.ascontiguousarray(mask, dtype=np.int64)
    elif mask.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            whole = np.isfinite(mask) & (mask == np.trunc(mask)) & (mask >= -2 ** 31) & (mask <= 2 ** 31 - 1)
        if whole.all():
            return np.ascontiguousarray(mask, dtype=np.int32)
    raise ValueError("%s of dtype %s cannot be read as labels: an integer dtype, or integral values within int32, "
                     "is needed" % (what, mask.dtype))


def _merge_planes(object_mask, cell_plane, overlap_thresh, object_name, mask_save_path, expansion_factor):
    """merge_masks_single with the cell mask already on the device, and the remaining cells left there."""
    object_mask = _label_plane(object_mask, "object_mask")
    if tuple(cell_plane.shape) != object_mask.shape:
        raise ValueError("Both masks must have the same shape")
    if object_mask.ndim != 2:
        raise ValueError("masks must be 2-D images, got shape %s" % (object_mask.shape,))
    if object_mask.size == 0:
        merged, remaining = np.zeros(object_mask.shape, np.int32), cell_plane
    else:
        merged, remaining = _merge_device(_to_device(object_mask), cell_plane, overlap_thresh, expansion_factor)
        merged = _to_host(merged)
    name = object_name[:-len(".tiff")] if object_name.endswith(".tiff") else object_name
    image_io.write_image(os.path.join(mask_save_path, name + "_merged.tiff"), merged.astype(np.int32, copy=False))
    return remaining


def merge_masks_seq(fov_list, object_list, object_mask_dir, cell_mask_dir, cell_mask_suffix, overlap_percent_threshold,
                    expansion_factor, save_path, log_dir) -> None:
    """For every FOV, merges the object masks ``<object_mask_dir>/<fov>_<object>.tiff`` of ``object_list``, in that
    order, with the cell mask ``<cell_mask_dir>/<fov>_<cell_mask_suffix>.tiff``: the cells one object type leaves are the
    cell mask of the next (relabelled again there), and stay in HBM in between.  Writes ``<fov>_<object>_merged.tiff``
    per object type and ``<fov>_final_<cell_mask_suffix>_remaining.tiff`` (int32) to ``save_path``, and the arguments to
    ``<log_dir>/mask_merge_log.txt``.  Under a process group (torchrun) the FOVs are dealt out by rank and rank 0 writes
    the log."""
    object_mask_dir, cell_mask_dir, save_path = (pathlib.Path(p) if isinstance(p, str) else p
                                                 for p in (object_mask_dir, cell_mask_dir, save_path))
    rank, _ = distributed.init_from_env()

    for fov in distributed.shard(fov_list):
        cells = _label_plane(image_io.read_image(os.path.join(cell_mask_dir, "%s_%s.tiff" % (fov, cell_mask_suffix))),
                             "cell_mask")
        names = ["%s_%s.tiff" % (fov, obj) for obj in object_list]
        cell_plane = _to_device(cells) if cells.size else cells
        for name in names:
            object_mask = image_io.read_image(os.path.join(object_mask_dir, name))
            cell_plane = _merge_planes(object_mask, cell_plane, overlap_percent_threshold, name, save_path, expansion_factor)
        remaining = _to_host(cell_plane) if cells.size else cells
        image_io.write_image(os.path.join(save_path, "%s_final_%s_remaining.tiff" % (fov, cell_mask_suffix)),
                             remaining.astype(np.int32))

    if rank == 0:
        log_creator({"fov_list": fov_list, "object_list": object_list, "object_mask_dir": object_mask_dir,
                     "cell_mask_dir": cell_mask_dir, "cell_mask_suffix": cell_mask_suffix,
                     "overlap_percent_threshold": overlap_percent_threshold, "save_path": save_path},
                    log_dir, "mask_merge_log.txt")
    distributed.barrier()
    print("Merged masks built and saved")


def merge_masks_single(object_mask, cell_mask, overlap_thresh, object_name, mask_save_path, expansion_factor) -> np.ndarray:
    """Merges one object mask with one cell mask (2-D arrays of one shape).  Both are relabelled (regions of equal value,
    8-neighbourhood, raster order).  Objects are taken in ascending label; each takes, among the cells whose centroid
    lies within its closed bounding box grown by ``expansion_factor``, the one with the largest overlap for which
    ``overlap / cell area > overlap_thresh / 100`` (both compares strict: a tie keeps the smaller cell label, no overlap
    never merges).  The object labels with every taken cell painted in its object's label (the last object, when several
    took it) are saved as ``<object_name without .tiff>_merged.tiff`` (int32) in ``mask_save_path``; the relabelled cell
    mask without the taken cells is returned (int32)."""
    cell_mask = _label_plane(cell_mask, "cell_mask")
    if cell_mask.shape != np.shape(object_mask):
        raise ValueError("Both masks must have the same shape")
    cell_plane = _to_device(cell_mask) if cell_mask.size else cell_mask
    remaining = _merge_planes(object_mask, cell_plane, overlap_thresh, object_name, mask_save_path, expansion_factor)
    return _to_host(remaining) if cell_mask.size else remaining.astype(np.int32)


def get_bounding_boxes(object_labels) -> dict:
    """label -> ((min row, min column), (max row, max column)), closed, for every non-zero label of a label image."""
    labels = np.asarray(object_labels)
    boxes = {}
    for lab in np.unique(labels[labels != 0]).tolist():
        rows, cols = np.nonzero(labels == lab)
        boxes[lab] = ((int(rows.min()), int(cols.min())), (int(rows.max()), int(cols.max())))
    return boxes


def filter_labels_in_bbox(bounding_box, cell_props, expansion_factor) -> list:
    """The ``label`` entries of ``cell_props`` (a table with the columns ``label``, ``centroid-0``, ``centroid-1``)
    whose centroid lies within the closed box ``((min row, min column), (max row, max column))`` grown by
    ``expansion_factor`` on every side."""
    (min_row, min_col), (max_row, max_col) = bounding_box
    rows, cols = np.asarray(cell_props["centroid-0"]), np.asarray(cell_props["centroid-1"])
    inside = ((rows >= min_row - expansion_factor) & (rows <= max_row + expansion_factor) &
              (cols >= min_col - expansion_factor) & (cols <= max_col + expansion_factor))
    return np.asarray(cell_props["label"])[inside].tolist()
