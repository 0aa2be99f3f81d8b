"""``ark.segmentation.segmentation_utils`` (the reference's ark/segmentation/segmentation_utils.py): the nucleus of a
cell, nuclei re-cut at cell borders, and the CSV concatenation.

``split_large_nuclei`` runs on the device: one streaming pass counts, per cell, the nucleus with the most
pixels inside it and, per nucleus, its pixels; the choice -- which overlaps get a new label, in the caller's order, and
which labels fall below 5 pixels afterwards -- is made on the host over those short tables; a second pass writes the
plane.  The reference builds two full-image masks per cell instead.  skimage's ``remove_small_objects`` is taken by its
documented behaviour on an integer array (sizes by ``bincount``, no connected components); its "only one label was
provided" warning is not reproduced.

``save_segmentation_labels`` writes the border plane and the channel overlays of every FOV through the one-pass overlay
kernel (``utils/plot_utils.py``).

``transform_expression_matrix`` is not mirrored: it takes and returns an xarray (generate_cell_table applies both
transforms itself)."""
import os

import numpy as np
import pandas as pd

from .. import image_io
from ..host_utils import remove_file_extensions

INT32_MAX = 2 ** 31 - 1


def find_nuclear_label_id(nuc_segmentation_labels, cell_coords):
    """The nuclear label with the most pixels among ``cell_coords`` ([n, 2] rows and columns), the smallest on a tie;
    None when the cell covers no nucleus."""
    ids, counts = np.unique(nuc_segmentation_labels[tuple(cell_coords.T)], return_counts=True)
    if ids[ids != 0].size == 0:
        return None
    return ids[ids != 0][np.argmax(counts[ids != 0])]


# ---- device entry point (the CPU tests swap it for the numpy statement of the same contract) -----------------------
def _split_device(cell, nuc, cell_ids, min_size):
    """som_device.split_large_nuclei: host label planes in, the host nuclear plane out."""
    import torch
    from .. import _capi, som_device
    dev = _capi.require_gpu()

    def up(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
    return som_device.split_large_nuclei(up(cell), up(nuc), cell_ids, min_size=min_size).cpu().numpy()


def _label_plane(a, what):
    """A 2-D integer label plane with labels in 0 .. 2^31 - 1, in a dtype the device reads."""
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError("Only bool or integer image types are supported. Got %s (%s)." % (a.dtype, what))
    if a.ndim != 2 or a.size == 0:
        raise ValueError("%s must be a non-empty [H, W] label plane, got shape %s" % (what, a.shape))
    lo, hi = int(a.min()), int(a.max())
    if lo < 0:
        raise ValueError("%s: negative labels are not supported (smallest: %d)" % (what, lo))
    if hi > INT32_MAX:
        raise ValueError("%s: label %d is past the limit %d" % (what, hi, INT32_MAX))
    if a.dtype == np.int8:
        a = a.astype(np.int16)
    elif a.dtype == np.uint64:
        a = a.astype(np.int64)
    return a, hi


def split_large_nuclei(cell_segmentation_labels, nuc_segmentation_labels, cell_ids, min_size=15):
    """The reference's split_large_nuclei: for every id of ``cell_ids``, in that order (an id named twice is handled
    twice), the nuclear label with the most pixels inside the cell (the smallest on a tie) gets a new label -- one past
    the largest so far -- inside the cell when more than ``min_size`` of its pixels lie outside the cell; then every
    label with fewer than 5 pixels is removed.  Host arrays in, the modified nuclear plane out in its own dtype.

    Raised before any launch: TypeError for a non-integer plane, ValueError for a negative label or one past int32,
    IndexError for a ``cell_ids`` entry that is no label of the cell plane (where the reference fails too).  A
    deviation: where the reference's numpy scalar wraps, ValueError names the dtype that ``max(nuc)`` plus the number of
    splits does not fit; the number is known after the counting pass, so that error comes before the write pass."""
    given = np.asarray(nuc_segmentation_labels).dtype
    cell, _ = _label_plane(cell_segmentation_labels, "cell_segmentation_labels")
    nuc, _ = _label_plane(nuc_segmentation_labels, "nuc_segmentation_labels")
    if cell.shape != nuc.shape:
        raise ValueError("the two planes must have one shape, got %s and %s" % (cell.shape, nuc.shape))
    ids = np.asarray(cell_ids).reshape(-1)
    if ids.size and ids.dtype.kind not in "iu":
        raise TypeError("cell_ids must be integers, got %s" % ids.dtype)
    labels = np.unique(cell)
    known = np.isin(ids, labels[labels != 0])
    if not known.all():
        raise IndexError("split_large_nuclei: cell id %d is no label of the cell segmentation" % int(ids[~known][0]))
    return np.asarray(_split_device(cell, nuc, ids.astype(np.int64), min_size)).astype(given, copy=False)


def concatenate_csv(base_dir, csv_files, column_name="fov", column_values=None):
    """Concatenates the CSV files ``csv_files`` of ``base_dir``, each with ``column_name`` set to its entry of
    ``column_values`` (default: the file name without its extension), into ``<base_dir>/combined_data.csv``."""
    if column_values is None:
        column_values = remove_file_extensions(csv_files)
    if len(column_values) != len(csv_files):
        raise ValueError("csv_files and column_values have different lengths: "
                         "csv {}, column_values {}".format(len(csv_files), len(column_values)))
    combined_data = None
    for idx, file in enumerate(csv_files):
        temp_data = pd.read_csv(os.path.join(base_dir, file), header=0, sep=",")
        temp_data[column_name] = column_values[idx]
        combined_data = temp_data if idx == 0 else pd.concat((combined_data, temp_data), axis=0, ignore_index=True)
    combined_data.to_csv(os.path.join(base_dir, "combined_data.csv"), index=False)


def save_segmentation_labels(segmentation_dir, data_dir, output_dir, fovs, channels=None):
    """For every FOV of ``fovs``: the inner borders of ``<segmentation_dir>/<fov>_whole_cell.tiff`` as
    ``<output_dir>/<fov>_segmentation_borders.tiff`` (uint8, 0 / 255) and, with ``channels`` (of ``nuclear_channel``,
    ``membrane_channel``: the pages of ``<data_dir>/<fov>.tiff``), their overlay under those borders as
    ``<output_dir>/<fov>_<chan>_..._overlay.tiff`` (uint8 RGB).  Both images of a FOV are computed before either file is
    written, so a refusal (``plot_utils.create_overlay``) leaves no file of that FOV behind."""
    from ..utils import plot_utils
    for fov in fovs:
        channel_overlay = None
        if channels is None:
            labels = np.squeeze(image_io.read_tiff_shaped(os.path.join(segmentation_dir, fov + "_whole_cell.tiff")))
            contour_mask = plot_utils.segmentation_borders(labels)
        else:
            chans = np.array(channels)      # (an array, so that chans.astype("str") names the file as the reference does)
            channel_overlay, contour_mask = plot_utils._create_overlay(fov, segmentation_dir, data_dir, chans, "whole_cell",
                                                                       None, True)
        image_io.write_image(os.path.join(output_dir, f"{fov}_segmentation_borders.tiff"), contour_mask)
        if channel_overlay is not None:
            save_path = "_".join([f"{fov}", *chans.astype("str"), "overlay.tiff"])
            image_io.write_rgb(os.path.join(output_dir, save_path), channel_overlay)
