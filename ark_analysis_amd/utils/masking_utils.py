"""``ark.utils.masking_utils``: signal masks from summed channels and cell masks from the cells of chosen phenotypes,
both through ``_create_object_mask`` (ark_analysis_amd.segmentation.ez_seg.ez_object_segmentation) on the device.
The membership test of ``create_cell_mask`` (``np.isin(seg, labels)``) is pxsom_segmask's lookup."""
import os

import numpy as np

from .. import distributed, image_io
from ..host_utils import list_files, list_folders, remove_file_extensions, validate_paths, verify_in_list
from ..segmentation.ez_seg.ez_object_segmentation import _create_object_mask
from . import data_utils

_CELL_TYPE = "cell_meta_cluster"        # ark.settings.CELL_TYPE


def _total_composite(img_dir, fov, channels) -> np.ndarray:
    """composite_builder(images_to_add=channels, images_to_subtract=[], image_type='total', composite_method='total') for
    one FOV: the float32 sum of the channels (a single channel: that channel as float32)."""
    names = image_io.channel_names(img_dir, fov, '')
    verify_in_list(images_to_add=channels, image_names=names)
    stack = np.ascontiguousarray(image_io.read_channels(img_dir, fov, list(channels), ''), dtype=np.float32)
    if len(channels) > 1:
        return stack.sum(axis=-1)        # numpy's order for a contiguous float32 axis, as the reference's array has it
    return np.ascontiguousarray(stack[..., 0])


def generate_signal_masks(img_dir, mask_dir, channels, mask_name, intensity_thresh_perc="auto",
                          sigma=2, min_object_area=5000, max_hole_area=1000):
    """One signal mask per FOV of ``img_dir`` from the summed ``channels``, saved as ``<mask_dir>/<fov>/<mask_name>.tiff``.
    Under a process group (torchrun) the FOVs are dealt out by rank."""
    validate_paths([img_dir])
    fovs = list_folders(img_dir)
    first_fov_channels = remove_file_extensions(list_files(os.path.join(img_dir, fovs[0])))
    verify_in_list(input_channels=channels, all_channels=first_fov_channels)
    distributed.init_from_env()
    for fov in distributed.shard(fovs):
        total = _total_composite(img_dir, fov, channels)
        _save(mask_dir, fov, mask_name,
              _create_object_mask(total, "blob", sigma, intensity_thresh_perc, max_hole_area, 400, min_object_area, total.size))
    distributed.barrier()


def _save(mask_dir, fov, mask_name, mask) -> None:
    """``<mask_dir>/<fov>/<mask_name>.tiff``, the folder made if it is missing."""
    folder = os.path.join(mask_dir, fov)
    os.makedirs(folder, exist_ok=True)
    data_utils.save_fov_mask(mask_name, folder, mask)


def _isin_device(seg_mask: np.ndarray, cell_labels) -> np.ndarray:
    """``np.isin(seg_mask, cell_labels).astype(np.int32)`` through pxsom_segmask's lookup (labels of the device dtypes;
    the CPU tests swap it for numpy)."""
    keys = np.unique(np.asarray(cell_labels).astype(np.int64))
    if seg_mask.dtype not in data_utils._DEVICE_DTYPES or keys.size == 0 or keys[0] < -2 ** 31 or keys[-1] >= 2 ** 31:
        return np.isin(seg_mask, cell_labels).astype(np.int32)
    if seg_mask.dtype.itemsize > 4 and seg_mask.size and (seg_mask.min() < -2 ** 31 or seg_mask.max() >= 2 ** 31):
        return np.isin(seg_mask, cell_labels).astype(np.int32)      # (the lookup compares int32 casts)
    table = (keys.astype(np.int32), np.ones(keys.size, dtype=np.int32))
    return data_utils._segmask_device(seg_mask, table=table, unassigned=0, out_dtype=np.int32)


def create_cell_mask(seg_mask, cell_table, fov_name, cell_types, cluster_col=_CELL_TYPE,
                     sigma=10, min_object_area=0, max_hole_area=1000):
    """A 0 / 1 int32 mask of the cells of ``fov_name`` whose ``cluster_col`` is in ``cell_types``: their pixels, blurred
    with ``sigma``, everything above 0 kept, holes below ``max_hole_area`` filled, objects below ``min_object_area`` dropped."""
    wanted = (cell_table["fov"] == fov_name) & cell_table[cluster_col].isin(cell_types)
    labels = cell_table.loc[wanted, "label"].to_numpy()
    seg = np.asarray(seg_mask)
    member = _isin_device(seg, labels) if seg.ndim == 2 and seg.size else np.isin(seg, labels).astype(np.int32)
    # no threshold: everything the blur reaches counts; the one area bound left is the minimum
    objects = _create_object_mask(member, "blob", sigma, None, max_hole_area, 0, min_object_area,
                                  member.shape[0] * member.shape[1])
    return (objects > 0).astype(np.int32)


def generate_cell_masks(seg_dir, mask_dir, cell_table, cell_types, mask_name,
                        cluster_col=_CELL_TYPE, sigma=10, min_object_area=0,
                        max_hole_area=1000):
    """One cell mask (create_cell_mask) per FOV of ``cell_table``, from ``<seg_dir>/<fov>_whole_cell.tiff``, saved as
    ``<mask_dir>/<fov>/<mask_name>.tiff``.  Under a process group (torchrun) the FOVs are dealt out by rank."""
    distributed.init_from_env()
    for fov in distributed.shard(np.unique(cell_table.fov)):
        seg = np.squeeze(data_utils._read_segmentation(seg_dir, fov, "_whole_cell.tiff"))
        _save(mask_dir, fov, mask_name,
              create_cell_mask(seg, cell_table, fov, cell_types, cluster_col, sigma, min_object_area, max_hole_area))
    distributed.barrier()
