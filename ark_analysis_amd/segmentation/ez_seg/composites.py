"""``ark.segmentation.ez_seg.composites``: composite channels for ez_seg -- channels (or pixel-cluster masks) added
together, others subtracted, as intensities ("total") or as a 0 / 1 mask ("binary").  Host numpy on the ``[H, W, C]``
stacks of image_io.read_channels: a handful of float32 adds per pixel, once per FOV, next to reading the TIFFs."""
import os
import pathlib
from typing import NamedTuple, Sequence

import numpy as np

from ... import image_io
from ...host_utils import verify_in_list
from .ez_seg_utils import log_creator


class ChannelStack(NamedTuple):
    """The channels of one FOV: ``values`` [H, W, C] and the C channel names."""
    values: np.ndarray
    channels: Sequence[str]


def _channel_sum(data: ChannelStack, names) -> np.ndarray:
    """The named channels as float32, summed along the channel axis with ``ndarray.sum`` (one channel: as it is)."""
    present = list(data.channels)
    picked = data.values[:, :, [present.index(name) for name in names]].astype(np.float32)
    return picked.sum(axis=2) if len(names) > 1 else picked[:, :, 0]


def composite_builder(image_data_dir, img_sub_folder, fov_list, images_to_add, images_to_subtract, image_type,
                      composite_method, composite_directory=None, composite_name=None, log_dir=None):
    """One composite per FOV from the channels under ``image_data_dir/<fov>/<img_sub_folder>``: ``images_to_add``
    summed, then ``images_to_subtract`` taken off (:func:`add_to_composite`, :func:`subtract_from_composite`).  With a
    ``composite_directory`` each is saved as ``<composite_directory>/<fov>/<composite_name>.tiff`` (uint32).  With a
    ``log_dir`` the arguments are logged to ``<composite_name>_composite_log.txt``; without one the dictionary
    fov -> float32 composite is returned."""
    composite_images = {}
    for fov in fov_list:
        channels = image_io.channel_names(image_data_dir, fov, img_sub_folder)
        data = ChannelStack(image_io.read_channels(image_data_dir, fov, channels, img_sub_folder), channels)
        verify_in_list(images_to_add=images_to_add, image_names=channels)
        verify_in_list(images_to_subtract=images_to_subtract, image_names=channels)
        verify_in_list(composite_method=composite_method, options=["binary", "total"])

        composite_array = np.zeros(data.values.shape[:2], dtype=np.float32)
        if images_to_add:
            composite_array = add_to_composite(data, composite_array, images_to_add, image_type, composite_method)
        if images_to_subtract:
            composite_array = subtract_from_composite(data, composite_array, images_to_subtract, image_type,
                                                      composite_method)
        if composite_directory:
            fov_dir = pathlib.Path(composite_directory) / fov
            fov_dir.mkdir(parents=True, exist_ok=True)
            image_io.write_image(os.path.join(fov_dir, "%s.tiff" % composite_name), composite_array.astype(np.uint32))
        composite_images[fov] = composite_array.astype(np.float32)

    if not log_dir:
        return composite_images
    log_creator({"image_data_dir": image_data_dir, "fov_list": fov_list, "images_to_add": images_to_add,
                 "images_to_subtract": images_to_subtract, "image_type": image_type,
                 "composite_method": composite_method, "composite_directory": composite_directory,
                 "composite_name": composite_name}, log_dir, "%s_composite_log.txt" % composite_name)
    print("Composites built and saved")


def add_to_composite(data, composite_array, images_to_add, image_type, composite_method) -> np.ndarray:
    """The float32 sum of the channels ``images_to_add`` of ``data`` (a :class:`ChannelStack`), capped at 1 for
    ``image_type`` "pixel_cluster" or ``composite_method`` "binary".  ``composite_array`` is replaced, not added to."""
    composite_array = _channel_sum(data, images_to_add)
    if image_type == "pixel_cluster" or composite_method == "binary":
        composite_array = composite_array.clip(min=None, max=1)
    return composite_array


def subtract_from_composite(data, composite_array, images_to_subtract, image_type, composite_method) -> np.ndarray:
    """``composite_array`` (changed in place) without the channels ``images_to_subtract``: for "signal" data under
    "binary", zero where their float32 sum is positive and capped at 1; otherwise the sum is subtracted and negative
    values become 0."""
    taken = _channel_sum(data, images_to_subtract)
    if image_type == "signal" and composite_method == "binary":
        composite_array[taken > 0] = 0
        composite_array[composite_array > 1] = 1
        return composite_array
    composite_array -= taken
    return composite_array.clip(min=0, max=None)
