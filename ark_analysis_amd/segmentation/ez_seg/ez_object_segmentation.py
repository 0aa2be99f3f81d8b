"""``ark.segmentation.ez_seg.ez_object_segmentation``: object masks of "blob"-like structures from one channel -- blur,
threshold, fill small holes, label the connected components, drop those outside an area range.  Every step runs on the
device (som_device.object_mask: the plane blur with skimage's "nearest" border, the binarising pass,
pxsom_label_components and pxsom_components_select); paths, the TIFFs and the log stay on the host.

skimage's functions are taken by their documented semantics (``filters.gaussian`` = scipy's gaussian_filter with
mode="nearest" and truncate 4 in float32 / float64, ``threshold_local``'s default Gaussian method,
``remove_small_holes`` with connectivity 1 and a strict <, ``measure.label(connectivity=2)``); parity with skimage itself
is unpinned.

``object_shape_type="projection"`` puts ``filters.meijering(mask, sigmas=range(1, 5), black_ridges=False) > 0`` between the
hole fill and the labelling.  That filter is this project's statement of skimage 0.19's algorithm (som_device.ridge_sign,
DESIGN.md K22), unpinned against skimage, so it is opt-in: with ``PROJECTION_FILTER = None`` (the default) "projection"
raises NotImplementedError as before; ``ez_object_segmentation.PROJECTION_FILTER = "meijering"`` enables it."""
import os

import numpy as np

from ... import distributed, image_io
from ...host_utils import validate_paths, verify_in_list
from .ez_seg_utils import log_creator


# How "projection" objects are filtered: None (refused) or "meijering"; read at call time.
PROJECTION_FILTER = None
_MEIJERING = (range(1, 5, 1), 0.5)         # the reference's sigmas; skimage's alpha = 1 / ndim


def _object_mask_device(img, sigma, thresh, hole_size, min_area, max_area, local_block=None, ridge=None) -> np.ndarray:
    """som_device.object_mask on a host image -> host int32 labels.  The one device entry point of the object masks (the
    CPU tests swap it for the numpy statement of the same contract)."""
    import torch
    from ... import _capi, som_device
    dev = _capi.require_gpu()
    img = np.ascontiguousarray(img)
    if img.dtype not in (np.float32, np.float64):
        img = img.astype(np.float64)           # filters.gaussian(preserve_range=True): "image.astype(float)"
    t = torch.from_numpy(img if img.flags.writeable else img.copy()).to(dev)
    return som_device.object_mask(t, sigma, thresh, hole_size, min_area, max_area, local_block, ridge=ridge).cpu().numpy()


def check_blur_sigma(sigma) -> None:
    from ... import som_device
    som_device.check_blur_sigma(sigma)


_SHAPES = ["blob", "projection"]
# what create_object_masks logs, in this order
_LOGGED = ("image_data_dir", "fov_list", "mask_name", "channel_to_segment", "masks_dir", "object_shape_type", "sigma",
           "thresh", "hole_size", "fov_dim", "min_object_area", "max_object_area")


def create_object_masks(image_data_dir, img_sub_folder, fov_list, mask_name, channel_to_segment, masks_dir, log_dir,
                        object_shape_type="blob", sigma=1, thresh=None, hole_size=None, fov_dim=400, min_object_area=100,
                        max_object_area=100000) -> None:
    """One object mask per FOV from ``channel_to_segment`` (read as float32), saved as
    ``<masks_dir>/<fov>_<mask_name>.tiff``; the arguments are logged to ``<log_dir>/<mask_name>_segmentation_log.txt``.
    A FOV folder that holds a single image is segmented on that image whatever its name.  Under a process group
    (torchrun) the FOVs are dealt out by rank and rank 0 writes the log."""
    settings = dict(locals())           # the call's arguments in signature order: what the log records
    validate_paths([image_data_dir, masks_dir, log_dir])
    verify_in_list(object_shape=[object_shape_type], object_shape_options=_SHAPES)
    rank, _ = distributed.init_from_env()

    for fov in distributed.shard(fov_list):
        present = image_io.channel_names(image_data_dir, fov, img_sub_folder)
        name = present[0] if len(present) == 1 else channel_to_segment
        if name not in present:
            raise KeyError(channel_to_segment)
        plane = image_io.read_channel(image_data_dir, fov, name, img_sub_folder).astype(np.float32)
        mask = _create_object_mask(plane, object_shape_type, sigma, thresh, hole_size, fov_dim, min_object_area,
                                   max_object_area)
        image_io.write_image(os.path.join(masks_dir, "%s_%s.tiff" % (fov, mask_name)), mask)

    if rank == 0:
        logged = {key: settings[key] for key in _LOGGED}
        if object_shape_type == "projection":
            logged["projection_filter"] = PROJECTION_FILTER
        log_creator(logged, log_dir, mask_name + "_segmentation_log.txt")
    distributed.barrier()
    print("ez masks built and saved")


def _create_object_mask(input_image, object_shape_type="blob", sigma=1, thresh=None, hole_size="auto", fov_dim=400,
                        min_object_area=10, max_object_area=100000) -> np.ndarray:
    """The int32 object mask of one 2-D image (an ndarray, or anything with ``to_numpy()``): components of the
    thresholded blur, numbered in raster order of their first pixel, 0 where a component's area is outside
    ``[min_object_area, max_object_area]`` (kept labels are not renumbered).  ``sigma`` None: no blur.  ``thresh``: an
    int percentile of the blur's non-zero values, "auto" (local Gaussian threshold, block from ``get_block_size``) or
    None (everything > 0).  ``hole_size``: background holes below this area are filled; "auto" takes
    ``get_block_size("small_holes", ...)``, None fills nothing."""
    verify_in_list(object_shape_type=[object_shape_type], object_shape_options=_SHAPES)
    ridge = None
    if object_shape_type == "projection":
        if PROJECTION_FILTER is None:
            raise NotImplementedError("object_shape_type 'projection' (skimage's Meijering filter) is not implemented "
                                      "on the device by default: set ez_object_segmentation.PROJECTION_FILTER = "
                                      "'meijering' to take this project's statement of skimage 0.19's filter")
        if PROJECTION_FILTER != "meijering":
            raise ValueError("PROJECTION_FILTER must be None or 'meijering', got %r" % (PROJECTION_FILTER,))
        ridge = _MEIJERING
    image = np.asarray(input_image if isinstance(input_image, np.ndarray) else input_image.to_numpy())
    if image.ndim != 2:
        raise ValueError("input_image must be a 2-D image, got shape %s" % (image.shape,))
    if sigma is not None:
        check_blur_sigma(sigma)

    # bool passes for an int, as isinstance has it in the reference; "auto" sizes come from the image's height
    def is_auto(value):
        return isinstance(value, str) and value == "auto"

    def refuse(what, value):
        raise ValueError("Invalid `%s` value: %s. Must be either `auto`, `None` or an integer." % (what, value))

    local_block = None
    if is_auto(thresh):
        local_block = get_block_size("local_thresh", fov_dim, image.shape[0])
        check_blur_sigma((local_block - 1) / 6.0)
    elif thresh is not None and not isinstance(thresh, int):
        refuse("threshold", thresh)
    holes = get_block_size("small_holes", fov_dim, image.shape[0]) if is_auto(hole_size) else hole_size
    if holes is not None and not isinstance(holes, int):
        refuse("hole_size", hole_size)

    if image.size == 0:
        return np.zeros(image.shape, dtype=np.int32)
    if ridge is None:
        return _object_mask_device(image, sigma, thresh, holes, min_object_area, max_object_area, local_block)
    if min(image.shape) < 2:                # np.gradient's refusal, in its words
        raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements "
                         "are required.")
    return _object_mask_device(image, sigma, thresh, holes, min_object_area, max_object_area, local_block, ridge=ridge)


def get_block_size(block_type, fov_dim, img_shape) -> int:
    """The block size in pixels for ``block_type`` "small_holes" (the area of a 5 um-radius-squared disc, scaled) or
    "local_thresh" (about 10 um, rounded to an odd number), from the FOV's size in um and in pixels."""
    verify_in_list(block_type=[block_type], block_types=["small_holes", "local_thresh"])
    if block_type == "small_holes":
        return round((np.pi * 5) ** 2 / (fov_dim / img_shape))
    block = round(10 / (fov_dim / img_shape))
    return block | 1            # the next odd number when even
