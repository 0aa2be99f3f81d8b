"""``ark.segmentation.ez_seg.ez_seg_utils``: the plain-text log the ez_seg functions leave behind (``log_creator``: one
``name: value`` line per entry, values formatted by ``str``) and ``renumber_masks``, which makes the labels of a folder
of mask TIFFs unique across the folder (the lookup runs on the device: som_device.segmentation_mask)."""
import pathlib

import numpy as np


def log_creator(variables_to_log: dict, base_dir: str, log_name: str = "config_values.txt"):
    """Writes the entries of ``variables_to_log`` to ``base_dir/log_name``, replacing the file, and says where."""
    target = pathlib.Path(base_dir, log_name)
    target.write_text("".join("%s: %s\n" % item for item in variables_to_log.items()))
    print("Values saved to %s" % target)


def _lookup_device(img: np.ndarray, old: np.ndarray, new: np.ndarray) -> np.ndarray:
    """``img`` with every value of ``old`` (sorted, unique) replaced by its entry of ``new``, in the image's dtype:
    som_device.segmentation_mask with the (old -> new) table.  The one device entry of renumber_masks (the CPU tests
    swap it for numpy's searchsorted)."""
    import torch
    from ... import _capi, som_device
    dev = _capi.require_gpu()
    seg = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    table = som_device.segmask_table(old, new, dev)
    return som_device.segmentation_mask(seg, table=table, unassigned=0).cpu().numpy()


def renumber_table(values: np.ndarray, start: int):
    """What the reference's in-place loop ``for label in unique(img): img[img == label] = counter; counter += 1`` makes
    of each of the image's sorted unique ``values`` (0 skipped), simulated on that vector: a label the counter has
    already handed out is met again later in the loop and renumbered again, together with the class that took it.
    Returns ``(new values, counter after the image)``."""
    current = np.array(values, dtype=np.int64)
    counter = int(start)
    for label in np.array(values, dtype=np.int64).tolist():
        if label != 0:
            current[current == label] = counter
            counter += 1
    return current, counter


def renumber_masks(mask_dir):
    """Relabels every ``*.tiff`` under ``mask_dir`` (recursively) in place so that labels are unique across the folder:
    numbering starts one past the number of non-zero labels of all images, and goes image by image, label by label in
    ascending order -- including the reference's in-place quirk (:func:`renumber_table`).  A number that does not fit
    the image's dtype is a ValueError (the reference wraps silently)."""
    from ... import image_io
    from ...host_utils import validate_paths
    root = pathlib.Path(mask_dir)
    validate_paths(root)
    counter = 1
    for path in root.rglob("*.tiff"):
        values = np.unique(image_io.read_image(str(path)))
        counter += int(np.count_nonzero(values))
    for path in root.rglob("*.tiff"):
        img = image_io.read_image(str(path))
        if img.dtype.kind not in "iu" or img.dtype.itemsize > 4 or img.dtype == np.uint32:
            raise ValueError("renumber_masks: %s holds %s pixels; a uint8, int16, uint16 or int32 mask is needed"
                             % (path, img.dtype))
        old = np.unique(img)
        new, counter = renumber_table(old, counter)
        if np.count_nonzero(old) and counter - 1 > np.iinfo(img.dtype).max:       # (the largest number handed out)
            raise ValueError("renumber_masks: label %d does not fit the %s pixels of %s"
                             % (counter - 1, img.dtype, path))
        if np.count_nonzero(old):
            img = _lookup_device(img, old.astype(np.int32), new.astype(np.int32)).astype(img.dtype, copy=False)
        image_io.write_image(str(path), img)
    print("Relabeling Complete.")
