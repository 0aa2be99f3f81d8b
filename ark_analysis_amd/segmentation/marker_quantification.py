"""``ark.segmentation.marker_quantification.generate_cell_table`` (the reference's
ark/segmentation/marker_quantification.py:455-593) under ``fast_extraction=True``: one row per cell with its size, its channel values
(``total_intensity``, ``positive_pixel`` or ``center_weighting``), its label and centroid, optionally the same for the
nucleus that overlaps it most, then the FOV and the mask type -- normalised by cell size, and arcsinh-transformed.

The per-cell reduction of the ``[H, W, C]`` image is one pxsom_cellquant pass per (FOV, compartment) on the device
(DESIGN.md K12): it returns counts, exact coordinate sums and the channel values in numpy's own summation order.  The
two transforms (``size_norm``, ``arcsinh``) and the frame layout stay on the host in numpy.  The morphology regionprops
of ``fast_extraction=False``, MIBItiff inputs and ``split_large_nuclei`` are not implemented (NotImplementedError);
``create_marker_count_matrices`` / ``compute_marker_counts`` are not mirrored (they take and return xarray)."""
import concurrent.futures
import warnings

import numpy as np
import pandas as pd

from .. import distributed, image_io
from ..host_utils import list_folders, remove_file_extensions, verify_in_list
from ..utils import data_utils

EXTRACTION_OPTIONS = ["positive_pixel", "center_weighting", "total_intensity"]   # signal_extraction.EXTRACTION_FUNCTION
PRE_CHANNEL_COL, POST_CHANNEL_COL = "cell_size", "label"                          # ark.settings
BASE_NAMES = ["label", "centroid-0", "centroid-1"]
LINEAR_FACTOR = 100                                                               # transform_expression_matrix's default


def _threshold_for(dtype, threshold) -> float:
    """The threshold of ``img > threshold`` as a binary64 that compares the same way: numpy compares in the promoted
    dtype (a Python float against a float32 image in float32), and every pixel value is exact in binary64."""
    res = np.result_type(dtype, threshold)
    if res.kind == "f":
        return float(res.type(threshold))
    return float(threshold)


# ---- device entry points (the CPU tests swap these for the numpy statement of the same contract) -------------------
def _upload_image(image):
    """Host ``[H, W, C]`` stack -> contiguous device image (planar stacks are interleaved on the device)."""
    from .. import _capi
    from ..flowsom import _image_to_device
    return _image_to_device(image, _capi.require_gpu())


def _quantify(image_dev, seg, mode, threshold, nuc=None) -> dict:
    """pxsom_cellquant over one compartment: host label images in, host tables out -- ``keys`` (the labels), ``count``,
    ``sums`` [n, 2], ``values`` [n, C] and, with ``nuc``, ``nuc_keys`` and ``nuc`` (index into ``nuc_keys``, -1: none)."""
    import torch
    from .. import som_device
    dev = image_dev.device

    def up(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
    got = som_device.cell_quantify(up(seg), image_dev, mode=mode, threshold=threshold,
                                   nuc=up(nuc) if nuc is not None else None)
    return {k: v.cpu().numpy() for k, v in got.items()}


# ---- host side ----------------------------------------------------------------------------------------------------
def _as_label_plane(seg, what) -> np.ndarray:
    """A segmentation file's array as ``[H, W]``: the reference's loader keeps the first plane of a ``(1, H, W)`` stack."""
    seg = np.asarray(seg)
    while seg.ndim > 2 and seg.shape[0] == 1:
        seg = seg[0]
    if seg.ndim != 2:
        raise NotImplementedError("%s: only single-plane segmentations are supported, got shape %s" % (what, seg.shape))
    if seg.dtype.kind not in "iu":
        raise NotImplementedError("%s: integer label images only, got %s" % (what, seg.dtype))
    if seg.dtype == np.int8:
        seg = seg.astype(np.int16)
    elif seg.dtype == np.uint64:
        seg = seg.astype(np.int64)
    return seg


def _raw_rows(q, n_channels):
    """(cell_size, channels, label, centroid-0, centroid-1) of a quantify result as a float64 [n, C + 4] block."""
    keys = np.asarray(q["keys"], dtype=np.int64)
    count = np.asarray(q["count"], dtype=np.int64)
    sums = np.asarray(q["sums"], dtype=np.int64).reshape(-1, 2)
    out = np.zeros((keys.size, n_channels + 4), dtype=np.float64)
    out[:, 0] = count
    out[:, 1:1 + n_channels] = np.asarray(q["values"], dtype=np.float64).reshape(-1, n_channels)
    out[:, 1 + n_channels] = keys
    if keys.size:
        out[:, 2 + n_channels] = sums[:, 0] / count     # coords.mean(axis=0): exact integer sums, one division
        out[:, 3 + n_channels] = sums[:, 1] / count
    return out


def _transforms(raw, n_channels):
    """(size_norm, arcsinh of size_norm) of one compartment's raw block (transform_expression_matrix): channels divided
    by cell_size where it is > 0 -- 0 where it is not (the reference leaves those entries uninitialised) -- then
    arcsinh(x * 100)."""
    ch = slice(1, 1 + n_channels)
    norm = raw.copy()
    size = raw[:, :1]
    norm[:, ch] = np.divide(raw[:, ch], size, out=np.zeros_like(raw[:, ch]), where=size > 0)
    asinh = norm.copy()
    asinh[:, ch] = np.arcsinh(norm[:, ch] * LINEAR_FACTOR)
    return norm, asinh


def _fov_frames(fov, image_dev, channels, segs, mask_types, add_underscore, nuclear_counts, mode, threshold):
    """The (size-normalised, arcsinh) frames of one FOV, one pair per mask type, from its segmentations ``segs``
    (mask file suffix -> label plane)."""
    names = [PRE_CHANNEL_COL] + list(channels) + BASE_NAMES
    frames = []
    for mask_type in mask_types:
        mask_type, mask_suff = _mask_name(mask_type, add_underscore)
        compartments = ["whole_cell"]
        if nuclear_counts and mask_type == "whole_cell":
            compartments = ["whole_cell", "nuclear"]
        if nuclear_counts:         # create_marker_count_matrices' check
            verify_in_list(nuclear_label="nuclear", compartment_names=compartments)
        seg = segs[mask_suff]
        nuc = segs["_nuclear"] if nuclear_counts else None
        q = _quantify(image_dev, seg, mode, threshold, nuc=nuc)
        if np.asarray(q["keys"]).size == 0:
            warnings.warn("No cells found in the following image: {}".format(fov))
        raw = _raw_rows(q, len(channels))
        norm, asinh = _transforms(raw, len(channels))
        norm_df = pd.DataFrame(data=norm, columns=names)
        asinh_df = pd.DataFrame(data=asinh, columns=names)
        norm_df[POST_CHANNEL_COL] = norm_df[POST_CHANNEL_COL].astype(np.int32)
        asinh_df[POST_CHANNEL_COL] = asinh_df[POST_CHANNEL_COL].astype(np.int32)
        if nuclear_counts:
            qn = _quantify(image_dev, nuc, mode, threshold)
            if np.asarray(qn["keys"]).size == 0:
                warnings.warn("No nuclei found in the following image: {}".format(fov))
            nuc_raw = _raw_rows(qn, len(channels))
            which = np.asarray(q["nuc"], dtype=np.int64)
            rows = np.zeros_like(raw)
            rows[which >= 0] = nuc_raw[which[which >= 0]]
            nuc_norm, nuc_asinh = _transforms(rows, len(channels))
            nuc_names = [f + "_nuclear" for f in names]
            norm_df = pd.concat((norm_df, pd.DataFrame(data=nuc_norm, columns=nuc_names)), axis=1)
            asinh_df = pd.concat((asinh_df, pd.DataFrame(data=nuc_asinh, columns=nuc_names)), axis=1)
        for df in (norm_df, asinh_df):
            df["fov"] = fov
            df["mask_type"] = "whole_cell" if mask_type == "final_cells_remaining" else mask_type
        frames.append((norm_df, asinh_df))
    return frames


def _mask_name(mask_type, add_underscore):
    """(mask type, file suffix): None is 'cell_mask' read from ``<fov>.tiff``."""
    if mask_type is None:
        return "cell_mask", ""
    return mask_type, ("_" + mask_type if add_underscore else mask_type)


def _read_fov(segmentation_dir, tiff_dir, img_sub_folder, fov, suffixes):
    """A FOV's ``[H, W, C]`` stack (channels in natural order) and its label planes (file suffix -> plane)."""
    channels = image_io.channel_names(tiff_dir, fov, img_sub_folder)
    image = image_io.read_channels(tiff_dir, fov, channels, img_sub_folder)
    segs = {s: _as_label_plane(data_utils._read_segmentation(segmentation_dir, fov, s + ".tiff"), fov + s + ".tiff")
            for s in suffixes}
    for s, seg in segs.items():
        if seg.shape != image.shape[:2]:
            raise ValueError("segmentation %s has shape %s, the FOV's images %s"
                             % (fov + s + ".tiff", seg.shape, image.shape[:2]))
    return channels, image, segs


def generate_cell_table(segmentation_dir, tiff_dir, img_sub_folder="TIFs", is_mibitiff=False, fovs=None,
                        extraction='total_intensity', nuclear_counts=False, fast_extraction=False,
                        mask_types=['whole_cell'], add_underscore=True, **kwargs):
    """The reference's generate_cell_table under ``fast_extraction=True``: ``(cell_table_size_normalized,
    cell_table_arcsinh_transformed)``, FOVs sorted, cells in ascending label order, each FOV's frame with its own
    RangeIndex.  ``signal_kwargs={'threshold': t}`` sets positive_pixel's threshold (default 0).  A cell without a
    nucleus keeps a zero ``_nuclear`` row.  Under a process group the FOVs are sharded over the ranks and every rank
    returns the whole table."""
    if is_mibitiff:
        raise NotImplementedError("generate_cell_table: MIBItiff inputs are not implemented; "
                                  "use single-channel TIFFs (is_mibitiff=False)")
    if fovs is None:
        fovs = list_folders(tiff_dir)
    fovs = remove_file_extensions(fovs)
    verify_in_list(extraction=extraction, extraction_options=EXTRACTION_OPTIONS)
    if not fast_extraction:
        raise NotImplementedError("generate_cell_table: the morphology regionprops of fast_extraction=False (area, "
                                  "perimeter, convex area, concavities, nc_ratio, ...) are not implemented; "
                                  "fast_extraction=True is what runs")
    if kwargs.get("split_large_nuclei", False):
        raise NotImplementedError("generate_cell_table: split_large_nuclei=True is not implemented")
    threshold = kwargs.get("signal_kwargs", {}).get("threshold", 0)
    fovs = sorted(fovs)
    suffixes = sorted({_mask_name(m, add_underscore)[1] for m in mask_types}
                      | ({"_nuclear"} if nuclear_counts else set()))

    mine = distributed.shard(fovs)
    done, error = {}, None
    try:
        with concurrent.futures.ThreadPoolExecutor(max_workers=1) as reader:
            ahead = reader.submit(_read_fov, segmentation_dir, tiff_dir, img_sub_folder, mine[0], suffixes) \
                if mine else None
            for i, fov in enumerate(mine):
                channels, image, segs = ahead.result()
                ahead = reader.submit(_read_fov, segmentation_dir, tiff_dir, img_sub_folder, mine[i + 1], suffixes) \
                    if i + 1 < len(mine) else None
                image_dev = _upload_image(image)
                thr = _threshold_for(image.dtype, threshold)
                done[fov] = _fov_frames(fov, image_dev, channels, segs, mask_types, add_underscore, nuclear_counts,
                                        extraction, thr)
    except Exception as e:      # noqa: BLE001 -- travels to every rank below, re-raised there
        error = e
    gathered = distributed.allgather_objects((error, done))
    for err, _ in gathered:        # the first rank's error, on every rank
        if err is not None:
            raise err
    frames = {}
    for _, part in gathered:
        frames.update(part)
    pairs = [pair for fov in fovs for pair in frames[fov]]
    if not pairs:
        raise ValueError("No objects to concatenate")
    return pd.concat([p[0] for p in pairs]), pd.concat([p[1] for p in pairs])
