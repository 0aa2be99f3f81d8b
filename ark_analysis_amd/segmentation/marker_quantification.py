"""``ark.segmentation.marker_quantification.generate_cell_table`` (the reference's
ark/segmentation/marker_quantification.py:455-593): one row per cell with its size, its channel values
(``total_intensity``, ``positive_pixel`` or ``center_weighting``), its label and centroid, optionally the same for the
nucleus that overlaps it most, then the FOV and the mask type -- normalised by cell size, and arcsinh-transformed.
With ``fast_extraction=False`` and at least one of ``regionprops_base``, ``regionprops_single_comp`` and
``regionprops_multi_comp`` named, the morphology columns stand between the label and the FOV: area, eccentricity, the
axis lengths, perimeter, convex_area, equivalent_diameter, the six derived ratios and ``nc_ratio``.

The per-cell reduction of the ``[H, W, C]`` image is one pxsom_cellquant pass per (FOV, compartment) on the device
(DESIGN.md K12): it returns counts, exact coordinate sums and the channel values in numpy's own summation order.  The
two transforms (``size_norm``, ``arcsinh``) and the frame layout stay on the host in numpy.  The morphology comes from
one pxsom_region_shape and one pxsom_region_hull pass per compartment: raw integers from the device,
the float columns from regionprops_extraction on the host; skimage is taken by its documented algorithms and parity
with skimage itself is not pinned.  The bare call (``fast_extraction=False`` with none of the three lists named) keeps
raising NotImplementedError, as do MIBItiff inputs and a base property outside the built ones
(regionprops_extraction.BUILT_BASE; ``orientation`` and ``euler_number`` came with DESIGN.md K23);
``create_marker_count_matrices`` / ``compute_marker_counts`` are not mirrored (they take and return xarray).
``split_large_nuclei=True`` re-cuts the nuclear plane at the cell borders on the device before anything nuclear is
computed (segmentation_utils.split_large_nuclei); it needs ``nuclear_counts=True``."""
import concurrent.futures
import warnings

import numpy as np
import pandas as pd

from .. import distributed, image_io
from ..host_utils import list_folders, remove_file_extensions, verify_in_list
from ..utils import data_utils
from . import regionprops_extraction as rpe
from . import segmentation_utils

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
    ``sums`` [n, 2], ``bbox`` [n, 4], ``values`` [n, C] and, with ``nuc``, ``nuc_keys`` and ``nuc`` (index into
    ``nuc_keys``, -1: none).  ``_device`` keeps the uploaded label image and the device tables for :func:`_region_raw`."""
    import torch
    from .. import som_device
    dev = image_dev.device

    def up(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
    seg_dev = up(seg)
    got = som_device.cell_quantify(seg_dev, image_dev, mode=mode, threshold=threshold,
                                   nuc=up(nuc) if nuc is not None else None)
    out = {k: v.cpu().numpy() for k, v in got.items()}
    out["_device"] = dict(seg=seg_dev, keys=got["keys"], count=got["count"], sums=got["sums"], bbox=got["bbox"])
    return out


def _region_raw(seg, q=None, euler=False, **thresholds) -> dict:
    """pxsom_region_shape and pxsom_region_hull over one compartment: a host label image in, the raw integers of
    som_device.region_props out as host arrays, the cells the device leaves out filled by the host route.  With the
    result ``q`` of :func:`_quantify` over the same label image, its uploaded image, key table, counts, sums and boxes
    are reused: no second upload, no second key table, and the shape pass skips the statistics atomics.  ``euler`` adds
    ``euler`` (one pxsom_region_euler pass), which only the ``euler_number`` column needs."""
    import torch
    from .. import _capi, som_device
    kept = q.get("_device") if q is not None else None
    if kept is not None:
        seg_dev = kept["seg"]
        got = som_device.region_props(seg_dev, keys=kept["keys"], count=kept["count"], sums=kept["sums"],
                                      bbox=kept["bbox"], **thresholds)
    else:
        dev = _capi.require_gpu()
        a = np.ascontiguousarray(seg)
        seg_dev = torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
        got = som_device.region_props(seg_dev, **thresholds)
    if euler:
        got["euler"] = som_device.region_euler(seg_dev, keys=got["keys"])
    raw = {k: v.cpu().numpy() for k, v in got.items()}
    return rpe.fill_left_out(raw, seg, **thresholds)


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


def _raw_rows(q, n_channels, morph=None):
    """(cell_size, channels, label, then centroid-0, centroid-1 or the morphology block ``morph``) of a quantify result
    as a float64 [n, C + 2 + ...] block."""
    keys = np.asarray(q["keys"], dtype=np.int64)
    count = np.asarray(q["count"], dtype=np.int64)
    sums = np.asarray(q["sums"], dtype=np.int64).reshape(-1, 2)
    tail = 2 if morph is None else morph.shape[1]
    out = np.zeros((keys.size, n_channels + 2 + tail), dtype=np.float64)
    out[:, 0] = count
    out[:, 1:1 + n_channels] = np.asarray(q["values"], dtype=np.float64).reshape(-1, n_channels)
    out[:, 1 + n_channels] = keys
    if morph is not None:
        out[:, 2 + n_channels:] = morph
    elif keys.size:
        out[:, 2 + n_channels] = sums[:, 0] / count     # coords.mean(axis=0): exact integer sums, one division
        out[:, 3 + n_channels] = sums[:, 1] / count
    return out


def _transforms(raw, n_channels):
    """(size_norm, arcsinh of size_norm) of one compartment's raw block (transform_expression_matrix): channels divided
    by cell_size where it is > 0 -- 0 where it is not (the reference leaves those entries uninitialised) -- then
    arcsinh(x * 100).  The other columns, the morphology among them, pass through."""
    ch = slice(1, 1 + n_channels)
    norm = raw.copy()
    size = raw[:, :1]
    norm[:, ch] = np.divide(raw[:, ch], size, out=np.zeros_like(raw[:, ch]), where=size > 0)
    asinh = norm.copy()
    asinh[:, ch] = np.arcsinh(norm[:, ch] * LINEAR_FACTOR)
    return norm, asinh


def _morph_block(seg, q, props):
    """The morphology columns of one compartment as a float64 [n, len(names)] block in the table's order
    (regionprops_extraction.table_names), rows in the order of the quantify result ``q``."""
    base, single, _, thresholds = props
    raw = _region_raw(seg, q, euler="euler_number" in base, **thresholds)
    if not np.array_equal(np.asarray(raw["keys"], dtype=np.int64), np.asarray(q["keys"], dtype=np.int64)):
        raise RuntimeError("generate_cell_table: the morphology pass and the signal pass name different cells")
    names = rpe.table_names(base, single)
    cols = rpe.morphology(raw, orientation="orientation" in names)
    block = np.zeros((np.asarray(raw["keys"]).size, len(names)), dtype=np.float64)
    for j, name in enumerate(names):
        block[:, j] = cols[name]
    return block


def get_single_compartment_props(segmentation_labels, regionprops_base, regionprops_single_comp, **kwargs):
    """The reference's get_single_compartment_props without ``coords``: one row per cell of a ``[H, W]`` label image,
    labels ascending -- the base properties in list order (``centroid`` as ``centroid-0``, ``centroid-1`` in its place),
    then the single-compartment ones; ``kwargs`` may set num_concavities' three thresholds.  An all-background image
    gives an empty frame with the same columns."""
    base, single, _ = rpe.resolve_lists(regionprops_base, regionprops_single_comp, [])
    seg = _as_label_plane(segmentation_labels, "segmentation_labels")
    return rpe.props_frame(_region_raw(seg, euler="euler_number" in base, **rpe.concavity_thresholds(**kwargs)), base,
                           single)


def _fov_frames(fov, image_dev, channels, segs, mask_types, add_underscore, nuclear_counts, mode, threshold,
                props=None, split_nuclei=False):
    """The (size-normalised, arcsinh) frames of one FOV, one pair per mask type, from its segmentations ``segs``
    (mask file suffix -> label plane).  ``props`` (base, single, multi, thresholds) adds the morphology columns.  With
    ``split_nuclei`` the nuclear plane of the whole_cell mask type is re-cut first (every cell label, ascending) and
    everything nuclear -- the signal, the morphology and each cell's nucleus -- is computed from the re-cut plane."""
    tail = BASE_NAMES[1:] if props is None else rpe.table_names(props[0], props[1])
    frames = []
    for mask_type in mask_types:
        names = [PRE_CHANNEL_COL] + list(channels) + [POST_CHANNEL_COL] + tail
        mask_type, mask_suff = _mask_name(mask_type, add_underscore)
        compartments = ["whole_cell"]
        if nuclear_counts and mask_type == "whole_cell":
            compartments = ["whole_cell", "nuclear"]
        if nuclear_counts:         # create_marker_count_matrices' check
            verify_in_list(nuclear_label="nuclear", compartment_names=compartments)
        seg = segs[mask_suff]
        nuc = segs["_nuclear"] if nuclear_counts else None
        if split_nuclei and nuc is not None and mask_type == "whole_cell":
            cell_ids = np.unique(seg)
            nuc = segmentation_utils.split_large_nuclei(seg, nuc, cell_ids[cell_ids != 0])
        q = _quantify(image_dev, seg, mode, threshold, nuc=nuc)
        if np.asarray(q["keys"]).size == 0:
            warnings.warn("No cells found in the following image: {}".format(fov))
        raw = _raw_rows(q, len(channels), None if props is None else _morph_block(seg, q, props))
        rows = None
        if nuclear_counts:
            qn = _quantify(image_dev, nuc, mode, threshold)
            if np.asarray(qn["keys"]).size == 0:
                warnings.warn("No nuclei found in the following image: {}".format(fov))
            nuc_raw = _raw_rows(qn, len(channels), None if props is None else _morph_block(nuc, qn, props))
            which = np.asarray(q["nuc"], dtype=np.int64)
            rows = np.zeros_like(raw)
            rows[which >= 0] = nuc_raw[which[which >= 0]]
            # nc_ratio: appended to both compartments once a cell of the FOV has a nucleus (the reference adds the
            # feature inside its loop over the cells, so a FOV without any never gets the column)
            if props is not None and "nc_ratio" in props[2] and (which >= 0).any():
                if "area" not in names:
                    raise ValueError("generate_cell_table: nc_ratio needs 'area' in regionprops_base")
                at = names.index("area")
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.nan_to_num(rows[:, at] / raw[:, at], posinf=0, neginf=0)
                raw = np.concatenate((raw, ratio[:, None]), axis=1)
                rows = np.concatenate((rows, ratio[:, None]), axis=1)
                names = names + ["nc_ratio"]
        norm, asinh = _transforms(raw, len(channels))
        norm_df = pd.DataFrame(data=norm, columns=names)
        asinh_df = pd.DataFrame(data=asinh, columns=names)
        norm_df[POST_CHANNEL_COL] = norm_df[POST_CHANNEL_COL].astype(np.int32)
        asinh_df[POST_CHANNEL_COL] = asinh_df[POST_CHANNEL_COL].astype(np.int32)
        if nuclear_counts:
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
    """The reference's generate_cell_table: ``(cell_table_size_normalized, cell_table_arcsinh_transformed)``, FOVs
    sorted, cells in ascending label order, each FOV's frame with its own RangeIndex.  ``signal_kwargs={'threshold': t}``
    sets positive_pixel's threshold (default 0).  A cell without a nucleus keeps a zero ``_nuclear`` row.

    ``fast_extraction=False`` runs once at least one of ``regionprops_base``, ``regionprops_single_comp`` and
    ``regionprops_multi_comp`` is named (a list not named takes the reference's default); the bare call raises
    NotImplementedError.  The columns are then ``cell_size``, the channels, ``label``, the base properties in list order
    with ``centroid-0``, ``centroid-1`` at the end of the base block, the single-compartment properties and, with
    ``nuclear_counts`` in a FOV where some cell has a nucleus, ``nc_ratio``.  ``regionprops_kwargs`` may set
    ``small_concavity_minimum``, ``max_compactness`` and ``large_concavity_minimum``.  With ``fast_extraction=True`` the
    lists are ignored.  ``split_large_nuclei=True`` (with ``nuclear_counts=True``; NotImplementedError without) re-cuts
    the nuclei at the cell borders first, as segmentation_utils.split_large_nuclei does.  Under a process group the FOVs
    are sharded over the ranks and every rank returns the whole table."""
    if is_mibitiff:
        raise NotImplementedError("generate_cell_table: MIBItiff inputs are not implemented; "
                                  "use single-channel TIFFs (is_mibitiff=False)")
    if fovs is None:
        fovs = list_folders(tiff_dir)
    fovs = remove_file_extensions(fovs)
    verify_in_list(extraction=extraction, extraction_options=EXTRACTION_OPTIONS)
    props = None
    if not fast_extraction:
        lists = [kwargs.get(k) for k in ("regionprops_base", "regionprops_single_comp", "regionprops_multi_comp")]
        if all(v is None for v in lists):
            raise NotImplementedError("generate_cell_table: the morphology regionprops of fast_extraction=False (area, "
                                      "perimeter, convex area, concavities, nc_ratio, ...) are not implemented; "
                                      "fast_extraction=True is what runs")
        props = rpe.resolve_lists(*lists) + (rpe.concavity_thresholds(**kwargs.get("regionprops_kwargs", {})),)
    split_nuclei = bool(kwargs.get("split_large_nuclei", False))
    if split_nuclei and not nuclear_counts:
        raise NotImplementedError("generate_cell_table: split_large_nuclei=True needs nuclear_counts=True (without it "
                                  "there is no nuclear plane to split; the reference ignores the flag then)")
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
                                        extraction, thr, props, split_nuclei)
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
