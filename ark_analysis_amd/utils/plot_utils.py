"""``ark.utils.plot_utils`` (the reference's ark/utils/plot_utils.py): the parts the notebooks run without a figure --
``tif_overlay_preprocess``, ``create_overlay``, ``MetaclusterColormap`` and ``save_colored_masks`` -- and an array-level
entry of our own, :func:`overlay_image`.

The overlay runs on the device: torch maxima, a radix select for the 5th and 95th percentile of each
channel's positive pixels, and one streaming pass (pxsom_overlay_rgb) that tests the borders of both segmentations,
rescales up to three channels to uint8 and composites.  The reference makes a sort, two morphology passes per
segmentation and several masked assignments over the full image.  skimage's ``rescale_intensity`` is taken as recalled
(0.19): clip to ``in_range``, ``(x - lo) / (hi - lo) * 255.0 + 0.0``, numpy's truncating cast; with ``lo == hi`` a second
clip to 0 .. 255 instead of the division.  The arithmetic is numpy 2's for the image's dtype.

Stated deviations: a channel whose maximum is not 0 but which has no positive pixel raises ValueError naming the channel
(the reference fails inside ``np.percentile``); plane dtypes other than uint8 / int16 / uint16 / int32 / float32 and label
dtypes other than uint8 .. int64 take the same statement in numpy on the host; what a NaN pixel becomes is unspecified
(its cast to uint8 is undefined in numpy too).  ``save_colored_masks`` refuses a mask value outside the colour table with
IndexError, negative ones included, which numpy would wrap.

Not mirrored: the matplotlib figures (``plot_cluster``, ``plot_pixel_cell_cluster``, ``cohort_cluster_plot``, ...),
``create_mantis_dir``, ``color_segmentation_by_stat`` and ``save_colored_mask`` (matplotlib's normalisation)."""
import os
import pathlib
from dataclasses import dataclass, field
from typing import Any, Dict, List, Literal, Tuple, Union

import numpy as np
import pandas as pd

from .. import image_io
from ..host_utils import validate_paths, verify_in_list, verify_same_elements

_DEVICE_PLANE_DTYPES = ("uint8", "int16", "uint16", "int32", "float32")
_DEVICE_LABEL_DTYPES = ("uint8", "int16", "uint16", "int32", "uint32", "int64")
_DEVICE_MASK_DTYPES = ("uint8", "int16", "uint16", "int32")


def tif_overlay_preprocess(segmentation_labels, plotting_tif):
    """Validates ``plotting_tif`` and lays it out as ``[H, W, 3]`` in its own dtype: a 2-D image goes to blue, channel ``i``
    of a 3-D one to byte ``2 - i``."""
    if len(plotting_tif.shape) == 2:
        if plotting_tif.shape != segmentation_labels.shape:
            raise ValueError("plotting_tif and segmentation_labels array dimensions not equal.")
        formatted_tif = np.zeros((plotting_tif.shape[0], plotting_tif.shape[1], 3), dtype=plotting_tif.dtype)
        formatted_tif[..., 2] = plotting_tif
    elif len(plotting_tif.shape) == 3:
        if plotting_tif.shape[2] > 3:
            raise ValueError("max 3 channels of overlay supported, got {}".format(plotting_tif.shape))
        formatted_tif = np.zeros((plotting_tif.shape[0], plotting_tif.shape[1], 3), dtype=plotting_tif.dtype)
        formatted_tif[..., :plotting_tif.shape[2]] = plotting_tif
        formatted_tif = np.flip(formatted_tif, axis=2)
    else:
        raise ValueError("plotting tif must be 2D or 3D array, got {}".format(plotting_tif.shape))
    return formatted_tif


# ---- device entry points (the CPU tests swap them for the numpy statement of the same contract) ---------------------
def _upload(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def _overlay_device(channels, seg, alt, want_rgb, want_borders, channel_names):
    """som_device.overlay_rgb: host planes in, ``(rgb, borders)`` host arrays out (None where not wanted)."""
    from .. import _capi, som_device
    dev = _capi.require_gpu()
    seg_d = _upload(seg, dev)
    if not want_rgb:
        return None, som_device.overlay_rgb(None, seg_d).cpu().numpy()
    got = som_device.overlay_rgb([_upload(c, dev) for c in channels], seg_d, None if alt is None else _upload(alt, dev),
                                 want_borders=want_borders, channel_names=channel_names)
    rgb, borders = got if want_borders else (got, None)
    return rgb.cpu().numpy(), None if borders is None else borders.cpu().numpy()


def _colorize_device(mask, table):
    """som_device.colorize: a host mask and uint8 table in, ``(image, status)`` out."""
    from .. import _capi, som_device
    dev = _capi.require_gpu()
    out, status = som_device.colorize(_upload(mask, dev), _upload(table, dev))
    return out.cpu().numpy(), status


# ---- the same statement on the host, for the dtypes the device does not read ----------------------------------------
def _inner_boundaries(seg):
    h, w = seg.shape
    pad = np.pad(seg, 1, mode="edge")
    edge = np.zeros(seg.shape, dtype=bool)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        edge |= pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != seg
    return edge & (seg != 0)


def _rescale_uint8(plane, lo, hi):
    lo, hi = float(lo), float(hi)
    plane = np.clip(plane, lo, hi)
    if lo != hi:
        plane = (plane - lo) / (hi - lo)
        return np.asarray(plane * 255.0 + 0.0, dtype=np.uint8)
    return np.clip(plane, 0.0, 255.0).astype(np.uint8)


def _positive_percentiles(plane, name):
    """``(lo, hi)`` of a channel whose maximum is not 0; the stated refusal when it has no positive pixel."""
    kept = plane[plane > 0]
    if kept.size == 0:
        raise ValueError("channel %s has a non-zero maximum but no positive pixel: its percentiles are undefined" % (name,))
    return np.percentile(kept, [5, 95])


def _overlay_host(channels, seg, alt, want_rgb, want_borders, channel_names):
    edge = _inner_boundaries(seg)
    rgb = None
    if want_rgb:
        rgb = np.zeros(seg.shape + (3,), dtype=np.uint8)
        for i, plane in enumerate(channels):
            if np.max(plane) == 0:
                continue
            lo, hi = _positive_percentiles(plane, channel_names[i] if channel_names is not None else i)
            rgb[:, :, 2 - i] = _rescale_uint8(plane, lo, hi)
        rgb[edge, :] = 255
        if alt is not None:
            alt_edge = _inner_boundaries(alt)
            rgb[alt_edge, 0] = 255
            rgb[alt_edge, 1:] = 0
    return rgb, (edge.astype(np.uint8) * np.uint8(255)) if want_borders else None


def _label_plane(a, what):
    a = np.asarray(a)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("%s must be a non-empty [H, W] label plane, got shape %s" % (what, a.shape))
    return a


def _overlay(channels, seg, alt, want_rgb, want_borders, channel_names=None):
    on_device = (seg.dtype.name in _DEVICE_LABEL_DTYPES and (alt is None or alt.dtype.name in _DEVICE_LABEL_DTYPES)
                 and all(c.dtype.name in _DEVICE_PLANE_DTYPES for c in channels)
                 and len({c.dtype for c in channels}) <= 1)
    return (_overlay_device if on_device else _overlay_host)(channels, seg, alt, want_rgb, want_borders, channel_names)


def _overlay_image(plotting_tif, segmentation_labels, alternate_segmentation, channel_names, want_borders):
    """``(overlay, borders)`` of :func:`overlay_image`; the border plane of the segmentation comes from the same pass."""
    plotting_tif = np.asarray(plotting_tif)
    seg = _label_plane(segmentation_labels, "segmentation_labels")
    if plotting_tif.ndim == 2:
        if plotting_tif.shape != seg.shape:
            raise ValueError("plotting_tif and segmentation_labels array dimensions not equal.")
        channels = [plotting_tif]
    elif plotting_tif.ndim == 3:
        if plotting_tif.shape[2] > 3:
            raise ValueError("max 3 channels of overlay supported, got {}".format(plotting_tif.shape))
        if plotting_tif.shape[:2] != seg.shape:
            raise ValueError("plotting_tif and segmentation_labels array dimensions not equal.")
        channels = [np.ascontiguousarray(plotting_tif[..., i]) for i in range(plotting_tif.shape[2])]
    else:
        raise ValueError("plotting tif must be 2D or 3D array, got {}".format(plotting_tif.shape))
    alt = None
    if alternate_segmentation is not None:
        alt = np.asarray(alternate_segmentation)
        if seg.shape != alt.shape:
            raise ValueError("segmentation_labels and alternate_segmentation array dimensions not equal.")
    return _overlay(channels, seg, alt, True, want_borders, channel_names)


def overlay_image(plotting_tif, segmentation_labels, alternate_segmentation=None, channel_names=None):
    """The overlay of ``create_overlay`` from arrays: ``plotting_tif`` ``[H, W]`` or ``[H, W, c]`` (``c <= 3``),
    ``segmentation_labels`` ``[H, W]`` and an optional second segmentation -> uint8 ``[H, W, 3]``.  Every channel with a
    non-zero maximum is rescaled from the 5th .. 95th percentile of its positive pixels to 0 .. 255, the inner borders of
    the segmentation are white, those of the alternate segmentation red.  ``channel_names`` only names the channels in
    the error for a channel without a positive pixel.  A NaN pixel gives an unspecified byte."""
    return _overlay_image(plotting_tif, segmentation_labels, alternate_segmentation, channel_names, False)[0]


def segmentation_borders(segmentation_labels):
    """``find_boundaries(labels, connectivity=1, mode="inner")`` as the uint8 plane the notebooks save: 255 on a border."""
    seg = _label_plane(segmentation_labels, "segmentation_labels")
    return _overlay([], seg, None, False, True)[1]


def _read_labels(path):
    return np.squeeze(image_io.read_tiff_shaped(path))


def _create_overlay(fov, segmentation_dir, data_dir, img_overlay_chans, seg_overlay_comp, alternate_segmentation, want_borders):
    """``(overlay, borders)`` of :func:`create_overlay`."""
    page_names = ["nuclear_channel", "membrane_channel"]
    pages = image_io.read_stack(os.path.join(data_dir, fov + ".tiff"))
    if pages.shape[0] != len(page_names):
        raise ValueError("%s.tiff must hold the two pages %s, got %d" % (fov, page_names, pages.shape[0]))
    verify_in_list(provided_channels=img_overlay_chans, img_channels=page_names)
    compartments = {"whole_cell": fov + "_whole_cell.tiff", "nuclear": fov + "_nuclear.tiff"}
    labels = {name: _read_labels(os.path.join(segmentation_dir, f)) for name, f in compartments.items()}
    verify_in_list(provided_compartments=seg_overlay_comp, seg_compartments=list(compartments))
    chans = [str(c) for c in np.asarray(img_overlay_chans).reshape(-1)]
    plotting_tif = np.stack([pages[page_names.index(c)] for c in chans], axis=-1)
    return _overlay_image(plotting_tif, labels[str(seg_overlay_comp)], alternate_segmentation, chans, want_borders)


def create_overlay(fov, segmentation_dir, data_dir, img_overlay_chans, seg_overlay_comp, alternate_segmentation=None):
    """The channels ``img_overlay_chans`` (of ``nuclear_channel``, ``membrane_channel``: the two pages of
    ``<data_dir>/<fov>.tiff``) under the borders of the compartment ``seg_overlay_comp`` (``whole_cell`` or ``nuclear``:
    ``<segmentation_dir>/<fov>_whole_cell.tiff`` / ``<fov>_nuclear.tiff``) -> uint8 ``[H, W, 3]``; the borders of
    ``alternate_segmentation`` are drawn red over them."""
    return _create_overlay(fov, segmentation_dir, data_dir, img_overlay_chans, seg_overlay_comp, alternate_segmentation, False)[0]


@dataclass
class MetaclusterColormap:
    """The colormap-related information for the metaclusters (the reference's dataclass): the cluster id -> name table
    with the rows "Unassigned" (largest id + 1) and "Empty" (0), ``mc_colors`` sorted by ``cluster_id`` so that colours
    align with mask integers, and matplotlib's ``cmap`` / ``norm`` over them.  ``metacluster_colors`` -- the caller's dict
    -- gains the two added colours."""
    cluster_type: str
    cluster_id_to_name_path: Union[str, pathlib.Path]
    metacluster_colors: Dict

    unassigned_color: Tuple[float, ...] = field(init=False)
    unassigned_id: int = field(init=False)
    background_color: Tuple[float, ...] = field(init=False)
    metacluster_id_to_name: pd.DataFrame = field(init=False)
    mc_colors: np.ndarray = field(init=False)
    cmap: Any = field(init=False)
    norm: Any = field(init=False)

    def __post_init__(self) -> None:
        self.unassigned_color = (0.9, 0.9, 0.9, 1.0)
        self.background_color = (0.0, 0.0, 0.0, 1.0)
        self._metacluster_cmap_generator()

    def _metacluster_cmap_generator(self) -> None:
        from matplotlib import colors
        cluster_id_to_name = pd.read_csv(self.cluster_id_to_name_path)
        t = self.cluster_type
        verify_in_list(required_cols=[f"{t}_som_cluster", f"{t}_meta_cluster", f"{t}_meta_cluster_rename", "cluster_id"],
                       cluster_mapping_cols=cluster_id_to_name.columns.values)
        id_to_name = cluster_id_to_name[[f"{t}_meta_cluster", f"{t}_meta_cluster_rename", "cluster_id"]].copy()
        unassigned_meta_cluster = int(id_to_name[f"{t}_meta_cluster"].max() + 1)
        unassigned_cluster_id = int(id_to_name["cluster_id"].max() + 1)
        id_to_name = pd.concat([
            id_to_name.drop_duplicates(),
            pd.DataFrame(data={f"{t}_meta_cluster": [unassigned_meta_cluster, 0],
                               f"{t}_meta_cluster_rename": ["Unassigned", "Empty"],
                               "cluster_id": [unassigned_cluster_id, 0]})])
        self.metacluster_colors.update({unassigned_meta_cluster: self.unassigned_color})
        self.metacluster_colors.update({0: self.background_color})
        verify_same_elements(metacluster_colors_ids=list(self.metacluster_colors.keys()),
                             metacluster_mapping_ids=id_to_name[f"{t}_meta_cluster"].values)
        id_to_name["color"] = id_to_name[f"{t}_meta_cluster"].map(self.metacluster_colors)
        id_to_name.sort_values(by="cluster_id", inplace=True)
        id_to_name.reset_index(drop=True, inplace=True)
        mc_colors = np.array(id_to_name["color"].to_list())
        self.cmap = colors.ListedColormap(mc_colors)
        self.norm = colors.BoundaryNorm(np.linspace(0, len(mc_colors), len(mc_colors) + 1) - 0.5, len(mc_colors))
        self.metacluster_id_to_name = id_to_name
        self.mc_colors = mc_colors
        # (the reference declares unassigned_id and never sets it)


def color_table(mc_colors) -> np.ndarray:
    """``(mc_colors * 255.999).astype(np.uint8)``: the conversion is elementwise, so it is made once per table row and the
    device gathers bytes."""
    mc_colors = np.asarray(mc_colors)
    if mc_colors.ndim != 2 or mc_colors.shape[0] < 1 or mc_colors.shape[1] not in (3, 4) or mc_colors.dtype.kind != "f":
        raise ValueError("mc_colors must be a float [n, 3] or [n, 4] array, got %s %s" % (mc_colors.dtype, mc_colors.shape))
    return np.ascontiguousarray((mc_colors * 255.999).astype(np.uint8))


def colored_mask(mask, mc_colors) -> np.ndarray:
    """``(mc_colors[mask] * 255.999).astype(np.uint8)`` for a 2-D integer mask -> uint8 ``[H, W, 3 | 4]``.  IndexError for
    a mask value outside ``[0, len(mc_colors))``: negative values are refused although numpy would wrap them."""
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.size == 0 or mask.dtype.kind not in "iu":
        raise ValueError("mask must be a non-empty 2-D integer array, got %s %s" % (mask.dtype, mask.shape))
    table = color_table(mc_colors)
    if mask.dtype.name in _DEVICE_MASK_DTYPES:
        out, status = _colorize_device(mask, table)
        bad = status != 0
    else:
        bad = int(mask.min()) < 0 or int(mask.max()) >= table.shape[0]
        out = None if bad else table[mask]
    if bad:
        raise IndexError("the mask holds a value outside the colour table's rows 0 .. %d" % (table.shape[0] - 1))
    return out


def save_colored_masks(fovs: List[str], mask_dir: Union[str, pathlib.Path], save_dir: Union[str, pathlib.Path],
                       cluster_id_to_name_path: Union[str, pathlib.Path], metacluster_colors: Dict,
                       cluster_type: Literal["cell", "pixel"]) -> None:
    """Converts the pixie TIFF masks ``<mask_dir>/<fov>_<cluster_type>_mask.tiff`` into coloured TIFF masks
    ``<save_dir>/<fov>_<cluster_type>_mask_colored.tiff`` with the colours of :class:`MetaclusterColormap`."""
    verify_in_list(provided_cluster_type=[cluster_type], valid_cluster_types=["pixel", "cell"])
    mask_dir, save_dir = pathlib.Path(mask_dir), pathlib.Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    validate_paths([mask_dir, save_dir])
    mcc = MetaclusterColormap(cluster_type=cluster_type, cluster_id_to_name_path=cluster_id_to_name_path,
                              metacluster_colors=metacluster_colors)
    for fov in fovs:
        mask = np.squeeze(image_io.read_image(str(mask_dir / f"{fov}_{cluster_type}_mask.tiff")))
        image_io.write_rgb(str(save_dir / f"{fov}_{cluster_type}_mask_colored.tiff"), colored_mask(mask, mcc.mc_colors))
