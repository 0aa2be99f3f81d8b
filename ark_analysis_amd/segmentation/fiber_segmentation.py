"""The reference's ``ark.segmentation.fiber_segmentation`` from the segmented mask onward: labelling, the
size filter, the fibre object table, the k-nearest-fibre alignment score and the FOV / tile summaries.

Built here: :func:`fiber_objects` (the tail of ``segment_fibers``: ``ndi.label``, ``remove_small_objects``,
``regionprops_table``), :func:`fiber_object_props`, :func:`fiber_object_table_from_labels` (the cohort call over saved
``<fov>_fiber_labels.tiff`` files, ending as ``run_fiber_segmentation`` ends), :func:`calculate_fiber_alignment`,
:func:`calculate_density`, :func:`generate_tile_stats` and :func:`generate_summary_stats`, with the reference's names,
signatures, defaults, columns, files and errors.

On the device: the labels (pxsom_label_components, pxsom_components_select), the raw integers of every object
(pxsom_region_shape, which streams the plane and has no object-size limit, and pxsom_region_euler) and the neighbours of
the alignment score (pxsom_nearest_indices, one launch for the whole table; the FOV's distance matrix is never built).
The float columns come from ``regionprops_extraction.morphology`` on the host; skimage is taken by its documented
algorithms (``orientation`` as skimage 0.19 states it) and parity with skimage itself is not pinned.  The summaries
are pandas on the host, as in the reference.

Also built: the middle of ``segment_fibers``, from the ridge map (frangi's output) to the two planes the
watershed receives -- :func:`fiber_watershed_inputs`: ``ridges > ridge_cutoff``, ``distance_transform_edt``, the sigma-1
blur, the 256-bin histogram, ``threshold_multiotsu`` on its counts (:func:`threshold_multiotsu_from_histogram`, on the
host), the 0 / 1 / 2 markers, the second blur and ``sobel``.  On the device: pxsom_plane_greater,
pxsom_distance_transform_edt, pxsom_gaussian_blur_plane_mode, pxsom_plane_minmax, pxsom_plane_histogram,
pxsom_class_markers, pxsom_sobel_magnitude.  The distance transform, the blurs, the histogram and the Sobel magnitude are
scipy's / numpy's bits; the multi-Otsu choice on the counts is skimage 0.19's as recalled (``RECALLED_MULTIOTSU``), and
skimage's ``sobel`` sums its 3 x 3 kernel in another order than scipy's separable one: parity with skimage is not pinned.

Also built: the ``frangi`` stage before that middle -- :func:`frangi_ridges`, the ridge map
``frangi(contrast_adjusted, sigmas=fiber_widths, black_ridges=False) * 10000`` in skimage 0.19's 2-D statement as recalled
(np.gradient twice on the reflect-mode blur, the eigenvalues ordered by magnitude, the maximum over the widths), and
:func:`fiber_watershed_inputs_from_contrast`, which runs it and the K25 middle as one chain on the device.  On the device:
pxsom_gaussian_blur_plane_mode and pxsom_frangi_scale, one of each per width.  The blur is scipy's bits; the rest equals
the numpy statement of tests/frangi_reference.py bit for bit, including its own exponential; parity with skimage itself
is not pinned.

Also built: the front -- :func:`contrast_adjusted_channel`, ``equalize_adapthist(b / np.max(b),
kernel_size=fov_len / contrast_scaling_divisor)`` with ``b = gaussian_filter(image, sigma=blur)`` in skimage 0.19's
statement as recalled (2^14 grey levels, 256 bins of 65, clipped tile histograms, four-tile interpolation in float32), and
:func:`fiber_watershed_inputs_from_channel`, which runs the front, the ridge filter and the K25 middle as one chain on
the device.  On the device: pxsom_gaussian_blur_plane_mode, pxsom_plane_minmax, pxsom_plane_divide, pxsom_clahe_quantize
and pxsom_clahe_equalize.  The result equals the numpy statement of tests/clahe_reference.py bit for bit; parity with
skimage itself is not pinned.

Also built: the stage between the middle and the tail -- :func:`watershed_labels`,
``watershed(elevation_map, markers)`` at skimage 0.19's defaults as recalled (``RECALLED_WATERSHED``; pxsom_watershed, the
priority flood computed in parallel rounds) -- and with it the whole of ``segment_fibers`` on one channel plane:
:func:`segment_fiber_channel` does the job of ``segment_fibers`` from its ``fiber_channel_data`` line to its return (the
labels file, the four debug files, the object table), and :func:`run_fiber_channel_segmentation` the job of
``run_fiber_segmentation`` (every FOV folder in natural order, the alignment score, ``fiber_object_table.csv``).  The
channel goes up once and the filtered labels come down; no plane crosses in between.  Parity with skimage itself is not
pinned.

The three entries that carry the reference's own names have not been switched over to these yet, and read as before K28:
Not built: ``watershed`` after the middle.
:func:`segment_fibers` (which takes an xarray), :func:`run_fiber_segmentation` and :func:`plot_fiber_segmentation_steps`
keep the reference's signatures, validate their paths and the channel as the reference does, and then raise
NotImplementedError; call :func:`segment_fiber_channel` and :func:`run_fiber_channel_segmentation` instead (the plots are
not built)."""
import os
from collections import namedtuple
from typing import Dict, Optional

import numpy as np
import pandas as pd

from .. import image_io
from ..host_utils import list_files, list_folders, natsorted, remove_file_extensions, validate_paths, verify_in_list
from . import regionprops_extraction as rpe
from .marker_quantification import _as_label_plane

FOV_ID = "fov"                                                                          # ark.settings
FIBER_OBJECT_PROPS = ("label", "centroid", "major_axis_length", "minor_axis_length", "orientation", "area",
                      "eccentricity", "euler_number")
BUILT_OBJECT_PROPS = FIBER_OBJECT_PROPS      # what fiber_object_props builds: today exactly the default list
NEAREST_MAX_K = 32          # som_device.nearest_indices keeps the k nearest in registers
_LABELS_SUFFIX = "_fiber_labels.tiff"
_TILE_PROPERTIES = ["major_axis_length", "minor_axis_length", "orientation", "area", "eccentricity", "euler_number"]
_UNBUILT = ("the front half of fibre segmentation (equalize_adapthist, frangi, threshold_multiotsu, sobel, watershed) "
            "is not implemented; from a segmented mask use fiber_objects, from saved <fov>_fiber_labels.tiff files "
            "fiber_object_table_from_labels")


# ---- device entry points (the CPU tests swap them for the numpy statements of the same contracts) -------------------
def _nearest_indices_device(xy: np.ndarray, seg: np.ndarray, k: int) -> np.ndarray:
    """som_device.nearest_indices on host arrays: ``xy`` [n, 2] float64, ``seg`` [F + 1] offsets -> [n, k] int32 on the
    host."""
    from .. import som_device
    from ..analysis._cells import _to_device
    return som_device.nearest_indices(_to_device(xy, np.float64), _to_device(seg, np.int64), k).cpu().numpy()


def _region_raw_device(labels: np.ndarray) -> dict:
    """som_device.region_moments and som_device.region_euler over a host label plane: host arrays ``keys``, ``count``,
    ``sums``, ``bbox``, ``shape`` and ``euler``."""
    import torch
    from .. import _capi, som_device
    a = np.ascontiguousarray(labels)
    seg = torch.from_numpy(a if a.flags.writeable else a.copy()).to(_capi.require_gpu())
    got = som_device.region_moments(seg)
    got["euler"] = som_device.region_euler(seg, keys=got["keys"])
    return {name: v.cpu().numpy() for name, v in got.items()}


def _label_and_filter_device(mask: np.ndarray, min_size: int) -> np.ndarray:
    """``ndi.label(mask)`` (4-connected) with the components under ``min_size`` pixels removed, not renumbered: int32."""
    import torch
    from .. import _capi, som_device
    fg = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8)).to(_capi.require_gpu())
    labels, _, areas = som_device.label_components(fg, connectivity=1)
    return som_device.components_select(labels, areas, "keep", min_area=min_size, out=labels).cpu().numpy()


def _watershed_inputs_device(ridges: np.ndarray, ridge_cutoff: float, sobel_blur: float, thresholds):
    """som_device.watershed_inputs on a host ``[H, W]`` float64 plane: host arrays ``(dist, (t0, t1), markers, elevation)``;
    ``thresholds(counts, edges)`` is the host's choice of the two thresholds."""
    import torch
    from .. import _capi, som_device
    plane = torch.from_numpy(np.array(ridges, dtype=np.float64, order="C")).to(_capi.require_gpu())
    dist, t, markers, elevation = som_device.watershed_inputs(plane, ridge_cutoff, sobel_blur, thresholds)
    return dist.cpu().numpy(), t, markers.cpu().numpy(), elevation.cpu().numpy()


def _frangi_device(image: np.ndarray, sigmas, beta: float, gamma: float, scale: float) -> np.ndarray:
    """som_device.frangi on a host ``[H, W]`` float64 plane: the host array ``frangi(image, sigmas, beta, gamma) * scale``."""
    import torch
    from .. import _capi, som_device
    plane = torch.from_numpy(np.array(image, dtype=np.float64, order="C")).to(_capi.require_gpu())
    return som_device.frangi(plane, sigmas, beta, gamma, scale).cpu().numpy()


def _ridge_watershed_inputs_device(contrast: np.ndarray, sigmas, ridge_cutoff: float, sobel_blur: float, thresholds):
    """som_device.ridge_watershed_inputs on a host ``[H, W]`` float64 plane, one upload and one chain on the device: host
    arrays ``(ridges, dist, (t0, t1), markers, elevation)``."""
    import torch
    from .. import _capi, som_device
    plane = torch.from_numpy(np.array(contrast, dtype=np.float64, order="C")).to(_capi.require_gpu())
    ridges, dist, t, markers, elevation = som_device.ridge_watershed_inputs(plane, sigmas, ridge_cutoff, sobel_blur, thresholds)
    return ridges.cpu().numpy(), dist.cpu().numpy(), t, markers.cpu().numpy(), elevation.cpu().numpy()


# ---- from the ridge map to the watershed's inputs (K25) -------------------------------------------------------------------
# Every detail of skimage 0.19's threshold_multiotsu that is recalled, not pinned by an installed skimage, as a named
# switch; the first value of each is the default.
#   prob        "float64": prob = counts / counts.sum() and all sums in binary64; "float32": cast as skimage casts, the
#               sums in float32
#   tie         "first" / "last": which pair (i, j), in row-major order, is taken among those that share the maximal
#               criterion.  Ties are normal: moving a threshold across an empty bin leaves the criterion bit-equal.
#   exact_bins  "occupied": with exactly `classes` occupied bins the thresholds are the first classes - 1 occupied bins;
#               "search": the general search runs there too
#   few_bins    "raise": ValueError with fewer than `classes` occupied bins; "search": the general search runs
RECALLED_MULTIOTSU = {"prob": "float64", "tie": "first", "exact_bins": "occupied", "few_bins": "raise"}
MULTIOTSU_CHOICES = {"prob": ("float64", "float32"), "tie": ("first", "last"), "exact_bins": ("occupied", "search"),
                     "few_bins": ("raise", "search")}
MULTIOTSU_FEW_VALUES = ("The input image has only %d different values. It cannot be thresholded in %d classes.")
# The same for skimage 0.19's watershed(image, markers) at its defaults; the device is built for the defaults.
#   marker_ties  "raster": markers of one value are popped in raster order; "reverse": in reverse raster order.  skimage
#                gives every marker age 0 and leaves equal keys to its binary heap.
#   neighbours   the order in which a popped pixel visits its 4-neighbours.  Under a (value, age) key no label depends on
#                it (every pixel one pop pushes carries one label, and stays together in every queue): recorded because
#                the statement has to choose one.
RECALLED_WATERSHED = {"marker_ties": "raster", "neighbours": "-W,-1,+1,+W"}
WATERSHED_CHOICES = {"marker_ties": ("raster", "reverse"), "neighbours": ("-W,-1,+1,+W", "+W,+1,-1,-W")}


def threshold_multiotsu_from_histogram(counts, edges, classes=3, recalled=None):
    """skimage 0.19's ``threshold_multiotsu(image, classes=3)`` from the ``nbins`` counts and ``nbins + 1`` edges of
    ``np.histogram(image, nbins)``: ``prob = counts / counts.sum()``, zeroth and first moments over the bin index, and
    over all ``i < j`` the pair that maximises ``sum S^2 / P`` over the classes ``[0 .. i]``, ``[i + 1 .. j]``,
    ``[j + 1 .. nbins - 1]`` (a class with ``P = 0`` adds 0); the thresholds are the bin centres ``(e[k] + e[k + 1]) / 2``
    at ``i`` and ``j``.  ``recalled``: overrides of ``RECALLED_MULTIOTSU``.  Only ``classes=3`` is built."""
    if classes != 3:
        raise NotImplementedError("threshold_multiotsu_from_histogram: classes=%r; only 3 classes are implemented" % (classes,))
    rules = dict(RECALLED_MULTIOTSU, **(recalled or {}))
    for name, value in rules.items():
        if value not in MULTIOTSU_CHOICES.get(name, ()):
            raise ValueError("RECALLED_MULTIOTSU: %s=%r is not one of %s" % (name, value, MULTIOTSU_CHOICES.get(name)))
    counts = np.asarray(counts)
    edges = np.asarray(edges, dtype=np.float64)
    if counts.ndim != 1 or counts.size < classes or edges.shape != (counts.size + 1,):
        raise ValueError("counts must be a vector of at least %d bins and edges one longer" % classes)
    if counts.sum() <= 0 or (counts < 0).any():
        raise ValueError("counts must be non-negative with a positive sum")
    nbins = counts.size
    centres = (edges[:-1] + edges[1:]) / 2
    real = np.float32 if rules["prob"] == "float32" else np.float64
    prob = (counts / counts.sum()).astype(real)
    occupied = np.flatnonzero(prob > 0)
    if occupied.size < classes and rules["few_bins"] == "raise":
        raise ValueError(MULTIOTSU_FEW_VALUES % (occupied.size, classes))
    if occupied.size == classes and rules["exact_bins"] == "occupied":
        return centres[occupied[:-1]]
    p = np.cumsum(prob, dtype=real)                                        # P[0 .. k]
    s = np.cumsum(np.arange(nbins, dtype=real) * prob, dtype=real)         # S[0 .. k]

    def term(pc, sc):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(pc > 0, sc * sc / pc, real(0))

    i, j = np.triu_indices(nbins - 1, k=1)                                 # i < j <= nbins - 2, row-major
    criterion = term(p[i], s[i]) + term(p[j] - p[i], s[j] - s[i]) + term(p[-1] - p[j], s[-1] - s[j])
    best = np.flatnonzero(criterion == criterion.max())
    k = best[0] if rules["tie"] == "first" else best[-1]
    return centres[[i[k], j[k]]]


WatershedInputs = namedtuple("WatershedInputs", ["distance_transformed", "thresholds", "markers", "elevation_map"])


def fiber_watershed_inputs(ridges, ridge_cutoff=0.1, sobel_blur=1, out_dir=None, fov=None, debug=False):
    """The middle of ``segment_fibers``: from ``ridges`` (``frangi(...) * 10000``, a ``[H, W]`` plane, taken as float64)
    to what ``watershed`` receives.  Returns the host arrays ``(distance_transformed, thresholds, markers,
    elevation_map)``: ``gaussian_filter(distance_transform_edt(ridges > ridge_cutoff), sigma=1)`` (float64),
    ``threshold_multiotsu`` of it (float64 ``[2]``), the reference's ``threshed`` as int32 (0; 1 below the first
    threshold; 2 above the second) and ``sobel(gaussian_filter(distance_transformed, sobel_blur))`` as int32.
    With ``debug`` and ``out_dir`` (and ``fov``) the reference's two debug files of these stages are written:
    ``_debug/<fov>_thresholded.tiff`` (the markers) and ``_debug/<fov>_ridges_thresholded.tiff`` (the distance map), both
    as float32 -- the reference saves float64 planes, which image_io.write_image does not write; the markers are exact
    in float32, the distance map is rounded once.
    ValueError: a plane in which every pixel exceeds the cutoff (no background: no distance), and a distance map with
    fewer than three occupied histogram bins (a plane without foreground among them); NotImplementedError: a
    ``sobel_blur`` beyond the device blur's radius."""
    from ..som_device.planes import check_blur_sigma
    ridges = np.asarray(ridges)
    if ridges.ndim != 2 or ridges.size == 0:
        raise ValueError("ridges must be a non-empty [H, W] array, got shape %s" % (ridges.shape,))
    check_blur_sigma(sobel_blur)
    _check_debug(out_dir, fov, debug)
    dist, t, markers, elevation = _watershed_inputs_device(ridges.astype(np.float64), float(ridge_cutoff), sobel_blur,
                                                           threshold_multiotsu_from_histogram)
    got = WatershedInputs(np.asarray(dist, dtype=np.float64), np.asarray(t, dtype=np.float64),
                          np.asarray(markers, dtype=np.int32), np.asarray(elevation, dtype=np.int32))
    _write_debug(out_dir, fov, debug, thresholded=got.markers, ridges_thresholded=got.distance_transformed)
    return got


def _check_debug(out_dir, fov, debug):
    """Debug files are written with ``debug`` and an ``out_dir``: that folder must exist and ``fov`` must name them."""
    if debug and out_dir is not None:
        validate_paths(out_dir)
        if fov is None:
            raise ValueError("debug files need fov")


def _write_debug(out_dir, fov, debug, **planes):
    """``_debug/<fov>_<name>.tiff`` per plane, as float32: the reference saves float64 planes, which
    image_io.write_image does not write."""
    if debug and out_dir is not None:
        folder = os.path.join(out_dir, "_debug")
        os.makedirs(folder, exist_ok=True)
        for name, plane in planes.items():
            image_io.write_image(os.path.join(folder, f"{fov}_{name}.tiff"), plane.astype(np.float32))


# ---- the ridge map (K26) ---------------------------------------------------------------------------------------------------
def _contrast_plane(image, what):
    image = np.asarray(image)
    if image.ndim != 2 or image.size == 0:
        raise ValueError("%s must be a non-empty [H, W] array, got shape %s" % (what, image.shape))
    if min(image.shape) < 2:
        from ..som_device.planes import GRADIENT_TOO_SMALL
        raise ValueError(GRADIENT_TOO_SMALL)
    return image.astype(np.float64)


def frangi_ridges(image, fiber_widths=range(1, 10, 2), beta=0.5, gamma=15, scale=10000, out_dir=None, fov=None, debug=False,
                  black_ridges=False):
    """The ``frangi`` stage of ``segment_fibers``: ``frangi(image, sigmas=fiber_widths, black_ridges=False) * scale`` of a
    ``[H, W]`` plane (taken as float64; ``H, W >= 2``) as a float64 host array -- with the defaults the reference's
    ``ridges``.  skimage 0.19's 2-D statement as recalled (``alpha`` only enters the 3-D formula); one
    plane blur and one launch of pxsom_frangi_scale per width.  With ``debug`` and ``out_dir`` (and ``fov``) the
    reference's debug file of this stage is written: ``_debug/<fov>_frangi_filter.tiff``, as float32 -- the reference
    saves a float64 plane, which image_io.write_image does not write; the ridge map is rounded once.
    ValueError: no width, a negative one ("Sigma values less than zero are not valid"), width 0 (skimage returns zeros
    there), ``beta`` or ``gamma`` not finite or <= 0, a plane with a side of 1 (numpy's message); NotImplementedError: a
    width beyond the device blur's radius, ``black_ridges=True``, ``gamma=None`` (skimage >= 0.20's default)."""
    from ..som_device.planes import frangi_arguments
    image = _contrast_plane(image, "image")
    sigmas, _, _ = frangi_arguments(fiber_widths, beta, gamma, black_ridges)
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError("scale must be finite, got %r" % (scale,))
    _check_debug(out_dir, fov, debug)
    ridges = np.asarray(_frangi_device(image, sigmas, float(beta), float(gamma), scale), dtype=np.float64)
    _write_debug(out_dir, fov, debug, frangi_filter=ridges)
    return ridges


def fiber_watershed_inputs_from_contrast(contrast_adjusted, fiber_widths=range(1, 10, 2), ridge_cutoff=0.1, sobel_blur=1,
                                         out_dir=None, fov=None, debug=False):
    """``segment_fibers`` from ``equalize_adapthist``'s result to what ``watershed`` receives, as one chain on the device:
    :func:`frangi_ridges` (the reference's defaults, ``* 10000``) and :func:`fiber_watershed_inputs` without the ridge map
    crossing to the host in between.  Returns ``(inputs, ridges)``: the ``WatershedInputs`` and the float64 ridge plane.
    With ``debug`` and ``out_dir`` (and ``fov``) the three debug files of these stages are written
    (``_debug/<fov>_frangi_filter.tiff``, ``_thresholded.tiff``, ``_ridges_thresholded.tiff``, float32).  Errors: those of
    the two functions."""
    from ..som_device.planes import check_blur_sigma, frangi_arguments
    contrast = _contrast_plane(contrast_adjusted, "contrast_adjusted")
    sigmas, _, _ = frangi_arguments(fiber_widths, 0.5, 15)
    check_blur_sigma(sobel_blur)
    _check_debug(out_dir, fov, debug)
    ridges, dist, t, markers, elevation = _ridge_watershed_inputs_device(contrast, sigmas, float(ridge_cutoff), sobel_blur,
                                                                         threshold_multiotsu_from_histogram)
    got = WatershedInputs(np.asarray(dist, dtype=np.float64), np.asarray(t, dtype=np.float64),
                          np.asarray(markers, dtype=np.int32), np.asarray(elevation, dtype=np.int32))
    ridges = np.asarray(ridges, dtype=np.float64)
    _write_debug(out_dir, fov, debug, frangi_filter=ridges, thresholded=got.markers, ridges_thresholded=got.distance_transformed)
    return got, ridges


# ---- the contrast-adjusted channel (K27) ---------------------------------------------------------------------------------
def _contrast_device(channel: np.ndarray, blur: float, kernel_size: float, clip_limit: float) -> np.ndarray:
    """som_device.contrast_adjust on a host ``[H, W]`` float64 plane: the host array ``equalize_adapthist(b / b.max(),
    kernel_size, clip_limit)`` with ``b = gaussian_filter(channel, blur)``."""
    import torch
    from .. import _capi, som_device
    plane = torch.from_numpy(np.array(channel, dtype=np.float64, order="C")).to(_capi.require_gpu())
    return som_device.contrast_adjust(plane, blur, kernel_size, clip_limit).cpu().numpy()


def _channel_watershed_inputs_device(channel: np.ndarray, blur: float, kernel_size: float, sigmas, ridge_cutoff: float,
                                     sobel_blur: float, thresholds):
    """som_device.channel_watershed_inputs on a host ``[H, W]`` float64 plane, one upload and one chain on the device:
    host arrays ``(contrast, ridges, dist, (t0, t1), markers, elevation)``."""
    import torch
    from .. import _capi, som_device
    plane = torch.from_numpy(np.array(channel, dtype=np.float64, order="C")).to(_capi.require_gpu())
    contrast, ridges, dist, t, markers, elevation = som_device.channel_watershed_inputs(plane, blur, kernel_size, sigmas,
                                                                                        ridge_cutoff, sobel_blur, thresholds)
    return contrast.cpu().numpy(), ridges.cpu().numpy(), dist.cpu().numpy(), t, markers.cpu().numpy(), elevation.cpu().numpy()


CLAHE_CLIP_LIMIT = 0.01                                       # equalize_adapthist's default, which the reference keeps


def _channel_arguments(image, blur, contrast_scaling_divisor):
    """The checked front arguments, without a device: ``(channel float64, blur, kernel_size)`` with ``kernel_size =
    image.shape[0] / contrast_scaling_divisor``, as the reference computes it from ``fov_len``."""
    from ..som_device.planes import check_blur_sigma, clahe_arguments
    image = np.asarray(image)
    if image.ndim != 2 or image.size == 0:
        raise ValueError("image must be a non-empty [H, W] array, got shape %s" % (image.shape,))
    divisor = float(contrast_scaling_divisor)
    if not (np.isfinite(divisor) and divisor > 0):
        raise ValueError("contrast_scaling_divisor must be finite and > 0, got %r" % (contrast_scaling_divisor,))
    blur = float(blur)
    if not (np.isfinite(blur) and blur >= 0):
        raise ValueError("blur must be finite and >= 0, got %r" % (blur,))
    check_blur_sigma(blur)
    kernel_size = image.shape[0] / divisor
    clahe_arguments(image.shape, kernel_size, CLAHE_CLIP_LIMIT)
    channel = image.astype(np.float64)
    if not np.isfinite(channel).all():
        raise ValueError("image must be finite: the reference's division by the maximum gives NaNs otherwise")
    if not channel.max() > 0:
        raise ValueError("image must hold a positive pixel: the reference divides the blurred image by its maximum")
    return channel, blur, kernel_size


def contrast_adjusted_channel(image, blur=2, contrast_scaling_divisor=128, out_dir=None, fov=None, debug=False):
    """The front of ``segment_fibers``: ``equalize_adapthist(b / np.max(b), kernel_size=image.shape[0] /
    contrast_scaling_divisor)`` with ``b = gaussian_filter(image, sigma=blur)`` of a ``[H, W]`` plane (taken as float64;
    ``H, W >= 2``) as a float64 host array in [0, 1] -- the reference's ``contrast_adjusted``.  skimage 0.19's statement as
    recalled (parity with skimage itself is unpinned); the plane blur, pxsom_plane_minmax,
    pxsom_plane_divide, pxsom_clahe_quantize and pxsom_clahe_equalize on the device.  With ``debug`` and ``out_dir`` (and
    ``fov``) the reference's debug file of this stage is written: ``_debug/<fov>_contrast_adjusted.tiff``, as float32 --
    the reference saves a float64 plane, which image_io.write_image does not write; the plane is rounded once.
    ValueError: a kernel size below 1 (the reference divides by zero there), a divisor that is not finite and positive,
    a ``blur`` that is not finite or negative, an image with a pixel that is not finite or without a positive pixel, a
    blurred image whose maximum is not positive; NotImplementedError: a kernel size beyond the shorter side, a ``blur`` beyond the
    device blur's radius."""
    channel, blur, kernel_size = _channel_arguments(image, blur, contrast_scaling_divisor)
    _check_debug(out_dir, fov, debug)
    contrast = np.asarray(_contrast_device(channel, blur, kernel_size, CLAHE_CLIP_LIMIT), dtype=np.float64)
    _write_debug(out_dir, fov, debug, contrast_adjusted=contrast)
    return contrast


def fiber_watershed_inputs_from_channel(image, blur=2, contrast_scaling_divisor=128, fiber_widths=range(1, 10, 2),
                                        ridge_cutoff=0.1, sobel_blur=1, out_dir=None, fov=None, debug=False):
    """``segment_fibers`` from the raw channel to what ``watershed`` receives, as one chain on the device:
    :func:`contrast_adjusted_channel`, :func:`frangi_ridges` (the reference's defaults, ``* 10000``) and
    :func:`fiber_watershed_inputs` without a plane crossing to the host in between.  Returns ``(inputs, ridges,
    contrast_adjusted)``: the ``WatershedInputs`` and two float64 planes.  With ``debug`` and ``out_dir`` (and ``fov``)
    the four debug files of these stages are written (``_debug/<fov>_contrast_adjusted.tiff``, ``_frangi_filter.tiff``,
    ``_thresholded.tiff``, ``_ridges_thresholded.tiff``, float32).  Errors: those of the three functions."""
    from ..som_device.planes import check_blur_sigma, frangi_arguments
    channel, blur, kernel_size = _channel_arguments(image, blur, contrast_scaling_divisor)
    sigmas, _, _ = frangi_arguments(fiber_widths, 0.5, 15)
    check_blur_sigma(sobel_blur)
    _check_debug(out_dir, fov, debug)
    contrast, ridges, dist, t, markers, elevation = _channel_watershed_inputs_device(
        channel, blur, kernel_size, sigmas, float(ridge_cutoff), sobel_blur, threshold_multiotsu_from_histogram)
    got = WatershedInputs(np.asarray(dist, dtype=np.float64), np.asarray(t, dtype=np.float64),
                          np.asarray(markers, dtype=np.int32), np.asarray(elevation, dtype=np.int32))
    contrast, ridges = np.asarray(contrast, dtype=np.float64), np.asarray(ridges, dtype=np.float64)
    _write_debug(out_dir, fov, debug, contrast_adjusted=contrast, frangi_filter=ridges, thresholded=got.markers,
                 ridges_thresholded=got.distance_transformed)
    return got, ridges, contrast


# ---- the object table -------------------------------------------------------------------------------------------------
def _object_columns(object_properties):
    names = []
    for p in object_properties:
        if p not in BUILT_OBJECT_PROPS:
            raise NotImplementedError("object_properties: %r is not implemented; the built properties are %s"
                                      % (p, ", ".join(BUILT_OBJECT_PROPS)))
        names += ["centroid-0", "centroid-1"] if p == "centroid" else [p]
    return names


def fiber_object_props(labels, fov, object_properties=FIBER_OBJECT_PROPS):
    """The ``regionprops_table`` step of ``segment_fibers``: one row per non-zero label of a ``[H, W]`` label plane,
    labels ascending -- ``fov`` first, then the properties in list order with ``centroid`` as ``centroid-0``,
    ``centroid-1``.  An object is every pixel of one label, of any size.  An all-background plane gives an empty frame
    with these columns; a property outside the built ones raises NotImplementedError."""
    names = _object_columns(object_properties)
    raw = _region_raw_device(_as_label_plane(labels, "labels"))
    raw.setdefault("hull", np.zeros((np.asarray(raw["keys"]).size, 4), dtype=np.int64))   # no convex columns here
    with np.errstate(divide="ignore", invalid="ignore"):
        cols = rpe.morphology(raw, orientation=True)
    cols["label"] = np.asarray(raw["keys"], dtype=np.int64)
    table = pd.DataFrame({name: cols[name] for name in names}, columns=names)
    table.insert(0, FOV_ID, fov)
    return table


def fiber_objects(mask, fov, out_dir=None, min_fiber_size=15, object_properties=FIBER_OBJECT_PROPS, save_csv=False):
    """The tail of ``segment_fibers`` from its binary ``segmentation`` on: ``ndi.label`` (4-connected), the components
    under ``min_fiber_size`` pixels removed (``remove_small_objects``; labels are not renumbered, so gaps stay, as in
    the reference), then :func:`fiber_object_props`.  With ``out_dir`` the labels are saved as
    ``<fov>_fiber_labels.tiff`` (int32) and, with ``save_csv``, the table as ``fiber_object_table.csv`` as the
    reference writes it.  Returns ``(table, labels)``."""
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.size == 0:
        raise ValueError("mask must be a non-empty [H, W] array, got shape %s" % (mask.shape,))
    _object_columns(object_properties)      # refuse an unbuilt property before any work
    if out_dir is not None:
        validate_paths(out_dir)
    labels = _label_and_filter_device(mask, int(min_fiber_size))
    if out_dir is not None:
        image_io.write_image(os.path.join(out_dir, f"{fov}{_LABELS_SUFFIX}"), labels)
    table = fiber_object_props(labels, fov, object_properties)
    if save_csv:
        if out_dir is None:
            raise ValueError("save_csv needs out_dir")
        table.to_csv(os.path.join(out_dir, "fiber_object_table.csv"))
    return table, labels


def fiber_object_table_from_labels(fibseg_dir, fovs=None, csv_compression: Optional[Dict[str, str]] = None):
    """The fibre object table of a cohort from the ``<fov>_fiber_labels.tiff`` files of ``fibseg_dir`` (every such file
    in natural order, or those of ``fovs``): one :func:`fiber_object_props` per FOV, stacked, with the alignment score
    of :func:`calculate_fiber_alignment` (default k and threshold) as the last column, returned and written to
    ``fiber_object_table.csv`` without the index -- the table ``run_fiber_segmentation`` leaves behind.  A cohort
    without a single fibre gives the empty table with the same columns."""
    validate_paths(fibseg_dir)
    if fovs is None:
        fovs = natsorted(f[:-len(_LABELS_SUFFIX)] for f in list_files(fibseg_dir, substrs=_LABELS_SUFFIX)
                         if f.endswith(_LABELS_SUFFIX))
    else:
        fovs = [fovs] if isinstance(fovs, str) else list(fovs)
        validate_paths([os.path.join(fibseg_dir, fov + _LABELS_SUFFIX) for fov in fovs])
    if len(fovs) == 0:
        raise ValueError("no %s files in %s" % ("<fov>" + _LABELS_SUFFIX, fibseg_dir))
    per_fov = (fiber_object_props(image_io.read_image(os.path.join(fibseg_dir, fov + _LABELS_SUFFIX)), fov) for fov in fovs)
    scored = calculate_fiber_alignment(pd.concat(list(per_fov)))
    scored.to_csv(os.path.join(fibseg_dir, "fiber_object_table.csv"), index=False, compression=csv_compression)
    return scored


# ---- alignment ------------------------------------------------------------------------------------------------------
def _rank_order_sums(terms: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """Per row of ``terms`` [m, k], the sum of its first ``counts[i]`` entries in the order numpy sums a contiguous
    float64 vector of that many elements (a fold below 8, its pairwise rule from 8 on): rows are grouped by count and
    every group is reduced along its contiguous last axis."""
    out = np.zeros(terms.shape[0], dtype=np.float64)
    for c in np.unique(counts):
        if c > 0:
            rows = counts == c
            out[rows] = np.add.reduce(np.ascontiguousarray(terms[rows, :c]), axis=1)
    return out


def calculate_fiber_alignment(fiber_object_table, k=4, axis_thresh=2):
    """The reference's alignment score, appended as ``alignment_score`` by a left merge on the shared columns: for every
    fibre with ``major_axis_length / minor_axis_length >= axis_thresh`` (numpy's division: x / 0 = inf is kept, 0 / 0
    is not), ``sqrt(sum (theta_j - theta_i)^2) / k`` over its k nearest such fibres j of the same FOV by centroid
    distance.  The neighbours of the whole table come from one pxsom_nearest_indices launch; the sum runs in rank order
    as numpy sums the reference's vector, so the scores are the reference's bits.  A fibre with m < k neighbours sums m
    terms and still divides by k (a FOV's only fibre scores 0.0); the other fibres get NaN.

    Where distances tie inside the first k + 1 ranks of a row the reference's ``argsort()[1 : 1 + k]`` is an unstable
    sort's choice, and with a fibre on the same centroid it may keep the fibre itself in place of the other: that is
    not reproducible.  Here ties go to the earlier row of the table and a fibre is never its own neighbour.  ``k`` is
    limited to 1 .. 32 (the device route); a table without rows comes back with an empty ``alignment_score`` column,
    where the reference's ``pd.concat`` raises."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1, got %d" % k)
    if k > NEAREST_MAX_K:
        raise NotImplementedError("k=%d: the device route keeps the k nearest fibres in registers, k <= %d"
                                  % (k, NEAREST_MAX_K))
    table = fiber_object_table
    fov_values = np.asarray(table[FOV_ID])
    fovs, codes = np.unique(fov_values, return_inverse=True) if len(table) else (np.array([]), np.zeros(0, np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = (table["major_axis_length"].values / table["minor_axis_length"].values) >= axis_thresh
    rows = np.flatnonzero(keep)
    rows = rows[np.argsort(codes[rows], kind="stable")]                 # FOV by FOV in np.unique's order, table order inside
    seg = np.concatenate([[0], np.cumsum(np.bincount(codes[rows], minlength=len(fovs)))]).astype(np.int64)
    xy = np.stack([table["centroid-0"].values[rows], table["centroid-1"].values[rows]], axis=1).astype(np.float64)
    theta = np.asarray(table["orientation"].values[rows], dtype=np.float64)
    if len(rows):
        idx = np.asarray(_nearest_indices_device(xy, seg, k)).reshape(len(rows), k)
        found = idx >= 0
        diff = np.where(found, theta[np.where(found, idx, 0)] - theta[:, None], 0.0)
        scores = np.sqrt(_rank_order_sums(np.square(diff), found.sum(axis=1))) / k
    else:
        scores = np.zeros(0, dtype=np.float64)
    alignment_data = pd.DataFrame({FOV_ID: fov_values[rows], "label": table["label"].values[rows],
                                   "alignment_score": scores})
    if len(table) == 0:
        alignment_data = alignment_data.astype({FOV_ID: table[FOV_ID].dtype, "label": table["label"].dtype})
    return table.merge(alignment_data, "left")


# ---- densities and summaries (host) ---------------------------------------------------------------------------------
# Written against the contract of the reference's functions -- their arguments, columns, file names, NaN rules and error
# text -- and the g26 fixture: fibres are binned into tiles once and every statistic is a grouped reduction over the bins.
_STAT_COLUMNS = ["pixel_density", "fiber_density"]


def _percent_of(count, total_pixels):
    """``count / total_pixels`` as a percentage, the quotient first (the rounding order the fixture records)."""
    return count / total_pixels * 100


def calculate_density(fov_fiber_table, total_pixels):
    """``(pixel_density, fiber_density)`` of a table of fibres over an area of ``total_pixels``, in percent: the fibres'
    summed ``area`` per pixel, and the number of distinct ``label`` values per pixel."""
    covered = fov_fiber_table["area"].to_numpy().sum()
    distinct = fov_fiber_table["label"].nunique()
    return _percent_of(covered, total_pixels), _percent_of(distinct, total_pixels)


def _tile_bins(centroids, tiles_per_side, tile_length):
    """The tile index along one axis of every centroid, -1 outside ``[0, tiles_per_side * tile_length)`` (NaN too):
    ``edge[i] <= c < edge[i + 1]`` decided by comparison with the integer edges, never by a division of the centroid."""
    edges = np.arange(tiles_per_side + 1) * tile_length
    bins = np.searchsorted(edges, np.asarray(centroids, dtype=np.float64), side="right") - 1
    return np.where((bins >= 0) & (bins < tiles_per_side), bins, -1)


def generate_tile_stats(fov_table, fov_fiber_img, fov_length, tile_length, min_fiber_num, save_dir, save_tiles):
    """Tile statistics of one FOV: one row per ``tile_length`` square of an image of side ``fov_length``, row by row of
    tiles (``fov``, ``tile_y``, ``tile_x``), over the fibres whose centroid lies in the square: ``pixel_density`` and
    ``fiber_density`` (:func:`calculate_density` over the tile's area), ``avg_alignment_score`` (the mean of the scores
    that are not NaN) and ``avg_<property>`` for the six object properties.  A tile with fewer than ``min_fiber_num``
    fibres is NaN throughout, and its alignment mean also when fewer than that many of its fibres are scored.
    ``save_tiles`` writes every tile of ``fov_fiber_img``, binarised, to ``<save_dir>/<fov>/tile_<y>,<x>.tiff``; the
    caller's image is left as it is (the reference binarises it in place, through the view it crops)."""
    if len(fov_table) == 0:
        raise ValueError("generate_tile_stats needs at least one fibre to name the FOV")
    fov = fov_table[FOV_ID].iloc[0]
    per_side = int(fov_length // tile_length)
    n_tiles = per_side * per_side
    by, bx = (_tile_bins(fov_table[c].to_numpy(), per_side, tile_length) for c in ("centroid-0", "centroid-1"))
    inside = (by >= 0) & (bx >= 0)
    fibres = fov_table[inside].assign(_tile=(by * per_side + bx)[inside])
    tiles = fibres.groupby("_tile")
    every = pd.RangeIndex(n_tiles)

    members = tiles.size().reindex(every, fill_value=0)
    scored = tiles["alignment_score"].count().reindex(every, fill_value=0)          # NaN is not counted
    enough = (members >= min_fiber_num).to_numpy()
    area = tiles["area"].sum().reindex(every, fill_value=0).to_numpy()
    distinct = tiles["label"].nunique().reindex(every, fill_value=0).to_numpy()
    out = pd.DataFrame({FOV_ID: [fov] * n_tiles,
                        "tile_y": np.repeat(np.arange(per_side), per_side) * tile_length,
                        "tile_x": np.tile(np.arange(per_side), per_side) * tile_length})
    out["pixel_density"] = np.where(enough, _percent_of(area, tile_length ** 2), np.nan)
    out["fiber_density"] = np.where(enough, _percent_of(distinct, tile_length ** 2), np.nan)
    score_mean = tiles["alignment_score"].mean().reindex(every).to_numpy(dtype=np.float64)
    out["avg_alignment_score"] = np.where(enough & (scored >= min_fiber_num).to_numpy(), score_mean, np.nan)
    means = tiles[_TILE_PROPERTIES].mean().reindex(every)
    for name in _TILE_PROPERTIES:
        out["avg_" + name] = np.where(enough, means[name].to_numpy(dtype=np.float64), np.nan)

    if save_tiles:
        folder = os.path.join(save_dir, fov)
        os.makedirs(folder, exist_ok=True)
        plane = np.asarray(fov_fiber_img)
        for y, x in zip(out["tile_y"], out["tile_x"]):
            binary = (plane[y:y + tile_length, x:x + tile_length] > 0).astype(plane.dtype)
            image_io.write_image(os.path.join(folder, "tile_%d,%d.tiff" % (y, x)), binary)
    return out


def generate_summary_stats(fiber_object_table, fibseg_dir, tile_length=512, min_fiber_num=5, save_tiles=False):
    """FOV and tile summaries of a fibre object table.  ``fov_stats``: per FOV (sorted) the two densities over the whole
    image -- its side read from ``<fov>_fiber_labels.tiff`` in ``fibseg_dir`` -- and ``avg_<column>`` for the six object
    properties and ``alignment_score`` (NaN skipped), written to ``fiber_stats_table.csv``.  ``tile_stats``:
    :func:`generate_tile_stats` of every FOV, stacked, written to
    ``tile_stats_<tile_length>/fiber_stats_table-tile_<tile_length>.csv``.  ``tile_length`` must divide 1024."""
    validate_paths(fibseg_dir)
    if 1024 % tile_length != 0:
        raise ValueError("Tile length must be a factor of the minimum image size.")
    tile_dir = os.path.join(fibseg_dir, "tile_stats_%s" % tile_length)
    columns = _TILE_PROPERTIES + ["alignment_score"]
    fov_rows, tile_frames = [], []
    for fov, fibres in fiber_object_table.groupby(FOV_ID, sort=True):
        plane = _as_label_plane(image_io.read_image(os.path.join(fibseg_dir, fov + _LABELS_SUFFIX)), fov)
        side = plane.shape[0]
        row = dict(zip([FOV_ID] + _STAT_COLUMNS, (fov,) + calculate_density(fibres, side ** 2)))
        row.update(("avg_" + name, value) for name, value in fibres[columns].mean().items())
        fov_rows.append(row)
        tile_frames.append(generate_tile_stats(fibres, plane, side, tile_length, min_fiber_num, tile_dir, save_tiles))
    fov_stats = pd.DataFrame(fov_rows, columns=[FOV_ID] + _STAT_COLUMNS + ["avg_" + name for name in columns])
    tile_stats = pd.concat(tile_frames)
    os.makedirs(tile_dir, exist_ok=True)
    fov_stats.to_csv(os.path.join(fibseg_dir, "fiber_stats_table.csv"), index=False)
    tile_stats.to_csv(os.path.join(tile_dir, "fiber_stats_table-tile_%s.csv" % tile_length), index=False)
    return fov_stats, tile_stats


# ---- the watershed, and segment_fibers end to end on one channel plane (K28) ---------------------------------------------
def _watershed_device(elevation: np.ndarray, markers: np.ndarray) -> np.ndarray:
    """som_device.watershed on two host ``[H, W]`` int32 planes: the int32 labels on the host."""
    import torch
    from .. import _capi, som_device
    gpu = _capi.require_gpu()
    planes = [torch.from_numpy(np.array(a, dtype=np.int32, order="C")).to(gpu) for a in (elevation, markers)]
    return som_device.watershed(planes[0], planes[1]).cpu().numpy()


def _channel_fiber_labels_device(channel: np.ndarray, blur: float, kernel_size: float, sigmas, ridge_cutoff: float,
                                 sobel_blur: float, thresholds, min_fiber_size: int, planes: bool):
    """som_device.channel_fiber_labels on a host ``[H, W]`` float64 plane, one upload and one chain on the device: the host
    arrays ``(labels, contrast, ridges, dist, (t0, t1), markers, elevation)``.  Only the int32 labels and the two
    thresholds come down unless ``planes`` (the debug files) asks for the rest, which is None otherwise."""
    import torch
    from .. import _capi, som_device
    plane = torch.from_numpy(np.array(channel, dtype=np.float64, order="C")).to(_capi.require_gpu())
    labels, contrast, ridges, dist, t, markers, elevation = som_device.channel_fiber_labels(
        plane, blur, kernel_size, sigmas, ridge_cutoff, sobel_blur, thresholds, min_fiber_size)
    rest = [p.cpu().numpy() if planes else None for p in (contrast, ridges, dist, markers, elevation)]
    return labels.cpu().numpy(), rest[0], rest[1], rest[2], t, rest[3], rest[4]


def watershed_labels(elevation, markers):
    """``skimage.segmentation.watershed(elevation, markers)`` at its defaults (connectivity 1, no mask, no compactness, no
    watershed line) of two ``[H, W]`` arrays, each taken ``.astype(np.int32)`` as the reference passes them: the int32
    labels on the host.  skimage 0.19's statement as recalled (``RECALLED_WATERSHED``; parity with skimage
    itself is unpinned): a priority flood keyed (value, age), markers of one value in raster order; any non-zero marker is
    a label, and a plane without one comes back all zeros.  ValueError: planes that are not 2-D, empty, or of two shapes,
    and values that an int32 does not hold (NaN among them)."""
    planes = []
    for name, a in (("elevation", elevation), ("markers", markers)):
        a = np.asarray(a)
        if a.ndim != 2 or a.size == 0:
            raise ValueError("%s must be a non-empty [H, W] array, got shape %s" % (name, a.shape))
        if a.dtype.kind not in "biuf":
            raise ValueError("%s must be numeric, got %s" % (name, a.dtype))
        if a.dtype.kind == "f" and not np.isfinite(a).all():
            raise ValueError("%s must be finite" % name)
        if a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1:
            raise ValueError("%s holds values beyond int32" % name)
        planes.append(a.astype(np.int32))
    if planes[0].shape != planes[1].shape:
        raise ValueError("elevation and markers must have one shape, got %s and %s" % (planes[0].shape, planes[1].shape))
    return np.asarray(_watershed_device(planes[0], planes[1]), dtype=np.int32)


def segment_fiber_channel(image, fov, out_dir, blur=2, contrast_scaling_divisor=128, fiber_widths=range(1, 10, 2),
                          ridge_cutoff=0.1, sobel_blur=1, min_fiber_size=15, object_properties=FIBER_OBJECT_PROPS,
                          save_csv=True, debug=False):
    """The reference's ``segment_fibers`` from its ``fiber_channel_data`` line to its return, on the channel plane itself:
    ``image`` is the ``[H, W]`` fibre channel of ``fov`` (taken as float64), where the reference takes an xarray and a
    channel name.  One chain on the device -- the front (K27), frangi (K26), the middle (K25), the watershed (K28), the
    pixels of marker class 2, ``ndi.label`` and the ``min_fiber_size`` filter (K23) -- then ``<fov>_fiber_labels.tiff``
    (int32) in ``out_dir``, with ``debug`` the four files of ``_debug/`` (float32, as :func:`fiber_watershed_inputs`
    explains), :func:`fiber_object_props` and, with ``save_csv``, ``fiber_object_table.csv`` written with its index, as the
    reference writes it.  Returns the table.  Errors: a missing ``out_dir`` (FileNotFoundError), an unbuilt property
    (NotImplementedError) and those of :func:`fiber_watershed_inputs_from_channel`, all before any device work."""
    from ..som_device.planes import check_blur_sigma, frangi_arguments
    _object_columns(object_properties)
    validate_paths(out_dir)
    channel, blur, kernel_size = _channel_arguments(image, blur, contrast_scaling_divisor)
    sigmas, _, _ = frangi_arguments(fiber_widths, 0.5, 15)
    check_blur_sigma(sobel_blur)
    labels, contrast, ridges, dist, _, markers, _ = _channel_fiber_labels_device(
        channel, blur, kernel_size, sigmas, float(ridge_cutoff), sobel_blur, threshold_multiotsu_from_histogram,
        int(min_fiber_size), bool(debug))
    labels = np.asarray(labels, dtype=np.int32)
    if debug:
        _write_debug(out_dir, fov, True, thresholded=np.asarray(markers), ridges_thresholded=np.asarray(dist),
                     frangi_filter=np.asarray(ridges), contrast_adjusted=np.asarray(contrast))
    image_io.write_image(os.path.join(out_dir, f"{fov}{_LABELS_SUFFIX}"), labels)
    table = fiber_object_props(labels, fov, object_properties)
    if save_csv:
        table.to_csv(os.path.join(out_dir, "fiber_object_table.csv"))
    return table


def run_fiber_channel_segmentation(data_dir, fiber_channel, out_dir, img_sub_folder=None,
                                   csv_compression: Optional[Dict[str, str]] = None, **kwargs):
    """The reference's ``run_fiber_segmentation``: both folders must exist and the first FOV folder of ``data_dir`` (natural
    order) must hold ``fiber_channel`` (FileNotFoundError, ValueError); then per FOV folder, in natural order, the channel's
    image file is read (``<data_dir>/<fov>/<img_sub_folder>/<fiber_channel>.<ext>``) and :func:`segment_fiber_channel`
    runs on it with ``save_csv=False`` and ``kwargs``.  The tables are stacked, scored by
    :func:`calculate_fiber_alignment` when there is a row, written to ``fiber_object_table.csv`` without the index and
    returned.  A cohort without a fibre gives the empty table with the object columns."""
    sub = img_sub_folder or ""
    validate_paths([data_dir, out_dir])
    fovs = natsorted(list_folders(data_dir))
    if len(fovs) == 0:
        raise ValueError("no FOV folder in %s" % (data_dir,))
    verify_in_list(fiber_channel=[fiber_channel],
                   all_channels=remove_file_extensions(list_files(os.path.join(data_dir, fovs[0], sub))))
    for name in ("save_csv", "fov", "out_dir", "image"):
        if name in kwargs:
            raise TypeError("run_fiber_channel_segmentation sets %s itself" % name)
    tables = []
    for fov in fovs:
        files = list_files(os.path.join(data_dir, fov, sub), substrs=fiber_channel, exact_match=True)
        if len(files) == 0:
            raise ValueError("FOV %s holds no image of channel %s" % (fov, fiber_channel))
        image = image_io.read_image(os.path.join(data_dir, fov, sub, files[0]))
        tables.append(segment_fiber_channel(image, fov, out_dir, save_csv=False, **kwargs))
    table = pd.concat(tables)
    if len(table) > 0:
        table = calculate_fiber_alignment(table)
    table.to_csv(os.path.join(out_dir, "fiber_object_table.csv"), index=False, compression=csv_compression)
    return table


# ---- the entries whose front half is not built --------------------------------------------------------------------------
def _refuse(entry, folders, channel_folder, fiber_channel):
    """What the three entries below share: every folder must exist, ``fiber_channel`` must name an image file of
    ``channel_folder()`` (None: nothing to look up), and then the entry is refused."""
    validate_paths(list(folders))
    if channel_folder is not None:
        channels = remove_file_extensions(list_files(channel_folder()))
        verify_in_list(fiber_channel=[fiber_channel], all_channels=channels)
    raise NotImplementedError(entry + ": " + _UNBUILT)


def plot_fiber_segmentation_steps(data_dir, fov_name, fiber_channel, img_sub_folder=None, blur=2,
                                  contrast_scaling_divisor=128, fiber_widths=range(1, 10, 2), ridge_cutoff=0.1,
                                  sobel_blur=1, min_fiber_size=15, img_cmap="bone", labels_cmap="cool"):
    """The reference's signature.  ``data_dir`` must exist and hold ``fiber_channel`` for ``fov_name``
    (FileNotFoundError, ValueError); then NotImplementedError: the steps it would plot are not built."""
    _refuse("plot_fiber_segmentation_steps", [data_dir],
            lambda: os.path.join(data_dir, fov_name, img_sub_folder or ""), fiber_channel)


def run_fiber_segmentation(data_dir, fiber_channel, out_dir, img_sub_folder=None,
                           csv_compression: Optional[Dict[str, str]] = None, **kwargs):
    """The reference's signature.  Both folders must exist and the first FOV of ``data_dir`` (natural order) must hold
    ``fiber_channel`` (FileNotFoundError, ValueError); then NotImplementedError naming the stages that are not built."""
    _refuse("run_fiber_segmentation", [data_dir, out_dir],
            lambda: os.path.join(data_dir, natsorted(list_folders(data_dir))[0], img_sub_folder or ""), fiber_channel)


def segment_fibers(data_xr, fiber_channel, out_dir, fov, blur=2, contrast_scaling_divisor=128,
                   fiber_widths=range(1, 10, 2), ridge_cutoff=0.1, sobel_blur=1, min_fiber_size=15,
                   object_properties=FIBER_OBJECT_PROPS, save_csv=True, debug=False):
    """The reference's signature; ``out_dir`` must exist and the properties must be built ones; then
    NotImplementedError naming the stages that are not built."""
    _object_columns(object_properties)
    _refuse("segment_fibers", [out_dir], None, fiber_channel)
