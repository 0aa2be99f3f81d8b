"""Image planes and masks: cluster and segmentation masks, the plane blurs, object masks (K16, K22), mask merging (K18),
the distance map, histogram, markers and elevation of fibre segmentation (K25), its Frangi ridge filter (K26), its
adaptive histogram equalisation (K27) and its marker watershed (K28)."""
import operator
from typing import Optional

import numpy as np
import torch

from .. import _capi
from ._args import (PAIR_CAPACITY_MAX, PLANE_DTYPES, PLANE_MODE_DTYPES, SEG_DTYPES, SEG_F64, _binary_plane, _check_apart,
                    _f64_plane, _label_image, _label_pair, _label_plane, _ld, _like_plane, _rows_plane)
from .pixels import gaussian_kernel1d, quantile_f32, quantile_nonzero


MASK_BAD_LABEL, MASK_BAD_PIXEL = 1, 2   # include/pxsom.h PXSOM_MASK_*
LUT_UNMAPPED = -2 ** 31                 # PXSOM_LUT_UNMAPPED


def cluster_mask(row_index: torch.Tensor, column_index: torch.Tensor, labels: torch.Tensor, lut: torch.Tensor,
                 h: int, w: int):
    """``mask.ravel()[row_index * w + column_index] = lut[labels]`` on an int16 ``[h, w]`` image of zeros
    (last row wins for a pixel listed twice).  int64 HBM vectors, int32 LUT.  Returns ``(mask, status)``:
    status 0, or MASK_BAD_LABEL / MASK_BAD_PIXEL bits (synchronises to read it)."""
    for name, t in (("row_index", row_index), ("column_index", column_index), ("labels", labels)):
        if t.dtype != torch.int64 or not t.is_cuda or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 HBM vector")
    if not (row_index.numel() == column_index.numel() == labels.numel()):
        raise ValueError("row_index, column_index and labels must have one entry per table row")
    if lut.dtype != torch.int32 or not lut.is_cuda or not lut.is_contiguous():
        raise ValueError("lut must be a contiguous int32 HBM vector")
    dev = labels.device
    mask = torch.empty((int(h), int(w)), dtype=torch.int16, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = _capi.lib().pxsom_cluster_mask_workspace_bytes(int(h), int(w))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    _capi.call("pxsom_cluster_mask", row_index.data_ptr(), column_index.data_ptr(), labels.data_ptr(),
               labels.numel(), lut.data_ptr(), lut.numel(), int(h), int(w),
               mask.data_ptr(), status.data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr())
    return mask, int(status.item())


SEG_ERODE = {None: 0, "thick": 1, "inner": 2}
SEGMASK_FORCE_SEARCH = 1


def segmask_table(keys, values, device, float_values: bool = False):
    """Host (key -> value) arrays as the device table of :func:`segmentation_mask`: ``keys`` int32, sorted ascending and
    unique (checked here: the library relies on it), ``values`` int32, or float64 with ``float_values``."""
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float64 if float_values else np.int32)
    if keys.ndim != 1 or values.shape != keys.shape:
        raise ValueError("keys and values must be vectors of one length")
    if keys.size > 1 and not np.all(keys[1:] > keys[:-1]):
        raise ValueError("keys must be sorted ascending without duplicates")
    return (torch.from_numpy(keys).to(device), torch.from_numpy(values).to(device),
            int(keys[0]) if keys.size else 0, int(keys[-1]) if keys.size else 0)


def segmentation_mask(seg: torch.Tensor, erode: Optional[str] = None, connectivity: int = 1, background: int = 0,
                      table=None, unassigned=0, out_dtype: Optional[torch.dtype] = None, force_search: bool = False,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One pass of pxsom_segmask over a ``[H, W]`` label image in HBM (rows contiguous, any row stride): optional border
    erosion (``erode`` "thick" / "inner": skimage's find_boundaries with ``connectivity`` and ``background``; boundary
    pixels become 0), then the optional lookup ``table`` of :func:`segmask_table` (label cast to int32, ``unassigned``
    where the table has no entry), stored as ``out_dtype`` (int16, int32, float64 or the image's dtype; default: the
    image's).  ``force_search`` takes the binary-search route even where a dense LUT would fit."""
    h, w, ld = _label_image(seg, "seg")
    if erode not in SEG_ERODE:
        raise NotImplementedError(f"erosion mode {erode!r}: only 'thick' and 'inner' are implemented")
    connectivity = max(int(connectivity), 1)        # scipy's generate_binary_structure treats < 1 as 1
    if out_dtype is None:
        out_dtype = seg.dtype
    if out_dtype != seg.dtype and out_dtype not in (torch.int16, torch.int32, torch.float64):
        raise ValueError("out_dtype must be int16, int32, float64 or the image's dtype")
    code_out = SEG_F64 if out_dtype == torch.float64 else SEG_DTYPES[out_dtype]
    out = _rows_plane(out, h, w, out_dtype, seg.device, "out")
    ldo = _ld(out)
    lib = _capi.lib()
    if table is None:
        keys = values = None
        n_keys, kmin, kmax = -1, 0, 0
    else:
        keys, values, kmin, kmax = table
        n_keys = keys.numel()
        if values.dtype != (torch.float64 if out_dtype == torch.float64 else torch.int32):
            raise ValueError("table values must be float64 for a float64 output, int32 otherwise")
    wsb = 0 if force_search or n_keys <= 0 else lib.pxsom_segmask_workspace_bytes(n_keys, kmin, kmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device=seg.device) if wsb else None
    _capi.call("pxsom_segmask", seg.data_ptr(), SEG_DTYPES[seg.dtype], h, w, ld, SEG_ERODE[erode], connectivity, int(background),
               keys.data_ptr() if keys is not None else None, values.data_ptr() if values is not None else None,
               n_keys, kmin, kmax, float(unassigned), out.data_ptr(), code_out, ldo,
               ws.data_ptr() if ws is not None else None, wsb,
               SEGMASK_FORCE_SEARCH if force_search else 0, _capi.stream_ptr())
    return out


BLUR_MAX_RADIUS = 64                     # kMaxRadius of csrc/pxsom_pre.hip
BLUR_SIGMA_LIMIT = 16.125                # int(4 sigma + 0.5) <= 64  <=>  sigma < 16.125


def check_blur_sigma(sigma: float) -> None:
    """NotImplementedError for a sigma whose radius the device blur does not take (sigma >= 16.125)."""
    if float(sigma) > 1e-15 and int(4.0 * float(sigma) + 0.5) > BLUR_MAX_RADIUS:
        raise NotImplementedError("gaussian blur on the device: sigma %r is beyond the radius limit "
                                  "(sigma < %g, radius <= %d)" % (sigma, BLUR_SIGMA_LIMIT, BLUR_MAX_RADIUS))


BLUR_MODES = {"reflect": 0, "nearest": 1}          # include/pxsom.h PXSOM_BLUR_REFLECT / PXSOM_BLUR_NEAREST


def _blur_plane(plane: torch.Tensor, sigma: float, mode: str, out, tmp, mode_entry: bool) -> torch.Tensor:
    """The body of both plane blurs; ``mode_entry``: through pxsom_gaussian_blur_plane_mode."""
    if mode not in BLUR_MODES:
        raise ValueError("mode must be 'reflect' or 'nearest', got %r" % (mode,))
    if plane.dim() != 2 or not plane.is_cuda or not plane.is_contiguous() or plane.dtype not in PLANE_MODE_DTYPES:
        raise ValueError("plane must be a contiguous 2-D uint8 / int16 / uint16 / int32 / float32 / float64 HBM tensor")
    h, w = plane.shape
    if h == 0 or w == 0:
        raise ValueError("plane must not be empty")
    check_blur_sigma(sigma)
    out = _like_plane(out, plane, "out")
    if float(sigma) <= 1e-15:
        if out.data_ptr() != plane.data_ptr():
            out.copy_(plane)
        return out
    tmp = _like_plane(tmp, plane, "tmp")
    weights, radius = gaussian_kernel1d(float(sigma))
    args = (plane.data_ptr(), out.data_ptr(), tmp.data_ptr(), h, w, PLANE_MODE_DTYPES[plane.dtype], weights.ctypes.data, radius)
    if mode_entry:
        _capi.call("pxsom_gaussian_blur_plane_mode", *args, BLUR_MODES[mode], _capi.stream_ptr())
    else:
        _capi.call("pxsom_gaussian_blur_plane", *args, _capi.stream_ptr())
    return out


def gaussian_blur_plane(plane: torch.Tensor, sigma: float, out: Optional[torch.Tensor] = None,
                        tmp: Optional[torch.Tensor] = None, mode: str = "reflect") -> torch.Tensor:
    """scipy.ndimage.gaussian_filter(plane, sigma, mode=mode) of a contiguous ``[H, W]`` HBM plane in its own dtype (uint8,
    int16, uint16, int32, float32 or float64): each pass stored in that dtype, as scipy stores it.  sigma <= 1e-15 skips
    both axes (scipy's rule): the result is a copy.  ``out`` may be ``plane`` itself.  ``mode``: scipy's border, "reflect"
    (the default) or "nearest".  The default mode on the five dtypes up to float32 is pxsom_gaussian_blur_plane, route and
    bits as before the keyword existed; "nearest", and float64 planes (which this function used to refuse) under either
    mode, go to pxsom_gaussian_blur_plane_mode."""
    return _blur_plane(plane, sigma, mode, out, tmp, mode != "reflect" or plane.dtype == torch.float64)


def gaussian_blur_plane_mode(plane: torch.Tensor, sigma: float, mode: str, out: Optional[torch.Tensor] = None,
                             tmp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scipy.ndimage.gaussian_filter(plane, sigma, mode=mode) through pxsom_gaussian_blur_plane_mode: the plane blur of
    :func:`gaussian_blur_plane` with the border "reflect" or "nearest" and float64 planes beside the others."""
    return _blur_plane(plane, sigma, mode, out, tmp, True)


def zero_by_segmentation(img: torch.Tensor, seg: torch.Tensor, exclude: bool = True) -> torch.Tensor:
    """In place: ``img[seg > 0] = 0`` (``exclude``) or ``img[seg == 0] = 0`` for a contiguous HBM image (uint8, int16,
    uint16, int32 or float32) and a contiguous segmentation of the same shape (uint8 .. int64)."""
    if not img.is_cuda or not img.is_contiguous() or img.dtype not in PLANE_DTYPES:
        raise ValueError("img must be a contiguous uint8 / int16 / uint16 / int32 / float32 HBM tensor")
    if not seg.is_cuda or not seg.is_contiguous() or seg.dtype not in SEG_DTYPES:
        raise ValueError("seg must be a contiguous uint8 / int16 / uint16 / int32 / uint32 / int64 HBM tensor")
    if seg.shape != img.shape:
        raise ValueError("img and seg must have the same shape, got %s and %s" % (tuple(img.shape), tuple(seg.shape)))
    _capi.call("pxsom_zero_by_seg", img.data_ptr(), PLANE_DTYPES[img.dtype], seg.data_ptr(), SEG_DTYPES[seg.dtype],
               img.numel(), 1 if exclude else 0, _capi.stream_ptr())
    return img


# ---- object masks (K16): labelling, the area passes, the foreground predicates ----------------------------------------
SELECT_FILL, SELECT_KEEP = 0, 1                      # include/pxsom.h PXSOM_SELECT_*
BIN_POSITIVE, BIN_LEVEL, BIN_LOCAL = 0, 1, 2         # PXSOM_BIN_*
CCL_TILE = 64                                        # kTile of csrc/pxsom_ccl.hip


def label_components(fg: torch.Tensor, connectivity: int, invert: bool = False, out: Optional[torch.Tensor] = None,
                     capacity: Optional[int] = None):
    """``skimage.measure.label(fg != 0, connectivity=connectivity)`` of a ``[H, W]`` uint8 / bool HBM plane (rows
    contiguous, any row stride); with ``invert`` the pixels equal to 0 are the foreground.  Returns ``(labels, n, areas)``,
    all in HBM: ``labels`` int32 ``[H, W]`` (``out`` if given: rows contiguous, any row stride), background 0, components
    numbered by their first pixel in raster order; ``n`` int32 ``[1]``, the count; ``areas`` int32 ``[capacity]`` with
    ``areas[0]`` the background pixels (default capacity: every image's worst case, ``(H W + 1) // 2 + 1``)."""
    fg = _binary_plane(fg, "fg")
    h, w = fg.shape
    if connectivity not in (1, 2):
        raise ValueError("connectivity must be 1 or 2, got %r" % (connectivity,))
    labels = _label_plane(out, h, w, fg.device, "out")
    capacity = (h * w + 1) // 2 + 1 if capacity is None else int(capacity)
    n = torch.empty(1, dtype=torch.int32, device=fg.device)
    areas = torch.empty(capacity, dtype=torch.int32, device=fg.device)
    lib = _capi.lib()
    wsb = lib.pxsom_label_components_workspace_bytes(h, w)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=fg.device)
    _capi.call("pxsom_label_components", fg.data_ptr(), h, w, _ld(fg), int(connectivity), int(bool(invert)), labels.data_ptr(),
               _ld(labels), n.data_ptr(), areas.data_ptr(), capacity, ws.data_ptr(), wsb,
               _capi.stream_ptr())
    return labels, n, areas


def components_select(labels: torch.Tensor, areas: torch.Tensor, mode: str, fg: Optional[torch.Tensor] = None,
                      area_threshold: Optional[int] = None, min_area: int = 0, max_area: Optional[int] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One pass over a label image and its area table (:func:`label_components`).
    ``mode="fill"``: ``fg | (labels != 0 & areas[labels] < area_threshold)`` as uint8, ``labels`` being those of the
    inverted ``fg`` under connectivity 1 -- ``morphology.remove_small_holes(fg, area_threshold)``.
    ``mode="keep"``: ``labels`` where ``min_area <= areas[labels] <= max_area``, else 0 (int32; not renumbered);
    ``out`` may be ``labels``."""
    if mode not in ("fill", "keep"):
        raise ValueError("mode must be 'fill' or 'keep', got %r" % (mode,))
    if labels.dim() != 2 or labels.shape[0] == 0 or labels.shape[1] == 0:
        raise ValueError("labels must be a non-empty [H, W] tensor")
    h, w = labels.shape
    labels = _label_plane(labels, h, w, labels.device, "labels")
    if areas.dtype != torch.int32 or not areas.is_cuda or areas.dim() != 1 or not areas.is_contiguous() or not areas.numel():
        raise ValueError("areas must be a contiguous int32 HBM vector")
    lim = 2 ** 62
    if mode == "fill":
        if fg is None or area_threshold is None:
            raise ValueError("mode 'fill' needs fg and area_threshold")
        fg = _binary_plane(fg, "fg")
        if fg.shape != (h, w):
            raise ValueError("fg and labels must have one shape")
        out = _rows_plane(out, h, w, torch.uint8, labels.device, "out")
        args = (SELECT_FILL, fg.data_ptr(), _ld(fg), 0, max(-lim, min(lim, int(area_threshold))))
    else:
        out = _label_plane(out, h, w, labels.device, "out")
        hi = lim if max_area is None else max(-lim, min(lim, int(np.floor(max_area))))
        args = (SELECT_KEEP, None, 0, max(-lim, min(lim, int(np.ceil(min_area)))), hi)
    _capi.call("pxsom_components_select", args[0], args[1], args[2], labels.data_ptr(), _ld(labels), areas.data_ptr(),
               areas.numel(), h, w, args[3], args[4], out.data_ptr(), _ld(out),
               _capi.stream_ptr())
    return out


def binarize_plane(plane: torch.Tensor, mode: int = BIN_POSITIVE, level: float = 0.0,
                   local: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The uint8 foreground of a contiguous float32 / float64 ``[H, W]`` HBM plane: ``v > 0`` (BIN_POSITIVE),
    ``!(v < level) & v > 0`` (BIN_LEVEL) or ``v > local`` (BIN_LOCAL, ``local`` a plane of the same dtype and shape)."""
    if plane.dim() != 2 or not plane.is_cuda or not plane.is_contiguous() or plane.dtype not in (torch.float32, torch.float64):
        raise ValueError("plane must be a contiguous 2-D float32 / float64 HBM tensor")
    if plane.numel() == 0:
        raise ValueError("plane must not be empty")
    if mode == BIN_LOCAL:
        if local is None:
            raise ValueError("BIN_LOCAL needs the local plane")
        local = _like_plane(local, plane, "local")
    h, w = plane.shape
    out = torch.empty((h, w), dtype=torch.uint8, device=plane.device)
    _capi.call("pxsom_binarize_plane", plane.data_ptr(), PLANE_MODE_DTYPES[plane.dtype], h, w, int(mode), float(level),
               local.data_ptr() if mode == BIN_LOCAL else None, out.data_ptr(), w,
               _capi.stream_ptr())
    return out


RIDGE_MAX_RADIUS, RIDGE_MAX_SCALES = 16, 8           # kRidgeMaxRadius / kRidgeMaxScales of csrc/pxsom_ridge.hip


def ridge_sign(fg: torch.Tensor, sigmas=(1, 2, 3, 4), alpha=0.5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``skimage.filters.meijering(fg != 0, sigmas, alpha, black_ridges=False) > 0`` in skimage 0.19's statement
    (include/pxsom.h "K22"; parity with skimage itself is unpinned) of a ``[H, W]`` uint8 / bool HBM plane (rows contiguous,
    any row stride) -> uint8 ``[H, W]`` of 1 / 0 in HBM (``out`` if given: rows contiguous, any row stride, not ``fg``).
    One launch of pxsom_ridge_sign.  ``H`` and ``W`` are at least 2, as np.gradient demands; up to 8 scales, each with
    ``int(4 sigma + 0.5)`` between 1 and 16."""
    fg = _binary_plane(fg, "fg")
    h, w = fg.shape
    if h < 2 or w < 2:
        raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements "
                         "are required.")
    sigmas = list(sigmas)
    if not 1 <= len(sigmas) <= RIDGE_MAX_SCALES:
        raise ValueError("ridge_sign takes 1 to %d scales, got %d" % (RIDGE_MAX_SCALES, len(sigmas)))
    if not all(float(s) > 0 and np.isfinite(float(s)) for s in sigmas) or not np.isfinite(float(alpha)):
        raise ValueError("ridge_sign takes finite sigmas > 0 and a finite alpha, got %r and %r" % (sigmas, alpha))
    kernels = [gaussian_kernel1d(float(s)) for s in sigmas]
    for s, (_, radius) in zip(sigmas, kernels):
        if not 1 <= radius <= RIDGE_MAX_RADIUS:
            raise NotImplementedError("ridge_sign: sigma %r has radius %d outside [1, %d]" % (s, radius, RIDGE_MAX_RADIUS))
    weights = np.ascontiguousarray(np.concatenate([k for k, _ in kernels]), dtype=np.float64)
    radii = np.array([r for _, r in kernels], dtype=np.int32)
    scales = np.array([float(s ** 2) for s in sigmas], dtype=np.float64)
    out = _rows_plane(out, h, w, torch.uint8, fg.device, "out")
    _capi.call("pxsom_ridge_sign", fg.data_ptr(), h, w, _ld(fg), weights.ctypes.data, radii.ctypes.data, scales.ctypes.data,
               len(sigmas), float(alpha), out.data_ptr(), _ld(out), _capi.stream_ptr())
    return out


def object_mask(img: torch.Tensor, sigma, thresh, hole_size, min_area, max_area, local_block=None, ridge=None) -> torch.Tensor:
    """The device chain of ``_create_object_mask`` on a ``[H, W]`` HBM image -> int32 ``[H, W]`` labels in HBM.
    float32 / float64 images go as they are, any other dtype is cast to float64 (skimage's ``preserve_range`` rule).
      blur       ``sigma`` None: none; else ``gaussian_filter(x, sigma, mode='nearest')`` in x's dtype
      threshold  ``thresh`` None: ``blur > 0``; an int: ``p = np.percentile(blur[blur != 0], thresh)``, foreground
                 ``!(blur < p) & blur > 0``; "auto": ``blur > gaussian_filter(blur, (local_block - 1) / 6, mode='reflect')``
      holes      ``hole_size`` None: none; else background components (4-neighbourhood) of area < hole_size are filled
      ridge      ``ridge`` None: none; a ``(sigmas, alpha)`` tuple: the foreground becomes :func:`ridge_sign` of it
                 ("projection" objects)
      labels     8-neighbourhood components, kept where ``min_area <= area <= max_area`` (not renumbered)
    The percentile is the one value read back to the host: pxsom_quantile_f32 / pxsom_quantile_nonzero with their
    ``!= 0`` keep rule (bits equal numpy's for both dtypes; a NaN pixel is dropped there where numpy's result turns NaN)."""
    if img.dim() != 2 or not img.is_cuda or img.shape[0] == 0 or img.shape[1] == 0:
        raise ValueError("img must be a non-empty 2-D HBM tensor")
    x = img if img.dtype in (torch.float32, torch.float64) else img.to(torch.float64)
    x = x.contiguous()
    blur = x if sigma is None else gaussian_blur_plane(x, sigma, mode="nearest")
    if thresh is None:
        fg = binarize_plane(blur, BIN_POSITIVE)
    elif isinstance(thresh, str):
        if thresh != "auto" or local_block is None:
            raise ValueError("thresh 'auto' needs local_block; got thresh=%r local_block=%r" % (thresh, local_block))
        local = gaussian_blur_plane(blur, (float(local_block) - 1) / 6.0, mode="reflect")
        fg = binarize_plane(blur, BIN_LOCAL, local=local)
    else:
        column = blur.reshape(-1, 1)
        q = np.true_divide(thresh, 100)        # np.percentile's own division
        p = (quantile_f32 if blur.dtype == torch.float32 else quantile_nonzero)(column, float(q), keep_mode=0)
        fg = binarize_plane(blur, BIN_LEVEL, level=float(p.item()))
    if hole_size is not None:
        holes, _, hole_areas = label_components(fg, 1, invert=True)
        fg = components_select(holes, hole_areas, "fill", fg=fg, area_threshold=hole_size)
    if ridge is not None:
        fg = ridge_sign(fg, ridge[0], ridge[1])
    labels, _, areas = label_components(fg, 2)
    return components_select(labels, areas, "keep", min_area=min_area, max_area=max_area, out=labels)


# ---- merging object masks into the cell segmentation (K18) --------------------------------------------------------------


def label_regions(seg: torch.Tensor, connectivity: int, out: Optional[torch.Tensor] = None,
                  capacity: Optional[int] = None):
    """``skimage.measure.label(seg, background=0, connectivity=connectivity)`` of a ``[H, W]`` integer HBM label plane
    (uint8 .. int64, rows contiguous, any row stride): regions of equal non-zero value, touching regions of different
    values kept apart.  Returns ``(labels, n, areas)`` with the conventions of :func:`label_components`; the default
    capacity is every image's worst case, ``H W + 1``."""
    h, w, ld = _label_image(seg, "seg")
    if connectivity not in (1, 2):
        raise ValueError("connectivity must be 1 or 2, got %r" % (connectivity,))
    labels = _label_plane(out, h, w, seg.device, "out")
    capacity = h * w + 1 if capacity is None else int(capacity)
    n = torch.empty(1, dtype=torch.int32, device=seg.device)
    areas = torch.empty(max(capacity, 0), dtype=torch.int32, device=seg.device)
    lib = _capi.lib()
    wsb = lib.pxsom_label_regions_workspace_bytes(h, w)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=seg.device)
    _capi.call("pxsom_label_regions", seg.data_ptr(), SEG_DTYPES[seg.dtype], h, w, ld, int(connectivity), labels.data_ptr(),
               _ld(labels), n.data_ptr(), areas.data_ptr(), capacity, ws.data_ptr(), wsb,
               _capi.stream_ptr())
    return labels, n, areas


def pair_overlaps(a: torch.Tensor, b: torch.Tensor, n_a: Optional[int] = None, n_b: Optional[int] = None) -> torch.Tensor:
    """The label pairs two ``[H, W]`` int32 HBM planes share: ``[P, 3]`` int32 in HBM, one row ``(a, b, pixels)`` per
    pair with ``1 <= a <= n_a``, ``1 <= b <= n_b`` (default: every positive label) and ``pixels > 0``, sorted by
    ``(a, b)``.  Two calls of pxsom_pair_overlaps: the first counts the runs of the image, which is read back and sizes
    the list and the table of the second."""
    h, w = _label_pair(a, b)
    top = 2 ** 31 - 1
    n_a, n_b = (top if v is None else int(v) for v in (n_a, n_b))
    if not (0 <= n_a <= top and 0 <= n_b <= top):
        raise ValueError("n_a and n_b must lie in 0 .. 2147483647")
    lib = _capi.lib()
    n = torch.empty(2, dtype=torch.int32, device=a.device)

    def call(pairs, capacity, ws, wsb):
        rc = lib.pxsom_pair_overlaps(a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), h, w, n_a, n_b, pairs, capacity,
                                     n.data_ptr(), ws, wsb, _capi.stream_ptr())
        _capi.check(rc, "pxsom_pair_overlaps")

    call(None, 0, None, 0)
    runs = int(n[1].item())
    if runs == 0:
        return torch.empty((0, 3), dtype=torch.int32, device=a.device)
    if runs > PAIR_CAPACITY_MAX:
        raise NotImplementedError("pair_overlaps: %d runs of label pairs are beyond the limit %d" % (runs, PAIR_CAPACITY_MAX))
    pairs = torch.empty((runs, 3), dtype=torch.int32, device=a.device)
    wsb = lib.pxsom_pair_overlaps_workspace_bytes(runs)
    ws = torch.empty(wsb, dtype=torch.uint8, device=a.device)
    call(pairs.data_ptr(), runs, ws.data_ptr(), wsb)
    count = int(n[0].item())
    if count < 0:
        raise RuntimeError("pair_overlaps: the planes changed between the two passes")
    return pairs[:count]


def merge_apply(a: torch.Tensor, b: torch.Tensor, winner: torch.Tensor, removed: torch.Tensor,
                merged: Optional[torch.Tensor] = None, remaining: Optional[torch.Tensor] = None):
    """One pass over two ``[H, W]`` int32 HBM planes with two int32 tables indexed by ``b``:
    ``merged = winner[b] != 0 ? winner[b] : a`` and ``remaining = removed[b] ? 0 : b`` (int32 planes, any row stride)."""
    h, w = _label_pair(a, b)
    for name, t in (("winner", winner), ("removed", removed)):
        if t.dtype != torch.int32 or not t.is_cuda or t.dim() != 1 or not t.is_contiguous() or not t.numel():
            raise ValueError("%s must be a contiguous int32 HBM vector" % name)
    if winner.numel() != removed.numel():
        raise ValueError("winner and removed must have one length")
    merged = _label_plane(merged, h, w, a.device, "merged")
    remaining = _label_plane(remaining, h, w, a.device, "remaining")
    _capi.call("pxsom_merge_apply", a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), h, w, winner.data_ptr(),
               removed.data_ptr(), winner.numel(), merged.data_ptr(), _ld(merged),
               remaining.data_ptr(), _ld(remaining), _capi.stream_ptr())
    return merged, remaining


def _region_tables(labels: torch.Tensor, n: int):
    """count [n] int64, sums [n, 2] int64 (row, column) and bbox [n, 4] int32 (closed) of the labels 1 .. n, on the host."""
    if n == 0:
        return np.zeros(0, np.int64), np.zeros((0, 2), np.int64), np.zeros((0, 4), np.int32)
    h, w, ld = _label_image(labels, "labels")
    dev = labels.device
    keys = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int64, device=dev)
    sums = torch.empty((n, 2), dtype=torch.int64, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    shape = torch.empty((n, 6), dtype=torch.int64, device=dev)
    lib = _capi.lib()
    wsb = lib.pxsom_region_shape_workspace_bytes(n, 1, n, 0)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    _capi.call("pxsom_region_shape", labels.data_ptr(), SEG_DTYPES[labels.dtype], ld, h, w, keys.data_ptr(), n, 1, n,
               shape.data_ptr(), count.data_ptr(), sums.data_ptr(), bbox.data_ptr(), ws.data_ptr(), wsb, 0,
               _capi.stream_ptr())
    return count.cpu().numpy(), sums.cpu().numpy(), bbox.cpu().numpy()


def choose_merges(pairs: np.ndarray, object_bbox: np.ndarray, cell_count: np.ndarray, cell_sums: np.ndarray,
                  overlap_thresh, expansion_factor):
    """The choice of merge_masks_single on the host, in the reference's float64 statements.  ``pairs`` [P, 3] sorted by
    (object, cell); ``object_bbox`` [n_o, 4] closed (row min, row max, column min, column max); ``cell_count`` [n_c] and
    ``cell_sums`` [n_c, 2] of the cells 1 .. n_c.  Returns the int32 tables ``(winner, removed)`` of n_c + 1 entries:
    the largest object that chose the cell (0: none) and whether any did.  A cell without overlap is never chosen, so
    only the cells of the pair list are candidates; they come in ascending label within an object."""
    n_c = len(cell_count)
    winner = np.zeros(n_c + 1, dtype=np.int32)
    removed = np.zeros(n_c + 1, dtype=np.int32)
    if len(pairs) == 0:
        return winner, removed
    cells = pairs[:, 1].astype(np.int64) - 1
    area = cell_count[cells].astype(np.int64)
    centroid = cell_sums[cells].astype(np.float64) / area.astype(np.float64)[:, None]      # one division per axis
    box = object_bbox[pairs[:, 0].astype(np.int64) - 1].astype(np.int64)
    inside = ((centroid[:, 0] >= box[:, 0] - expansion_factor) & (centroid[:, 0] <= box[:, 1] + expansion_factor) &
              (centroid[:, 1] >= box[:, 2] - expansion_factor) & (centroid[:, 1] <= box[:, 3] + expansion_factor))
    overlap = pairs[:, 2].astype(np.int64)
    meets = overlap / area > overlap_thresh / 100
    best_object, best_overlap, best_cell = 0, 0, 0

    def settle():
        if best_cell:
            winner[best_cell] = best_object       # objects ascend: the last to choose a cell keeps it
            removed[best_cell] = 1

    for obj, cell, ov, ok in zip(pairs[:, 0].tolist(), pairs[:, 1].tolist(), overlap.tolist(), (inside & meets).tolist()):
        if obj != best_object:
            settle()
            best_object, best_overlap, best_cell = obj, 0, 0
        if ok and ov > best_overlap:
            best_overlap, best_cell = ov, cell
    settle()
    return winner, removed


def merge_masks(object_mask: torch.Tensor, cell_mask: torch.Tensor, overlap_thresh, expansion_factor):
    """The device chain of ``merge_masks_single`` on two ``[H, W]`` integer HBM masks of one shape -> ``(merged,
    remaining)`` int32 planes in HBM.  Both masks are relabelled (:func:`label_regions`, 8-neighbourhood); every object,
    in ascending order, takes the cell with the largest overlap among the cells whose centroid lies in the object's
    closed bounding box grown by ``expansion_factor`` and whose ``overlap / area > overlap_thresh / 100`` (both compares
    strict, the smaller label on a tie).  ``merged`` is the object labels with every chosen cell painted in its object's
    label (the largest, when several chose it); ``remaining`` the relabelled cells without the chosen ones.  One small
    read-back -- the pair list and the region tables -- serves the choice (:func:`choose_merges`)."""
    if object_mask.shape != cell_mask.shape:
        raise ValueError("Both masks must have the same shape")
    objects, n_o, _ = label_regions(object_mask, 2)
    cells, n_c, cell_areas = label_regions(cell_mask, 2)
    n_o, n_c = int(n_o.item()), int(n_c.item())
    pairs = pair_overlaps(objects, cells, n_o, n_c).cpu().numpy() if n_o and n_c else np.zeros((0, 3), np.int32)
    if len(pairs):
        _, _, object_bbox = _region_tables(objects, n_o)
        _, cell_sums, _ = _region_tables(cells, n_c)
        cell_count = cell_areas[1:n_c + 1].cpu().numpy()
    else:
        object_bbox, cell_sums, cell_count = np.zeros((n_o, 4), np.int32), np.zeros((n_c, 2), np.int64), np.ones(n_c, np.int64)
    winner, removed = choose_merges(pairs, object_bbox, cell_count, cell_sums, overlap_thresh, expansion_factor)
    dev = objects.device
    return merge_apply(objects, cells, torch.from_numpy(winner).to(dev), torch.from_numpy(removed).to(dev))


# ---- fibre segmentation: distance map, histogram, markers, elevation (K25) ---------------------------------------------
HISTOGRAM_MAX_BINS = 1024                            # kMaxBins of csrc/pxsom_markers.hip
EDT_NO_BACKGROUND = "the plane has no background pixel: the distance transform is undefined"


def plane_greater(plane: torch.Tensor, level: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``plane > level`` of a ``[H, W]`` float64 HBM plane as uint8 1 / 0 (pxsom_plane_greater); a NaN pixel is 0."""
    h, w, ld = _f64_plane(plane, "plane")
    if np.isnan(float(level)):
        raise ValueError("level must not be NaN")
    out = _rows_plane(out, h, w, torch.uint8, plane.device, "out")
    _capi.call("pxsom_plane_greater", plane.data_ptr(), h, w, ld, float(level), out.data_ptr(), _ld(out), _capi.stream_ptr())
    return out


def distance_transform_edt(fg: torch.Tensor, out: Optional[torch.Tensor] = None, squared: bool = False,
                           check: bool = True) -> torch.Tensor:
    """``scipy.ndimage.distance_transform_edt(fg)`` of a ``[H, W]`` uint8 / bool HBM plane (rows contiguous, any row
    stride), scipy's bits: float64 ``[H, W]`` in HBM, or with ``squared`` the exact int32 squared distances (``out`` if
    given: that dtype, rows contiguous, any row stride).  ``H^2 + W^2`` must fit an int32 (NotImplementedError).  A plane
    without a background pixel has no answer: pxsom_distance_transform_edt writes +inf (squared: 2^31 - 1) everywhere, and
    this function reads one pixel back and raises ValueError; ``check=False`` leaves that to the caller and does not
    synchronise."""
    fg = _binary_plane(fg, "fg")
    h, w = fg.shape
    if h * h + w * w > 2 ** 31 - 1:
        raise NotImplementedError("distance_transform_edt: H^2 + W^2 of a %d x %d plane is beyond int32" % (h, w))
    out = _rows_plane(out, h, w, torch.int32 if squared else torch.float64, fg.device, "out")
    wsb = _capi.lib().pxsom_distance_transform_edt_workspace_bytes(h, w)
    ws = torch.empty(wsb, dtype=torch.uint8, device=fg.device)
    _capi.call("pxsom_distance_transform_edt", fg.data_ptr(), h, w, _ld(fg), None if squared else out.data_ptr(), _ld(out),
               out.data_ptr() if squared else None, _ld(out), ws.data_ptr(), wsb, _capi.stream_ptr())
    if check and out[0, 0].item() == (2 ** 31 - 1 if squared else float("inf")):
        raise ValueError(EDT_NO_BACKGROUND)
    return out


def plane_minmax(plane: torch.Tensor):
    """``(plane.min(), plane.max())`` of a ``[H, W]`` float64 HBM plane as two Python floats (pxsom_plane_minmax; the two
    doubles are read back).  ValueError for a plane that holds a NaN."""
    h, w, ld = _f64_plane(plane, "plane")
    both = torch.empty(2, dtype=torch.float64, device=plane.device)
    wsb = _capi.lib().pxsom_plane_minmax_workspace_bytes()
    ws = torch.empty(wsb, dtype=torch.uint8, device=plane.device)
    _capi.call("pxsom_plane_minmax", plane.data_ptr(), h, w, ld, both.data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr())
    lo, hi = both.tolist()
    if np.isnan(lo):
        raise ValueError("the plane holds a NaN")
    return lo, hi


def histogram_edges(lo: float, hi: float, nbins: int) -> np.ndarray:
    """The ``nbins + 1`` edges np.histogram makes for the range ``(lo, hi)``: ``lo == hi`` widens by 0.5 on each side."""
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("autodetected range of [%s, %s] is not finite" % (lo, hi))
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, nbins + 1, endpoint=True, dtype=np.float64)


def plane_histogram(plane: torch.Tensor, nbins: int = 256, value_range=None):
    """``np.histogram(plane, nbins)`` of a ``[H, W]`` float64 HBM plane -> ``(counts, edges)``: int64 ``[nbins]`` in HBM
    and the float64 edges on the host.  The range is the plane's own minimum and maximum (:func:`plane_minmax`, or
    ``value_range`` when the caller has them); numpy makes the edges from it on the host and pxsom_plane_histogram counts
    against them, so the counts are numpy's whatever the rounding of a bin estimate.  ValueError for NaN or an infinite
    range, as numpy raises."""
    h, w, ld = _f64_plane(plane, "plane")
    nbins = operator.index(nbins)
    if not 1 <= nbins <= HISTOGRAM_MAX_BINS:
        raise ValueError("nbins must lie in 1 .. %d, got %d" % (HISTOGRAM_MAX_BINS, nbins))
    lo, hi = plane_minmax(plane) if value_range is None else (float(value_range[0]), float(value_range[1]))
    edges = histogram_edges(lo, hi, nbins)
    counts = torch.empty(nbins, dtype=torch.int64, device=plane.device)
    _capi.call("pxsom_plane_histogram", plane.data_ptr(), h, w, ld, torch.from_numpy(edges).to(plane.device).data_ptr(), nbins,
               counts.data_ptr(), _capi.stream_ptr())
    return counts, edges


def sobel_magnitude(plane: torch.Tensor, out: Optional[torch.Tensor] = None, as_int32: bool = False) -> torch.Tensor:
    """``sqrt((a * a + b * b) / 2)`` with ``a, b = scipy.ndimage.sobel(plane, axis, mode='reflect') / 4`` of a ``[H, W]``
    float64 HBM plane, scipy's bits (pxsom_sobel_magnitude; skimage.filters.sobel sums the same 3 x 3 kernel in another
    order).  float64, or with ``as_int32`` the magnitude converted toward zero (``out`` if given: that dtype, rows
    contiguous, any row stride, not the plane)."""
    h, w, ld = _f64_plane(plane, "plane")
    out = _rows_plane(out, h, w, torch.int32 if as_int32 else torch.float64, plane.device, "out")
    _capi.call("pxsom_sobel_magnitude", plane.data_ptr(), h, w, ld, None if as_int32 else out.data_ptr(), _ld(out),
               out.data_ptr() if as_int32 else None, _ld(out), _capi.stream_ptr())
    return out


def class_markers(dist: torch.Tensor, t0: float, t1: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 ``[H, W]`` markers of a float64 HBM plane: 0, then 1 where ``dist < t0``, then 2 where ``dist > t1``
    (pxsom_class_markers)."""
    h, w, ld = _f64_plane(dist, "dist")
    if np.isnan(float(t0)) or np.isnan(float(t1)):
        raise ValueError("thresholds must not be NaN")
    out = _label_plane(out, h, w, dist.device, "out")
    _capi.call("pxsom_class_markers", dist.data_ptr(), h, w, ld, float(t0), float(t1), out.data_ptr(), _ld(out), _capi.stream_ptr())
    return out


def watershed_inputs(ridges: torch.Tensor, ridge_cutoff: float, sobel_blur: float, thresholds=None,
                     markers: Optional[torch.Tensor] = None, elevation: Optional[torch.Tensor] = None):
    """The device chain of ``segment_fibers`` between frangi and watershed on a contiguous ``[H, W]`` float64 HBM plane:

      fg        ``ridges > ridge_cutoff``                                   :func:`plane_greater`
      dist      ``gaussian_filter(distance_transform_edt(fg), 1)``           :func:`distance_transform_edt`, the plane blur
      counts    ``np.histogram(dist, 256)``                                  :func:`plane_minmax`, :func:`plane_histogram`
      t0, t1    ``thresholds(counts, edges)`` on the host (default: fiber_segmentation.threshold_multiotsu_from_histogram)
      markers   0 / 1 (``dist < t0``) / 2 (``dist > t1``), int32              :func:`class_markers`
      elevation ``sobel(gaussian_filter(dist, sobel_blur))`` as int32        the plane blur, :func:`sobel_magnitude`

    Returns ``(dist, (t0, t1), markers, elevation)``, the planes in HBM (``markers`` / ``elevation`` if given: int32, rows
    contiguous, any row stride).  The host sees the minimum and maximum (two doubles down, 257 edges up) and the 256
    counts; the thresholds return as kernel arguments.  ValueError for a plane without background (the distance map is
    +inf) and whatever ``thresholds`` raises."""
    if ridges.dim() != 2 or not ridges.is_cuda or ridges.dtype != torch.float64 or not ridges.is_contiguous() or not ridges.numel():
        raise ValueError("ridges must be a non-empty contiguous 2-D float64 HBM tensor")
    check_blur_sigma(sobel_blur)
    if thresholds is None:
        from ..segmentation.fiber_segmentation import threshold_multiotsu_from_histogram as thresholds
    fg = plane_greater(ridges, ridge_cutoff)
    edt = distance_transform_edt(fg, check=False)
    dist = gaussian_blur_plane_mode(edt, 1, "reflect")
    lo, hi = plane_minmax(dist)
    if hi == float("inf"):
        raise ValueError(EDT_NO_BACKGROUND)
    counts, edges = plane_histogram(dist, 256, (lo, hi))
    t0, t1 = (float(t) for t in thresholds(counts.cpu().numpy(), edges))
    markers = class_markers(dist, t0, t1, out=markers)
    smooth = gaussian_blur_plane_mode(dist, sobel_blur, "reflect", out=edt)
    elevation = sobel_magnitude(smooth, out=elevation, as_int32=True)
    return dist, (t0, t1), markers, elevation


# ---- fibre segmentation: the Frangi ridge filter (K26) -------------------------------------------------------------------
FRANGI_SIGMAS = (1, 3, 5, 7, 9)                      # the reference's fiber_widths, range(1, 10, 2)
GRADIENT_TOO_SMALL = ("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements "
                      "are required.")


def frangi_arguments(sigmas, beta, gamma, black_ridges=False):
    """The checked arguments of the Frangi filter, without a device: ``(sigmas, bsq, gsq)`` with ``sigmas`` a list of
    Python floats (any iterable of numbers, flattened as skimage flattens it) and ``bsq = 2 beta^2``, ``gsq = 2 gamma^2``
    in host doubles.  ValueError: no sigma, a negative one (skimage's text), sigma 0 (skimage returns zeros there: a
    deliberate narrowing), a sigma, ``beta`` or ``gamma`` that is not finite, ``beta`` or ``gamma`` <= 0.
    NotImplementedError: a sigma beyond the plane blur's radius, ``black_ridges=True``, ``gamma=None`` (skimage >= 0.20's
    data-dependent default)."""
    if black_ridges:
        raise NotImplementedError("frangi: black_ridges=True is not implemented (the reference passes False)")
    if gamma is None:
        raise NotImplementedError("frangi: gamma=None (skimage >= 0.20's data-dependent default) is not implemented; "
                                  "skimage 0.19's default is 15")
    if not isinstance(sigmas, np.ndarray) and hasattr(sigmas, "__iter__"):
        sigmas = list(sigmas)
    flat = np.asarray(sigmas, dtype=np.float64).ravel()
    if flat.size == 0:
        raise ValueError("frangi needs at least one sigma")
    if np.any(flat < 0.0):
        raise ValueError("Sigma values less than zero are not valid")
    if not np.all(np.isfinite(flat)):
        raise ValueError("frangi takes finite sigmas, got %r" % (flat.tolist(),))
    if np.any(flat == 0.0):
        raise ValueError("frangi: sigma 0 is not taken (skimage returns zeros for it)")
    for s in flat.tolist():
        check_blur_sigma(s)
    beta, gamma = float(beta), float(gamma)
    if not (np.isfinite(beta) and beta > 0 and np.isfinite(gamma) and gamma > 0):
        raise ValueError("frangi takes finite beta and gamma > 0, got %r and %r" % (beta, gamma))
    return [float(s) for s in flat], 2.0 * beta * beta, 2.0 * gamma * gamma


def frangi(plane: torch.Tensor, sigmas=FRANGI_SIGMAS, beta=0.5, gamma=15.0, scale=1.0,
           out: Optional[torch.Tensor] = None, black_ridges: bool = False) -> torch.Tensor:
    """``skimage.filters.frangi(plane, sigmas, beta=beta, gamma=gamma, black_ridges=False, mode="reflect") * scale`` in
    skimage 0.19's 2-D statement (include/pxsom.h "K26"; parity with skimage itself is unpinned) of a ``[H, W]`` float64
    HBM plane (rows contiguous, any row stride; ``H, W >= 2``) -> float64 ``[H, W]`` in HBM (``out`` if given: rows
    contiguous, any row stride, not sharing memory with the plane).  Per scale the reflect-mode plane blur runs into one
    reused temporary and one launch of pxsom_frangi_scale folds that scale's vesselness into the result, the last one
    applying ``scale``; no host synchronisation.  The arguments are those of :func:`frangi_arguments`."""
    h, w, _ = _f64_plane(plane, "plane")
    if h < 2 or w < 2:
        raise ValueError(GRADIENT_TOO_SMALL)
    sigmas, bsq, gsq = frangi_arguments(sigmas, beta, gamma, black_ridges)
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError("scale must be finite, got %r" % (scale,))
    out = _rows_plane(out, h, w, torch.float64, plane.device, "out")
    _check_apart(out, plane, "every scale blurs the plane again", what="the plane")
    x = plane.contiguous()                           # the blur takes contiguous planes
    g, tmp = torch.empty_like(x), torch.empty_like(x)
    for i, sigma in enumerate(sigmas):
        gaussian_blur_plane_mode(x, sigma, "reflect", out=g, tmp=tmp)
        _capi.call("pxsom_frangi_scale", g.data_ptr(), _ld(g), h, w, sigma ** 2, bsq, gsq, int(i == 0),
                   scale if i == len(sigmas) - 1 else 1.0, out.data_ptr(), _ld(out), _capi.stream_ptr())
    return out


def ridge_watershed_inputs(contrast: torch.Tensor, sigmas=FRANGI_SIGMAS, ridge_cutoff: float = 0.1, sobel_blur: float = 1,
                           thresholds=None, beta=0.5, gamma=15.0):
    """The device chain of ``segment_fibers`` from the contrast-adjusted plane (``equalize_adapthist``'s result, a ``[H, W]``
    float64 HBM plane) to what ``watershed`` receives: ``ridges = frangi(contrast, sigmas, beta, gamma) * 10000``
    (:func:`frangi`), then :func:`watershed_inputs` on it.  Returns ``(ridges, dist, (t0, t1), markers, elevation)``; the
    ridge map stays in HBM."""
    ridges = frangi(contrast, sigmas, beta, gamma, scale=10000.0)
    return (ridges,) + tuple(watershed_inputs(ridges, ridge_cutoff, sobel_blur, thresholds))


# ---- fibre segmentation: adaptive histogram equalisation, the front (K27) -------------------------------------------------
CLAHE_GREY_LEVELS = 2 ** 14                          # skimage's NR_OF_GRAY
CLAHE_NBINS = 256                                    # kBins of csrc/pxsom_clahe.hip


def clahe_arguments(shape, kernel_size, clip_limit=0.01, nbins=256):
    """The checked arguments of :func:`equalize_adapthist` for a plane of ``shape``, without a device: ``(k, clim,
    map_scale)`` -- the tile side ``int(kernel_size)``, the clip limit in counts (``int(clip(clip_limit * k * k, 1,
    None))``, or 2^14 for ``clip_limit <= 0``: no clipping) and ``16383 / (k * k)`` in a host double.  ValueError: a shape
    that is not ``(H, W)`` with ``H, W >= 2``, a kernel size that is not finite or below 1 (the reference divides by zero
    there), a ``clip_limit`` that is not finite.  NotImplementedError: ``nbins`` other than 256, a kernel size that is
    not a scalar (None, skimage's data-dependent default, among them), one beyond ``min(H, W)``."""
    shape = tuple(shape)
    if len(shape) != 2 or min(shape) < 2:
        raise ValueError("equalize_adapthist takes a [H, W] plane with H, W >= 2, got shape %s" % (shape,))
    if isinstance(nbins, (bool, np.bool_)) or nbins != CLAHE_NBINS:
        raise NotImplementedError("equalize_adapthist: nbins=%r; only 256 bins are implemented" % (nbins,))
    if kernel_size is None or np.ndim(kernel_size) != 0:
        raise NotImplementedError("equalize_adapthist: kernel_size=%r; only a scalar kernel size is implemented"
                                  % (kernel_size,))
    if not np.isfinite(float(kernel_size)) or int(kernel_size) < 1:
        raise ValueError("equalize_adapthist: kernel_size=%r must be finite and at least 1" % (kernel_size,))
    k = int(kernel_size)
    if k > min(shape):
        raise NotImplementedError("equalize_adapthist: kernel_size %d beyond the shorter side of a %d x %d plane is not "
                                  "implemented" % (k, shape[0], shape[1]))
    clip_limit = float(clip_limit)
    if not np.isfinite(clip_limit):
        raise ValueError("equalize_adapthist: clip_limit must be finite, got %r" % (clip_limit,))
    ke = k * k
    clim = int(np.clip(clip_limit * ke, 1, None)) if clip_limit > 0.0 else CLAHE_GREY_LEVELS
    return k, clim, (CLAHE_GREY_LEVELS - 1) / ke


def _equalize_gray(gray: torch.Tensor, k: int, clim: int, map_scale: float, out, maps_out, raw_out) -> torch.Tensor:
    """pxsom_clahe_equalize on a uint16 ``[H, W]`` HBM plane of grey levels; ``out`` is the caller's checked plane."""
    h, w = gray.shape
    nty, ntx = -(-h // k), -(-w // k)
    if maps_out is not None and (maps_out.shape != (nty, ntx, CLAHE_NBINS) or maps_out.dtype != torch.uint16 or not maps_out.is_cuda
                                 or not maps_out.is_contiguous()):
        raise ValueError("maps_out must be a contiguous [%d, %d, 256] uint16 HBM tensor" % (nty, ntx))
    if raw_out is not None:
        _rows_plane(raw_out, h, w, torch.uint16, gray.device, "raw_out")
    for name, t in (("out", out), ("maps_out", maps_out), ("raw_out", raw_out)):
        if t is not None and t.device != gray.device:
            raise ValueError("%s must be on the plane's device" % name)
    wsb = _capi.lib().pxsom_clahe_workspace_bytes(h, w, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=gray.device)
    _capi.call("pxsom_clahe_equalize", gray.data_ptr(), h, w, _ld(gray), k, min(clim, 2 ** 31 - 1), map_scale, out.data_ptr(),
               _ld(out), None if maps_out is None else maps_out.data_ptr(), None if raw_out is None else raw_out.data_ptr(),
               w if raw_out is None else _ld(raw_out), ws.data_ptr(), wsb, _capi.stream_ptr())
    return out


def equalize_adapthist(plane: torch.Tensor, kernel_size, clip_limit=0.01, nbins=256, out: Optional[torch.Tensor] = None,
                       lo_hi=None, maps_out: Optional[torch.Tensor] = None, raw_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``skimage.exposure.equalize_adapthist(plane, kernel_size, clip_limit, nbins=256)`` in skimage 0.19's statement as
    recalled (include/pxsom.h "K27"; parity with skimage itself is unpinned) of a ``[H, W]`` float64 HBM plane (rows
    contiguous, any row stride; ``H, W >= 2``) -> float64 ``[H, W]`` in [0, 1] in HBM (``out`` if given: rows contiguous,
    any row stride, not sharing memory with the plane).  pxsom_clahe_quantize turns the plane into 2^14 grey levels over
    its own minimum and maximum; pxsom_clahe_equalize builds the clipped tile maps, interpolates and rescales, its minimum
    and maximum never leaving the device.  One host synchronisation at most: :func:`plane_minmax`, skipped when the caller
    has ``lo_hi = (min, max)``.  ``maps_out`` (uint16 ``[ceil(H / k), ceil(W / k), 256]``, contiguous) and ``raw_out``
    (uint16 ``[H, W]``, rows contiguous) receive the tile maps and the interpolated plane before the last rescale.  The
    arguments are those of :func:`clahe_arguments`; ValueError for a plane that holds a NaN or an infinity."""
    h, w, ld = _f64_plane(plane, "plane")
    k, clim, map_scale = clahe_arguments((h, w), kernel_size, clip_limit, nbins)
    out = _rows_plane(out, h, w, torch.float64, plane.device, "out")
    _check_apart(out, plane, "the result is written while the caller may still hold the plane")
    lo, hi = plane_minmax(plane) if lo_hi is None else (float(lo_hi[0]), float(lo_hi[1]))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError("equalize_adapthist takes a finite plane, its range is [%r, %r]" % (lo, hi))
    gray = torch.empty((h, w), dtype=torch.uint16, device=plane.device)
    _capi.call("pxsom_clahe_quantize", plane.data_ptr(), h, w, ld, lo, hi, gray.data_ptr(), w, _capi.stream_ptr())
    return _equalize_gray(gray, k, clim, map_scale, out, maps_out, raw_out)


def contrast_adjust(channel: torch.Tensor, blur=2.0, kernel_size=8, clip_limit=0.01, out: Optional[torch.Tensor] = None,
                    maps_out: Optional[torch.Tensor] = None, raw_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The front of ``segment_fibers`` on a contiguous ``[H, W]`` float64 HBM plane (``H, W >= 2``):
    ``b = gaussian_filter(channel, blur)`` (:func:`gaussian_blur_plane_mode`, reflect), ``b / b.max()``
    (pxsom_plane_divide, in place) and :func:`equalize_adapthist` of it -> float64 ``[H, W]`` in [0, 1] in HBM.  One
    :func:`plane_minmax` of the blurred plane serves the division and the first rescale: division by a positive number
    is monotone, so the divided plane's range is ``[min / max, 1.0]``.  ValueError for a NaN in the blurred plane or a
    maximum that is not finite and positive (the reference produces NaNs there); otherwise the errors of
    :func:`clahe_arguments` and the plane blur."""
    if channel.dim() != 2 or not channel.is_cuda or channel.dtype != torch.float64 or not channel.is_contiguous() or not channel.numel():
        raise ValueError("channel must be a non-empty contiguous 2-D float64 HBM tensor")
    h, w = channel.shape
    k, clim, map_scale = clahe_arguments((h, w), kernel_size, clip_limit)
    check_blur_sigma(blur)
    out = _rows_plane(out, h, w, torch.float64, channel.device, "out")
    _check_apart(out, channel, "the result is written while the caller may still hold the channel")
    b = gaussian_blur_plane_mode(channel, blur, "reflect")
    lo, hi = plane_minmax(b)
    if not (np.isfinite(hi) and hi > 0.0 and np.isfinite(lo)):
        raise ValueError("contrast_adjust: the blurred channel's range [%r, %r] must be finite with a positive maximum" % (lo, hi))
    _capi.call("pxsom_plane_divide", b.data_ptr(), h, w, w, hi, b.data_ptr(), w, _capi.stream_ptr())
    gray = torch.empty((h, w), dtype=torch.uint16, device=channel.device)
    _capi.call("pxsom_clahe_quantize", b.data_ptr(), h, w, w, lo / hi, 1.0, gray.data_ptr(), w, _capi.stream_ptr())
    return _equalize_gray(gray, k, clim, map_scale, out, maps_out, raw_out)


def channel_watershed_inputs(channel: torch.Tensor, blur=2.0, kernel_size=8, sigmas=FRANGI_SIGMAS, ridge_cutoff: float = 0.1,
                             sobel_blur: float = 1, thresholds=None, clip_limit=0.01, beta=0.5, gamma=15.0):
    """The device chain of ``segment_fibers`` from the raw channel (a contiguous ``[H, W]`` float64 HBM plane) to what
    ``watershed`` receives: :func:`contrast_adjust`, then :func:`ridge_watershed_inputs` on its result.  Returns
    ``(contrast, ridges, dist, (t0, t1), markers, elevation)``; every plane stays in HBM."""
    contrast = contrast_adjust(channel, blur, kernel_size, clip_limit)
    return (contrast,) + tuple(ridge_watershed_inputs(contrast, sigmas, ridge_cutoff, sobel_blur, thresholds, beta, gamma))


# ---- fibre segmentation: the marker watershed, and the chain to filtered labels (K28) ---------------------------------------
WATERSHED_STATS = ("rounds", "levels", "descents", "labelled")     # the four int64 of pxsom_watershed's stats_host


def _i32_plane(plane: torch.Tensor, what: str):
    """``(h, w, ld)`` of a non-empty ``[H, W]`` int32 HBM plane with contiguous rows (any row stride)."""
    if plane.dim() != 2 or not plane.is_cuda or plane.dtype != torch.int32:
        raise ValueError("%s must be a 2-D int32 HBM tensor" % what)
    h, w = plane.shape
    if h == 0 or w == 0:
        raise ValueError("%s must not be empty" % what)
    if w > 1 and plane.stride(1) != 1:
        raise ValueError("%s rows must be contiguous (stride(1) == 1)" % what)
    return h, w, _ld(plane)


def watershed(elevation: torch.Tensor, markers: torch.Tensor, out: Optional[torch.Tensor] = None, return_stats: bool = False):
    """``skimage.segmentation.watershed(elevation, markers)`` at its defaults in skimage 0.19's statement as recalled
    (include/pxsom.h "K28"; parity with skimage itself is unpinned) of two ``[H, W]`` int32 HBM planes (rows contiguous, any
    row stride) -> int32 ``[H, W]`` labels in HBM (``out`` if given: rows contiguous, any row stride, sharing no memory with
    the inputs).  Any non-zero marker is a label; without a marker the result is all zeros.  pxsom_watershed drives its
    rounds from the host and synchronises once per round (a 40-byte read-back); no plane crosses.  With ``return_stats``
    the result is ``(labels, stats)``, ``stats`` a dict of ``WATERSHED_STATS``: rounds, levels visited, rounds that took the
    basin path, pixels the flood labelled."""
    h, w, lde = _i32_plane(elevation, "elevation")
    _, _, ldm = _i32_plane(markers, "markers")
    if markers.shape != elevation.shape:
        raise ValueError("elevation and markers must have one shape, got %s and %s" % (tuple(elevation.shape), tuple(markers.shape)))
    if markers.device != elevation.device:
        raise ValueError("markers must be on the elevation's device")
    out = _label_plane(out, h, w, elevation.device, "out")
    if out.device != elevation.device:
        raise ValueError("out must be on the elevation's device")
    for name, t in (("elevation", elevation), ("markers", markers)):
        _check_apart(out, t, "the labels grow in out while %s is still read" % name)
    wsb = _capi.lib().pxsom_watershed_workspace_bytes(h, w)
    if wsb == 0:
        raise NotImplementedError("watershed: a %d x %d plane is beyond int32 pixels" % (h, w))
    ws = torch.empty(wsb, dtype=torch.uint8, device=elevation.device)
    stats = np.zeros(len(WATERSHED_STATS), dtype=np.int64)
    _capi.call("pxsom_watershed", elevation.data_ptr(), lde, markers.data_ptr(), ldm, h, w, out.data_ptr(), _ld(out),
               ws.data_ptr(), wsb, stats.ctypes.data, _capi.stream_ptr())
    return (out, dict(zip(WATERSHED_STATS, (int(s) for s in stats)))) if return_stats else out


def channel_fiber_labels(channel: torch.Tensor, blur=2.0, kernel_size=8, sigmas=FRANGI_SIGMAS, ridge_cutoff: float = 0.1,
                         sobel_blur: float = 1, thresholds=None, min_fiber_size: int = 15, clip_limit=0.01, beta=0.5,
                         gamma=15.0):
    """``segment_fibers`` from the raw channel (a contiguous ``[H, W]`` float64 HBM plane) to its filtered fibre labels, as
    one chain on the device: :func:`channel_watershed_inputs`, :func:`watershed` of its elevation and markers, the pixels
    labelled 2 (the reference's ``watershed(...) - 1``) as the mask, :func:`label_components` (4-connected) and
    :func:`components_select` ("keep", ``min_area=min_fiber_size``; not renumbered).  Returns ``(labels, contrast, ridges,
    dist, (t0, t1), markers, elevation)``: the int32 labels and the planes the debug files need, all in HBM.  The host sees
    what the K25 chain and the watershed's rounds read back, never a plane."""
    contrast, ridges, dist, t, markers, elevation = channel_watershed_inputs(channel, blur, kernel_size, sigmas, ridge_cutoff,
                                                                             sobel_blur, thresholds, clip_limit, beta, gamma)
    flooded = watershed(elevation, markers)
    labels, _, areas = label_components(flooded == 2, connectivity=1)
    labels = components_select(labels, areas, "keep", min_area=int(min_fiber_size), out=labels)
    return labels, contrast, ridges, dist, t, markers, elevation
