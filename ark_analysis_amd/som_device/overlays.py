"""Cell overlays and coloured masks (K29): the positive-pixel percentiles, the one-pass border / rescale / compositing
kernel and the colour gather."""
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _capi
from ._args import PLANE_DTYPES, SEG_DTYPES, _image_plane, _label_image
from .pixels import quantile_nonzero

OVERLAY_ZERO, OVERLAY_RESCALE, OVERLAY_CLIP = 0, 1, 2     # include/pxsom.h PXSOM_OVERLAY_*
COLORIZE_BAD_INDEX = 1                                    # PXSOM_COLORIZE_BAD_INDEX
COLORIZE_MASK_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.uint16: 2, torch.int32: 3}   # PXSOM_SEG_* codes


def _as_float64_column(plane: torch.Tensor) -> torch.Tensor:
    """The integer plane as a float64 ``[H * W, 1]`` column (uint16 through its int16 bits)."""
    if plane.dtype == torch.uint16:
        plane = plane.view(torch.int16).to(torch.int32) & 0xFFFF
    col = torch.empty((plane.numel(), 1), dtype=torch.float64, device=plane.device)     # (canonical strides for one pixel too)
    col.copy_(plane.reshape(-1, 1))
    return col


def percentiles_positive(plane: torch.Tensor, q: Sequence[float] = (5, 95)) -> torch.Tensor:
    """``np.percentile(plane[plane > 0], q)`` for a LIST ``q`` of a contiguous ``[H, W]`` HBM plane (uint8, int16, uint16,
    int32 or float32) -> float64 ``[len(q)]`` in HBM, NaN when no pixel is positive.  A float32 plane goes through
    pxsom_percentile_f32_listq (numpy's mixed arithmetic for a list of q: index and fraction binary64, ``b - a`` binary32,
    interpolation binary64); an integer plane is cast to float64 and goes through pxsom_quantile_nonzero, which is what
    numpy computes for it."""
    _image_plane(plane, "plane")
    qs = np.ascontiguousarray([float(v) / 100 for v in q], dtype=np.float64)
    if qs.ndim != 1 or qs.size == 0 or not np.all((qs >= 0) & (qs <= 1)):
        raise ValueError("Percentiles must be in the range [0, 100]")
    if plane.dtype != torch.float32:
        col = _as_float64_column(plane)
        return torch.cat([quantile_nonzero(col, float(v), keep_mode=1) for v in qs])
    n = plane.numel()
    out = torch.empty(qs.size, dtype=torch.float64, device=plane.device)
    wsb = _capi.lib().pxsom_quantile_workspace_bytes(n, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=plane.device)
    _capi.call("pxsom_percentile_f32_listq", plane.data_ptr(), n, 1, 1, qs.ctypes.data, int(qs.size), 1, out.data_ptr(),
               ws.data_ptr(), wsb, _capi.stream_ptr())
    return out


def overlay_compose(rgb_planes, modes, ranges, seg: torch.Tensor, alt: Optional[torch.Tensor] = None, want_rgb: bool = True,
                    want_borders: bool = False, rgb: Optional[torch.Tensor] = None, borders: Optional[torch.Tensor] = None):
    """One launch of pxsom_overlay_rgb.  ``rgb_planes``: the planes of the red, green and blue byte (None where the mode is
    OVERLAY_ZERO), ``modes`` and ``ranges`` ``[(lo, hi)] * 3`` per output byte; ``seg`` and ``alt`` contiguous ``[H, W]``
    label planes.  Returns ``(rgb, borders)``: uint8 ``[H, W, 3]`` and uint8 ``[H, W]`` (0 / 255), None where not wanted."""
    h, w, ld = _label_image(seg, "seg")
    if ld != w:
        raise ValueError("seg must be contiguous")
    if alt is not None:
        if _label_image(alt, "alt") != (h, w, w) or alt.device != seg.device:
            raise ValueError("alt must be a contiguous label plane of seg's shape on seg's device")
    code = None
    ptrs = [None, None, None]
    modes = [int(m) for m in modes]
    if want_rgb:
        for j, plane in enumerate(rgb_planes):
            if modes[j] == OVERLAY_ZERO:
                continue
            if plane is None or tuple(_image_plane(plane, "plane")) != (h, w) or plane.device != seg.device:
                raise ValueError("every plane must have seg's shape and lie on seg's device")
            if code is not None and PLANE_DTYPES[plane.dtype] != code:
                raise ValueError("the planes must have one dtype")
            code = PLANE_DTYPES[plane.dtype]
            ptrs[j] = plane.data_ptr()
        if rgb is None:
            rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=seg.device)
        elif rgb.shape != (h, w, 3) or rgb.dtype != torch.uint8 or not rgb.is_cuda or not rgb.is_contiguous():
            raise ValueError("rgb must be a contiguous uint8 [H, W, 3] HBM tensor")
    else:
        rgb = None
    if want_borders:
        if borders is None:
            borders = torch.empty((h, w), dtype=torch.uint8, device=seg.device)
        elif borders.shape != (h, w) or borders.dtype != torch.uint8 or not borders.is_cuda or not borders.is_contiguous():
            raise ValueError("borders must be a contiguous uint8 [H, W] HBM tensor")
    else:
        borders = None
    modes_host = np.ascontiguousarray(modes, dtype=np.int32)
    ranges_host = np.ascontiguousarray(ranges, dtype=np.float64).reshape(3, 2)
    _capi.call("pxsom_overlay_rgb", ptrs[0], ptrs[1], ptrs[2], 0 if code is None else code, modes_host.ctypes.data,
               ranges_host.ctypes.data, seg.data_ptr(), SEG_DTYPES[seg.dtype], alt.data_ptr() if alt is not None else None,
               SEG_DTYPES[alt.dtype] if alt is not None else 0, h, w, rgb.data_ptr() if rgb is not None else None,
               borders.data_ptr() if borders is not None else None, _capi.stream_ptr())
    return rgb, borders


def _channel_planes(planes):
    """``planes`` as a list of contiguous 2-D planes: None, one ``[H, W]`` tensor, an ``[H, W, c]`` tensor or a sequence."""
    if planes is None:
        return []
    if isinstance(planes, torch.Tensor):
        if planes.dim() == 2:
            return [planes.contiguous()]
        if planes.dim() != 3:
            raise ValueError("plotting tif must be 2D or 3D array, got {}".format(tuple(planes.shape)))
        if planes.shape[2] > 3:
            raise ValueError("max 3 channels of overlay supported, got {}".format(tuple(planes.shape)))
        return [planes[..., i].contiguous() for i in range(planes.shape[2])]
    planes = list(planes)
    if len(planes) > 3:
        raise ValueError("max 3 channels of overlay supported, got {}".format(len(planes)))
    return [p.contiguous() for p in planes]


def overlay_ranges(channels, channel_names=None):
    """Mode and ``(lo, hi)`` of every channel plane, from its maximum and ``percentiles_positive(plane, (5, 95))``: mode
    OVERLAY_ZERO for a maximum of 0, OVERLAY_CLIP where the two percentiles are equal, else OVERLAY_RESCALE.  ValueError,
    naming the channel, for a non-zero maximum without a positive pixel (the reference fails inside numpy there).  Two
    read-backs: the maxima, then the percentiles."""
    if not channels:
        return [], []
    flags = []
    for plane in channels:
        _image_plane(plane, "plane")
        if plane.dtype == torch.uint16:            # unsigned: the maximum is 0 only if every pixel is
            flags.append((plane.view(torch.int16) != 0).any().to(torch.float64))
        else:
            flags.append(plane.max().to(torch.float64))
    maxima = torch.stack(flags).cpu().numpy()
    for i, mx in enumerate(maxima):
        if mx != 0 and not mx > 0:
            name = channel_names[i] if channel_names is not None else i
            raise ValueError("channel %s has a non-zero maximum but no positive pixel: its percentiles are undefined" % (name,))
    live = [i for i, mx in enumerate(maxima) if mx != 0]
    modes, ranges = [OVERLAY_ZERO] * len(channels), [(0.0, 0.0)] * len(channels)
    if live:
        got = torch.stack([percentiles_positive(channels[i], (5, 95)) for i in live]).cpu().numpy()
        for i, (lo, hi) in zip(live, got):
            modes[i] = OVERLAY_CLIP if lo == hi else OVERLAY_RESCALE
            ranges[i] = (float(lo), float(hi))
    return modes, ranges


def overlay_rgb(planes, seg: torch.Tensor, alt: Optional[torch.Tensor] = None, want_borders: bool = False,
                channel_names=None):
    """The body of the reference's ``create_overlay`` on resident tensors: ``planes`` one ``[H, W]`` plane (it goes to
    blue), an ``[H, W, c]`` image or up to three planes (channel ``i`` goes to byte ``2 - i``) of one dtype (uint8, int16,
    uint16, int32 or float32); every channel with a non-zero maximum is rescaled from the 5th .. 95th percentile of its
    positive pixels to 0 .. 255 (skimage 0.19's ``rescale_intensity`` as recalled), then the inner borders of ``seg`` are
    drawn white and those of ``alt`` red.  Returns the uint8 ``[H, W, 3]`` image, or ``(image, borders)`` with
    ``want_borders`` (uint8 ``[H, W]``, 255 on a border of ``seg``).  ``planes=None``: the borders alone.  The chain is torch
    maxima, the percentile selects and one launch of pxsom_overlay_rgb; the host reads back the maxima and the percentiles.
    A NaN pixel gives an unspecified byte."""
    channels = _channel_planes(planes)
    if planes is None:
        return overlay_compose([None] * 3, [OVERLAY_ZERO] * 3, [(0.0, 0.0)] * 3, seg, alt, want_rgb=False, want_borders=True)[1]
    for plane in channels:
        if tuple(_image_plane(plane, "plane")) != tuple(seg.shape):
            raise ValueError("every plane must have seg's shape, got %s and %s" % (tuple(plane.shape), tuple(seg.shape)))
    modes, ranges = overlay_ranges(channels, channel_names)
    rgb_planes, rgb_modes, rgb_ranges = [None] * 3, [OVERLAY_ZERO] * 3, [(0.0, 0.0)] * 3
    for i, plane in enumerate(channels):
        rgb_planes[2 - i], rgb_modes[2 - i], rgb_ranges[2 - i] = plane, modes[i], ranges[i]
    rgb, borders = overlay_compose(rgb_planes, rgb_modes, rgb_ranges, seg, alt, want_rgb=True, want_borders=want_borders)
    return (rgb, borders) if want_borders else rgb


def colorize(mask: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None):
    """``table[mask]`` for a contiguous ``[H, W]`` HBM mask (uint8, int16, uint16 or int32) and a contiguous uint8
    ``[n, 3]`` or ``[n, 4]`` HBM table -> ``(out, status)``: uint8 ``[H, W, 3 | 4]`` and 0 or COLORIZE_BAD_INDEX when an
    index lies outside ``[0, n)`` (such pixels are zeros; negative indices do not wrap).  Synchronises to read the
    status."""
    if mask.dim() != 2 or not mask.is_cuda or not mask.is_contiguous() or mask.dtype not in COLORIZE_MASK_DTYPES \
            or mask.numel() == 0:
        raise ValueError("mask must be a non-empty contiguous 2-D uint8 / int16 / uint16 / int32 HBM tensor")
    if table.dim() != 2 or table.dtype != torch.uint8 or not table.is_cuda or not table.is_contiguous() \
            or table.shape[0] < 1 or table.shape[1] not in (3, 4) or table.device != mask.device:
        raise ValueError("table must be a contiguous uint8 [n, 3] or [n, 4] HBM tensor on the mask's device")
    h, w = mask.shape
    ncol = table.shape[1]
    if out is None:
        out = torch.empty((h, w, ncol), dtype=torch.uint8, device=mask.device)
    elif out.shape != (h, w, ncol) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 [H, W, %d] HBM tensor" % ncol)
    status = torch.empty(1, dtype=torch.int32, device=mask.device)
    _capi.call("pxsom_colorize", mask.data_ptr(), COLORIZE_MASK_DTYPES[mask.dtype], h, w, table.data_ptr(), table.shape[0],
               ncol, out.data_ptr(), status.data_ptr(), _capi.stream_ptr())
    return out, int(status.item())
