"""The argument checks and dtype-code tables that the kernel families of som_device share."""
import operator
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _capi


def _matrix_args(x: torch.Tensor) -> Tuple[int, int, int, int]:
    if x.dim() != 2:
        raise ValueError("pixel matrix must be 2-D [rows, channels]")
    if not x.is_cuda:
        raise ValueError("pixel matrix must live in HBM (a cuda/HIP tensor)")
    n, c = x.shape
    if n == 0:                         # an empty shard (more ranks than rows): no element, no stride to check
        return 0, c, c, _capi.dtype_code(x)
    if c > 1 and x.stride(1) != 1:     # (a single column has no second stride to speak of: torch reports anything)
        raise ValueError("pixel matrix rows must be contiguous (stride(1) == 1)")
    ldx = x.stride(0) if n > 1 else max(c, x.stride(0))
    return n, c, ldx, _capi.dtype_code(x)


def _codebook(w: torch.Tensor) -> torch.Tensor:
    if w.dtype != torch.float64 or not w.is_cuda or not w.is_contiguous() or w.dim() != 2:
        raise ValueError("codebook must be a contiguous float64 [K, C] HBM tensor")
    return w


def _check_metric(metric: int) -> int:
    code = None
    if not isinstance(metric, (bool, np.bool_)):
        try:
            code = operator.index(metric)
        except TypeError:
            pass
    if code not in _capi.METRICS:
        raise ValueError(f"unknown metric {metric!r}: FlowSOM distf 1 (Manhattan), 2 (Euclidean), 3 (Chebyshev) "
                         f"or 4 (cosine)")
    return code


# include/pxsom.h PXSOM_SEG_*: the label dtypes of a segmentation image, and float64 (an output only)
SEG_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.uint16: 2, torch.int32: 3, torch.uint32: 4, torch.int64: 5}
SEG_F64 = 6
# pxsom_gaussian_blur_plane / pxsom_zero_by_seg: the plane dtypes (PXSOM_SEG_* codes, float32 = PXSOM_SEG_F32)
PLANE_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.uint16: 2, torch.int32: 3, torch.float32: 7}
PLANE_MODE_DTYPES = {**PLANE_DTYPES, torch.float64: 6}
PAIR_CAPACITY_MAX = 1 << 27                          # kMaxPairCapacity of csrc/pxsom_pairtable.h


def _binary_plane(fg: torch.Tensor, what: str) -> torch.Tensor:
    if fg.dim() != 2 or not fg.is_cuda or fg.dtype not in (torch.uint8, torch.bool):
        raise ValueError("%s must be a 2-D uint8 or bool HBM tensor" % what)
    if fg.shape[0] == 0 or fg.shape[1] == 0:
        raise ValueError("%s must not be empty" % what)
    if fg.shape[1] > 1 and fg.stride(1) != 1:
        raise ValueError("%s rows must be contiguous (stride(1) == 1)" % what)
    return fg.view(torch.uint8) if fg.dtype == torch.bool else fg


def _rows_plane(t: Optional[torch.Tensor], h: int, w: int, dtype, device, what: str) -> torch.Tensor:
    """``t``, checked to be a ``[h, w]`` HBM plane of ``dtype`` with contiguous rows (any row stride), or a new one."""
    if t is None:
        return torch.empty((h, w), dtype=dtype, device=device)
    if t.shape != (h, w) or t.dtype != dtype or not t.is_cuda or (w > 1 and t.stride(1) != 1):
        raise ValueError("%s must be a [H, W] %s HBM tensor with contiguous rows" % (what, str(dtype).replace("torch.", "")))
    return t


def _label_plane(t: Optional[torch.Tensor], h: int, w: int, device, what: str) -> torch.Tensor:
    return _rows_plane(t, h, w, torch.int32, device, what)


def _like_plane(t: Optional[torch.Tensor], plane: torch.Tensor, what: str) -> torch.Tensor:
    """``t``, checked to be a contiguous HBM tensor of the plane's shape and dtype, or a new one."""
    if t is None:
        return torch.empty_like(plane)
    if t.shape != plane.shape or t.dtype != plane.dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError("%s must be a contiguous HBM tensor of the plane's shape and dtype" % what)
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _f64_plane(plane: torch.Tensor, what: str):
    """``(h, w, ld)`` of a non-empty ``[H, W]`` float64 HBM plane with contiguous rows (any row stride)."""
    if plane.dim() != 2 or not plane.is_cuda or plane.dtype != torch.float64:
        raise ValueError("%s must be a 2-D float64 HBM tensor" % what)
    h, w = plane.shape
    if h == 0 or w == 0:
        raise ValueError("%s must not be empty" % what)
    if w > 1 and plane.stride(1) != 1:
        raise ValueError("%s rows must be contiguous (stride(1) == 1)" % what)
    return h, w, _ld(plane)


def _image_plane(plane: torch.Tensor, what: str):
    if plane.dim() != 2 or not plane.is_cuda or not plane.is_contiguous() or plane.dtype not in PLANE_DTYPES:
        raise ValueError("%s must be a contiguous 2-D uint8 / int16 / uint16 / int32 / float32 HBM tensor" % what)
    if plane.numel() == 0:
        raise ValueError("%s must not be empty" % what)
    return plane.shape


def _byte_range(t: torch.Tensor):
    return t.data_ptr(), t.data_ptr() + ((t.shape[0] - 1) * _ld(t) + t.shape[1]) * t.element_size()


def _check_apart(out: torch.Tensor, plane: torch.Tensor, why: str, what: str = "the input") -> None:
    lo, hi = _byte_range(out)
    plo, phi = _byte_range(plane)
    if lo < phi and plo < hi:
        raise ValueError("out must not share memory with %s: %s" % (what, why))


def _label_pair(a: torch.Tensor, b: torch.Tensor):
    for name, t in (("a", a), ("b", b)):
        if t.dim() != 2 or not t.is_cuda or t.dtype != torch.int32 or t.shape[0] == 0 or t.shape[1] == 0 or \
                (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError("%s must be a non-empty [H, W] int32 HBM plane with contiguous rows" % name)
    if a.shape != b.shape:
        raise ValueError("a and b must have one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    return a.shape


def _label_image(seg: torch.Tensor, what: str):
    if seg.dim() != 2 or not seg.is_cuda or seg.dtype not in SEG_DTYPES:
        raise ValueError("%s must be a 2-D uint8 / int16 / uint16 / int32 / uint32 / int64 HBM tensor" % what)
    h, w = seg.shape
    if h == 0 or w == 0:
        raise ValueError("%s must not be empty" % what)
    if w > 1 and seg.stride(1) != 1:
        raise ValueError("%s rows must be contiguous (stride(1) == 1)" % what)
    return h, w, seg.stride(0) if h > 1 else w


def _key_range(keys: torch.Tensor):
    if keys.dtype != torch.int32 or keys.dim() != 1 or not keys.is_cuda or not keys.is_contiguous():
        raise ValueError("keys must be a contiguous int32 HBM vector")
    if keys.numel() == 0:
        return 0, 0
    lo, hi = (int(v) for v in keys[[0, -1]].cpu())
    return lo, hi
