"""Pixel pre-processing: the channel blur, row and column normalisation, the exact quantiles."""
from typing import Optional

import numpy as np
import torch

from .. import _capi


def gaussian_kernel1d(sigma: float, truncate: float = 4.0):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius): host numpy, as scipy builds it."""
    radius = int(truncate * float(sigma) + 0.5)
    sigma2 = sigma * sigma
    xs = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * xs ** 2)
    phi_x = phi_x / phi_x.sum()
    return np.ascontiguousarray(phi_x[::-1], dtype=np.float64), radius


def gaussian_blur_hwc(img: torch.Tensor, sigma: float, tmp: Optional[torch.Tensor] = None,
                      f32_semantics: bool = False, generic_form: bool = False) -> torch.Tensor:
    """In-place per-channel Gaussian blur of an [H, W, C] float64 HBM image (scipy semantics).
    ``f32_semantics``: the values are widened float32 and every pass is stored as float32, as scipy does
    for a float32 image."""
    if img.dtype != torch.float64 or not img.is_cuda or not img.is_contiguous() or img.dim() != 3:
        raise ValueError("image must be a contiguous float64 [H, W, C] HBM tensor")
    h, w, c = img.shape
    if tmp is None:
        tmp = torch.empty_like(img)
    weights, radius = gaussian_kernel1d(sigma)
    _capi.call("pxsom_gaussian_blur_hwc", img.data_ptr(), tmp.data_ptr(), h, w, c,
               weights.ctypes.data, radius,
               int(bool(f32_semantics)) | (2 if generic_form else 0), _capi.stream_ptr())
    return img


def rowsum_filter_normalize(x: torch.Tensor, thresh: float, f32_semantics: bool = False):
    """(rows [m, C] f64 = x_i / rowsum_i for kept pixels, flat pixel index [m] i64), compacted in order.
    ``f32_semantics``: widened float32 values, row sum and division in binary32 (a float32 pandas frame)."""
    if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
        raise ValueError("matrix must be a contiguous float64 [N, C] HBM tensor")
    n, c = x.shape
    out = torch.empty_like(x)
    idx = torch.empty(n, dtype=torch.int64, device=x.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=x.device)
    wsb = _capi.lib().pxsom_rownorm_workspace_bytes(n)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=x.device)
    _capi.call("pxsom_rowsum_filter_normalize", x.data_ptr(), n, c, float(thresh), out.data_ptr(),
               idx.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb,
               int(bool(f32_semantics)), _capi.stream_ptr())
    m = int(cnt.item())
    return out[:m], idx[:m]


def normalize_columns(x: torch.Tensor, norm: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if x.dtype != torch.float64 or norm.dtype != torch.float64:
        raise ValueError("normalize_columns works in float64 like the reference")
    n, c = x.shape
    if out is None:
        out = torch.empty((n, c), dtype=torch.float64, device=x.device)
    _capi.call("pxsom_normalize_columns", x.data_ptr(), n, c, x.stride(0) if n > 1 else c, norm.data_ptr(),
               out.data_ptr(), out.stride(0) if n > 1 else c, _capi.stream_ptr())
    return out


def quantile_nonzero(x: torch.Tensor, q: float, keep_mode: int = 0) -> torch.Tensor:
    """Exact type-7 quantile of the kept (non-zero / positive) values of every column -> [C] f64."""
    if x.dtype != torch.float64 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("matrix must be a float64 [N, C] HBM tensor with contiguous rows")
    n, c = x.shape
    out = torch.empty(c, dtype=torch.float64, device=x.device)
    wsb = _capi.lib().pxsom_quantile_workspace_bytes(n, c)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    _capi.call("pxsom_quantile_nonzero", x.data_ptr(), n, c, x.stride(0) if n > 1 else c, float(q),
               int(keep_mode), out.data_ptr(), ws.data_ptr(), wsb,
               _capi.stream_ptr())
    return out


def to_numpy(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


def quantile_f32(x: torch.Tensor, q: float, keep_mode: int = 1) -> torch.Tensor:
    """``np.quantile`` of the kept values of every float32 column, in numpy's float32 arithmetic
    (keep_mode 1: > 0, 2: every non-NaN value) -> [C] float32."""
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("matrix must be a float32 [N, C] HBM tensor with contiguous rows")
    n, c = x.shape
    out = torch.empty(c, dtype=torch.float64, device=x.device)
    wsb = _capi.lib().pxsom_quantile_workspace_bytes(n, c)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    _capi.call("pxsom_quantile_f32", x.data_ptr(), n, c, x.stride(0) if n > 1 else c, float(q), int(keep_mode),
               out.data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr())
    return out.to(torch.float32)


def scaled_rowsum(img: torch.Tensor, norm: torch.Tensor) -> torch.Tensor:
    """``np.sum(img / norm, axis=-1)`` for [N, C] pixels and [C] divisors of one floating type (float32: numpy's
    binary32 arithmetic; float64: what numpy computes for every other image dtype), in numpy's summation
    order -> [N] of that type."""
    if img.dtype not in (torch.float32, torch.float64) or norm.dtype != img.dtype or not img.is_cuda \
            or img.dim() != 2 or img.stride(1) != 1:
        raise ValueError("img must be a float32 / float64 [N, C] HBM tensor with contiguous rows, norm [C] of the same type")
    n, c = img.shape
    out = torch.empty(n, dtype=img.dtype, device=img.device)
    _capi.call("pxsom_scaled_rowsum_f32" if img.dtype == torch.float32 else "pxsom_scaled_rowsum_f64",
               img.data_ptr(), n, c, img.stride(0) if n > 1 else c, norm.contiguous().data_ptr(), out.data_ptr(),
               _capi.stream_ptr())
    return out


def scaled_rowsum_f32(img: torch.Tensor, norm: torch.Tensor) -> torch.Tensor:
    if img.dtype != torch.float32 or norm.dtype != torch.float32:
        raise ValueError("img must be a float32 [N, C] HBM tensor with contiguous rows, norm float32 [C]")
    return scaled_rowsum(img, norm)
