"""Cell geometry: the neighbourhood matrix (K13), close-pair counts (K20), nearest-type distances (K14), nearest
points (K23), neighbourhood feature sums (K24)."""
import operator
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _capi


# ---- neighbourhood matrix (K13) -------------------------------------------------------------------------------------
def _smallest_double(pred):
    """The smallest double s in [0, +inf] with ``pred(s)`` for a monotone pred (False, ..., False, True, ..., True),
    as its bit pattern; None when pred(+inf) is False.  Non-negative doubles order as their bit patterns do."""
    def at(bits):
        return bool(pred(np.array(bits, dtype=np.uint64).view(np.float64)[()]))
    lo, hi = 0, 0x7FF0000000000000
    if not at(hi):
        return None
    if at(lo):
        return lo
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if at(mid):
            hi = mid
        else:
            lo = mid
    return hi


def neighbor_thresholds(distlim) -> Tuple[float, float]:
    """``(s_lim, s_zero)`` for pxsom_neighbor_counts: with ``d = float32(sqrt(s))`` the entry of the reference's distance
    matrix for a squared distance s, ``d < distlim`` is ``s < s_lim`` and ``d == 0`` is ``s <= s_zero``, exactly --
    sqrt and the cast to float32 are correctly rounded and monotone, so each test flips at one double, found here by
    bisection over the bit patterns.  ``distlim`` compares in the dtype numpy compares a float32 array with it in
    (``np.result_type(np.float32, distlim)``: a Python scalar in float32, an ``np.float64`` in float64)."""
    lim = np.result_type(np.float32, distlim).type(distlim)

    def d32(s):
        with np.errstate(over="ignore"):
            return np.float32(np.sqrt(s))
    at_lim = _smallest_double(lambda s: d32(s) >= lim)
    above_zero = _smallest_double(lambda s: d32(s) > 0)
    as_double = lambda bits: float(np.array(bits, dtype=np.uint64).view(np.float64)[()])  # noqa: E731
    # a NaN distlim is below nothing: s < 0 never holds
    return (0.0 if at_lim is None else as_double(at_lim)), as_double(above_zero - 1)


def _cell_args(xy: torch.Tensor, seg: torch.Tensor, check_rows):
    """The ``xy`` / ``seg`` checks of the cell-geometry calls, with the caller's checks of its per-row vectors
    (``check_rows(n, device)``) in their place between the two: ``(n, device, seg made contiguous, n_fovs)``."""
    if xy.dim() != 2 or xy.shape[1] != 2 or xy.dtype != torch.float64 or not xy.is_cuda:
        raise ValueError("xy must be an [n, 2] float64 HBM tensor")
    check_rows(xy.shape[0], xy.device)
    if seg.dim() != 1 or seg.numel() < 1 or seg.dtype != torch.int64 or seg.device != xy.device:
        raise ValueError("seg must be an [F + 1] int64 HBM vector on xy's device")
    return xy.shape[0], xy.device, seg.contiguous(), seg.numel() - 1


def _check_offsets(seg: torch.Tensor, n: int, *more) -> list:
    """ValueError unless ``seg`` is right.  A call's one read-back: it returns the values of the 0-d bools ``more``."""
    ok = torch.stack([seg[0] == 0, seg[-1] == n, (seg[1:] >= seg[:-1]).all(), *more]).cpu()
    if not bool(ok[:3].all()):
        raise ValueError("seg must be non-decreasing offsets from 0 to n")
    return ok[3:].tolist()


def _cells_sorted_by_type(xy: torch.Tensor, types: torch.Tensor, seg: torch.Tensor, n_types: int):
    """The arguments :func:`neighbor_counts` and :func:`nearest_type_means` share, checked (one read-back), and the cells
    as their kernels want them: sorted by type inside each FOV.  Returns ``(xy_s, types_s, seg, order, n_fovs)``; sorted
    row r is the caller's row ``order[r]``.  With no cells the first two and ``order`` are None."""
    def check_types(n, dev):
        if types.dim() != 1 or types.shape[0] != n or types.dtype not in (torch.int32, torch.int64) or types.device != dev:
            raise ValueError("types must be an [n] int32 / int64 HBM vector on xy's device")
    n, dev, seg, n_fovs = _cell_args(xy, seg, check_types)
    if n_types < 1:
        raise ValueError("n_types must be at least 1")
    if not _check_offsets(seg, n, ((types >= 0) & (types < n_types)).all())[0]:
        raise ValueError("types must lie in [0, n_types)")
    if n == 0:
        return None, None, seg, None, n_fovs
    rows = torch.arange(n, device=dev)
    fov = torch.searchsorted(seg[1:], rows, right=True)
    order = torch.argsort(fov * n_types + types.to(torch.int64), stable=True)
    return xy[order].contiguous(), types[order].to(torch.int32).contiguous(), seg, order, n_fovs


def neighbor_counts(xy: torch.Tensor, types: torch.Tensor, seg: torch.Tensor, n_types: int, distlim,
                    self_neighbor: bool = False) -> torch.Tensor:
    """pxsom_neighbor_counts: ``counts[i, t]`` (``[n, n_types]`` int32, HBM) = how many cells j of cell i's FOV with
    ``types[j] == t`` have ``float32(dist(i, j)) < distlim`` (and ``!= 0`` unless ``self_neighbor``), dist the binary64
    Euclidean distance of the centroids ``xy`` [n, 2] -- the reference's compute_neighbor_counts over calc_dist_matrix's
    matrix, which is never built.  ``types`` [n] int32 / int64 in [0, n_types); ``seg`` [F + 1] int64 offsets (FOV f is
    rows seg[f] .. seg[f + 1], seg[0] = 0, seg[F] = n, empty FOVs allowed).  Rows come in and go out in the caller's
    order: the sort by type inside each FOV that the kernel wants is done here."""
    n_types = operator.index(n_types)
    xy_s, types_s, seg, order, n_fovs = _cells_sorted_by_type(xy, types, seg, n_types)
    s_lim, s_zero = neighbor_thresholds(distlim)
    n = xy.shape[0]
    counts = torch.empty((n, n_types), dtype=torch.int32, device=xy.device)
    if n == 0:
        return counts
    sorted_counts = torch.empty_like(counts)
    _capi.call("pxsom_neighbor_counts", xy_s.data_ptr(), types_s.data_ptr(), seg.data_ptr(), n_fovs, n, n_types,
               s_lim, s_zero, 1 if self_neighbor else 0, sorted_counts.data_ptr(),
               _capi.stream_ptr())
    counts[order] = sorted_counts
    return counts


CLOSE_PAIR_MAX_SETS = 64    # pxsom_close_pair_counts: a set is a bit of a 64-bit membership mask


def close_pair_counts(xy: torch.Tensor, member_q: torch.Tensor, member_c: torch.Tensor, seg: torch.Tensor,
                      n_sets_q: int, n_sets_c: int, distlim, self_neighbor: bool = False) -> torch.Tensor:
    """pxsom_close_pair_counts: ``out[f, s, t]`` (``[F, n_sets_q, n_sets_c]`` int64, HBM) = the number of ordered pairs
    (a, b) of cells of FOV f with bit s of ``member_q[a]`` and bit t of ``member_c[b]`` set and
    ``float32(dist(a, b)) < distlim`` (and ``!= 0`` unless ``self_neighbor``: without it a cell pairs neither with itself
    nor with a cell on its own centroid) -- the pair test of :func:`neighbor_counts`, the N x N matrix never built.
    ``member_q`` / ``member_c`` are ``[n]`` int64 tensors holding the uint64 masks (bit 63 is the sign bit; they may be
    the same tensor); bits at or above the set counts are ignored.  ``1 <= n_sets <= 64``: callers with more sets go
    through blocks of 64 rows x 64 columns.  ``seg`` as for :func:`neighbor_counts`; the rows need no order inside a
    FOV.  The entry clears the output itself."""
    n_sets_q, n_sets_c = operator.index(n_sets_q), operator.index(n_sets_c)
    def check_members(n, dev):
        for name, m in (("member_q", member_q), ("member_c", member_c)):
            if m.dim() != 1 or m.shape[0] != n or m.dtype != torch.int64 or m.device != dev:
                raise ValueError("%s must be an [n] int64 HBM vector (the bits of a uint64 mask) on xy's device" % name)
    n, dev, seg, n_fovs = _cell_args(xy, seg, check_members)
    if not (1 <= n_sets_q <= CLOSE_PAIR_MAX_SETS and 1 <= n_sets_c <= CLOSE_PAIR_MAX_SETS):
        raise ValueError("n_sets_q and n_sets_c must lie in 1 .. %d, got %d and %d"
                         % (CLOSE_PAIR_MAX_SETS, n_sets_q, n_sets_c))
    _check_offsets(seg, n)
    s_lim, s_zero = neighbor_thresholds(distlim)
    out = torch.empty((n_fovs, n_sets_q, n_sets_c), dtype=torch.int64, device=dev)
    if n_fovs == 0:
        return out
    xy, same = xy.contiguous(), member_c is member_q
    member_q = member_q.contiguous()
    member_c = member_q if same else member_c.contiguous()
    _capi.call("pxsom_close_pair_counts", xy.data_ptr(), member_q.data_ptr(), member_c.data_ptr(), seg.data_ptr(),
               n_fovs, n, n_sets_q, n_sets_c, s_lim, s_zero, 1 if self_neighbor else 0,
               out.data_ptr(), _capi.stream_ptr())
    return out


# ---- cell-distance analysis (K14) -----------------------------------------------------------------------------------
NEAREST_MAX_K = 32      # pxsom_nearest_type_means keeps the k smallest squared distances in registers
_S_ZERO = None


def _nearest_s_zero() -> float:
    """neighbor_thresholds' s_zero (it does not depend on distlim), bisected once per process."""
    global _S_ZERO
    if _S_ZERO is None:
        _S_ZERO = neighbor_thresholds(1)[1]
    return _S_ZERO


def nearest_type_means(xy: torch.Tensor, types: torch.Tensor, seg: torch.Tensor, n_types: int, k: int) -> torch.Tensor:
    """pxsom_nearest_type_means: ``means[i, t]`` (``[n, n_types]`` float32, HBM) = the mean of the k smallest non-zero
    float32 distances from cell i to the cells j of its FOV with ``types[j] == t``, NaN when fewer than k are non-zero
    -- the reference's calculate_mean_distance_to_cell_type over calc_dist_matrix's matrix, which is never built, bit for
    bit (float32 sum in numpy's pairwise order).  Arguments as for :func:`neighbor_counts`; ``1 <= k <= 32``.  Rows come
    in and go out in the caller's order: the sort by type inside each FOV that the kernel wants is done here."""
    k = operator.index(k)
    if not 1 <= k <= NEAREST_MAX_K:
        raise ValueError("k must lie in 1 .. %d (the device route keeps the k nearest in registers), got %d"
                         % (NEAREST_MAX_K, k))
    n_types = operator.index(n_types)
    xy_s, types_s, seg, order, n_fovs = _cells_sorted_by_type(xy, types, seg, n_types)
    s_zero = _nearest_s_zero()
    n = xy.shape[0]
    means = torch.empty((n, n_types), dtype=torch.float32, device=xy.device)
    if n == 0:
        return means
    sorted_means = torch.empty_like(means)
    _capi.call("pxsom_nearest_type_means", xy_s.data_ptr(), types_s.data_ptr(), seg.data_ptr(), n_fovs, n, n_types, k,
               s_zero, sorted_means.data_ptr(), _capi.stream_ptr())
    means[order] = sorted_means
    return means


# ---- nearest points (K23) -------------------------------------------------------------------------------------------
def nearest_indices(xy: torch.Tensor, seg: torch.Tensor, k: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pxsom_nearest_indices: ``idx[i]`` (``[n, k]`` int32, HBM; ``out`` when given) = the positions in ``0 .. n - 1`` of
    the k nearest other points of point i's FOV, nearest first, ordered by ``s = fl(fl(dx * dx) + fl(dy * dy))`` in
    binary64 with ties to the lower position; i is excluded by identity, so a point on i's coordinates is a neighbour.
    A FOV with fewer than k + 1 points leaves the tail of its rows at -1.  ``xy`` [n, 2] float64 and finite, ``seg``
    [F + 1] int64 offsets as for :func:`neighbor_counts`; the rows need no order inside a FOV.  ``1 <= k <= 32``."""
    k = operator.index(k)
    if not 1 <= k <= NEAREST_MAX_K:
        raise ValueError("k must lie in 1 .. %d (the device route keeps the k nearest in registers), got %d"
                         % (NEAREST_MAX_K, k))
    n, dev, seg, n_fovs = _cell_args(xy, seg, lambda n, dev: None)
    if out is None:
        out = torch.empty((n, k), dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or tuple(out.shape) != (n, k) or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous [n, k] int32 HBM tensor on xy's device")
    if not _check_offsets(seg, n, torch.isfinite(xy).all())[0]:
        raise ValueError("xy must be finite")
    if n == 0:
        return out
    xy = xy.contiguous()
    _capi.call("pxsom_nearest_indices", xy.data_ptr(), seg.data_ptr(), n_fovs, n, k, out.data_ptr(), _capi.stream_ptr())
    return out


# ---- spatial-LDA neighbourhood sums (K24) ---------------------------------------------------------------------------
def radius_threshold(radius, closed: bool = False) -> float:
    """The double ``s_lim`` for pxsom_neighborhood_sums: for a squared distance s, ``s < s_lim`` holds exactly when
    ``np.sqrt(s) < np.float64(radius)`` (``closed``: ``<=``).  sqrt is correctly rounded and monotone, so the test flips
    at one double, found by bisection over the bit patterns as in :func:`neighbor_thresholds`.  This is not a test
    against ``radius ** 2``: for a radius that is a power of two, sqrt of the double above ``radius ** 2`` rounds down
    to ``radius``, so ``sqrt(s) <= radius`` holds where ``s <= radius ** 2`` does not.  A NaN radius is below nothing:
    0.0."""
    lim = np.float64(radius)
    if np.isnan(lim):
        return 0.0
    with np.errstate(invalid="ignore"):
        at = _smallest_double((lambda s: np.sqrt(s) > lim) if closed else (lambda s: np.sqrt(s) >= lim))
    # no double's root is beyond the radius: every finite s is inside
    return float("inf") if at is None else float(np.array(at, dtype=np.uint64).view(np.float64)[()])


def neighborhood_sums(xy: torch.Tensor, feats: Optional[torch.Tensor], seg: torch.Tensor, radius,
                      closed: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """pxsom_neighborhood_sums: ``(sums [n, p] float64, counts [n] int32)`` on the device.  ``counts[i]`` is the number
    of cells j of cell i's FOV, i included, with ``sqrt(fl(fl(dx * dx) + fl(dy * dy))) < radius`` in binary64
    (``closed``: ``<=``) and ``sums[i]`` the sum of the rows ``feats[j]`` (``[n, p]`` float64) over them in ascending row
    order, one add per row.  A row is taken by a select: a NaN or infinite feature reaches exactly the cells within the
    radius of its cell.  ``feats=None``: only the counts, ``sums`` is ``[n, 0]``.  ``xy`` [n, 2] float64 (a cell with NaN
    coordinates has count 0 and is nobody's neighbour), ``seg`` [F + 1] int64 offsets as for :func:`neighbor_counts`;
    the rows need no order inside a FOV."""
    def check_feats(n, dev):
        if feats is not None and (feats.dim() != 2 or feats.shape[0] != n or feats.dtype != torch.float64
                                  or feats.device != dev):
            raise ValueError("feats must be an [n, p] float64 HBM tensor on xy's device, or None")
    n, dev, seg, n_fovs = _cell_args(xy, seg, check_feats)
    _check_offsets(seg, n)
    p = 0 if feats is None else feats.shape[1]
    s_lim = radius_threshold(radius, closed)
    sums = torch.empty((n, p), dtype=torch.float64, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return sums, counts
    xy = xy.contiguous()
    feats = feats.contiguous() if p else None
    _capi.call("pxsom_neighborhood_sums", xy.data_ptr(), feats.data_ptr() if p else None, seg.data_ptr(), n_fovs, n, p,
               s_lim, sums.data_ptr() if p else None, counts.data_ptr(), _capi.stream_ptr())
    return sums, counts
