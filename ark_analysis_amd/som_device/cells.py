"""Cell tables: per-cell quantification (K12), regionprops (K17), splitting large nuclei (K21)."""
from typing import Optional

import numpy as np
import torch

from .. import _capi
from ._args import PAIR_CAPACITY_MAX, SEG_DTYPES, _key_range, _label_image, _ld, _rows_plane


# pxsom_cellquant (K12): image dtypes (PXSOM_SEG_* codes) and modes
CELLQUANT_IMAGE_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.uint16: 2, torch.int32: 3, torch.float64: 6,
                          torch.float32: 7}
CELLQUANT_MODES = {"total_intensity": 0, "positive_pixel": 1, "center_weighting": 2}
CELLQUANT_FORCE_SEARCH = 1
CELLQUANT_NUC_CAPACITY = 128


def label_keys(seg: torch.Tensor) -> torch.Tensor:
    """The sorted unique nonzero labels of an HBM label image as the int32 key table of :func:`cell_quantify`.
    Labels must be positive int32 values (NotImplementedError otherwise: negative labels and labels past int32 have no
    cell-table row the reference's int32 label column could name)."""
    wide = seg if seg.dtype in (torch.int32, torch.int64) else seg.to(
        torch.int64 if seg.dtype == torch.uint32 else torch.int32)
    keys = torch.unique(wide, sorted=True)
    if keys.numel():
        lo, hi = (int(v) for v in keys[[0, -1]].cpu())
        if lo < 0 or hi > 2147483647:
            raise NotImplementedError("cell table: labels must lie in 0 .. 2147483647, got %d .. %d" % (lo, hi))
        if lo == 0:
            keys = keys[1:]
    return keys.to(torch.int32)


def cell_quantify(seg: torch.Tensor, img: torch.Tensor, keys: Optional[torch.Tensor] = None,
                  mode: str = "total_intensity", threshold: float = 0.0, nuc: Optional[torch.Tensor] = None,
                  nuc_keys: Optional[torch.Tensor] = None, nuc_capacity: int = 0, force_search: bool = False) -> dict:
    """One pass of pxsom_cellquant: the per-cell table of a ``[H, W]`` label image (any row stride) over a contiguous
    ``[H, W, C]`` (or ``[H, W]``) HBM image.  ``keys`` (default :func:`label_keys` of ``seg``) name the cells, sorted
    ascending, unique and positive.  Returns a dict of HBM tensors: ``keys``, ``count`` [n] int64, ``sums`` [n, 2] int64
    (row, column), ``bbox`` [n, 4] int32 (row min, row max, column min, column max), ``values`` [n, C] float64 (``mode``
    total_intensity / positive_pixel with ``threshold``, compared in binary64 / center_weighting), and with a nuclear
    label image ``nuc``: ``nuc`` [n] int32, the index in ``nuc_keys`` (default :func:`label_keys` of ``nuc``, also
    returned as ``nuc_keys``) of the nucleus with the most pixels in the cell, the smaller on a tie, -1 for none.
    ``nuc_capacity`` bounds the per-cell overlap table (0: 128); ``force_search`` takes the binary-search route for
    both key tables."""
    h, w, ld = _label_image(seg, "seg")
    if img.dim() == 2:
        img = img.unsqueeze(-1)
    if img.dim() != 3 or tuple(img.shape[:2]) != (h, w) or not img.is_cuda or not img.is_contiguous() or \
            img.dtype not in CELLQUANT_IMAGE_DTYPES:
        raise ValueError("img must be a contiguous [H, W, C] uint8 / int16 / uint16 / int32 / float32 / float64 HBM "
                         "tensor of the segmentation's height and width")
    c = img.shape[2]
    if c == 0:
        raise ValueError("img must have at least one channel")
    if mode not in CELLQUANT_MODES:
        raise ValueError("mode must be one of %s" % sorted(CELLQUANT_MODES))
    if keys is None:
        keys = label_keys(seg)
    kmin, kmax = _key_range(keys)
    n = keys.numel()
    if n and kmin <= 0:
        raise ValueError("keys must be positive")
    dev = seg.device
    out = {"keys": keys,
           "count": torch.empty(n, dtype=torch.int64, device=dev),
           "sums": torch.empty((n, 2), dtype=torch.int64, device=dev),
           "bbox": torch.empty((n, 4), dtype=torch.int32, device=dev),
           "values": torch.empty((n, c), dtype=torch.float64, device=dev)}
    n_nuc, nmin, nmax, ldn, nuc_code = -1, 0, 0, w, 0
    if nuc is not None:
        if tuple(nuc.shape) != (h, w):
            raise ValueError("nuc must have the segmentation's shape")
        _, _, ldn = _label_image(nuc, "nuc")
        nuc_code = SEG_DTYPES[nuc.dtype]
        if nuc_keys is None:
            nuc_keys = label_keys(nuc)
        nmin, nmax = _key_range(nuc_keys)
        n_nuc = nuc_keys.numel()
        if n_nuc and nmin <= 0:
            raise ValueError("nuc_keys must be positive")
        out["nuc_keys"] = nuc_keys
        out["nuc"] = torch.empty(n, dtype=torch.int32, device=dev)
    if not 0 <= int(nuc_capacity) <= CELLQUANT_NUC_CAPACITY:
        raise ValueError("nuc_capacity must lie in 0 .. %d" % CELLQUANT_NUC_CAPACITY)
    flags = CELLQUANT_FORCE_SEARCH if force_search else 0
    img_code, mode_code = CELLQUANT_IMAGE_DTYPES[img.dtype], CELLQUANT_MODES[mode]
    lib = _capi.lib()
    wsb = lib.pxsom_cellquant_workspace_bytes(h, w, c, img_code, mode_code, n, kmin, kmax, n_nuc, nmin, nmax, flags)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _capi.call("pxsom_cellquant", seg.data_ptr(), SEG_DTYPES[seg.dtype], ld, nuc.data_ptr() if nuc is not None else None,
               nuc_code, ldn, h, w, img.data_ptr(), img_code, c, keys.data_ptr() if n else None, n, kmin,
               kmax, nuc_keys.data_ptr() if nuc is not None and n_nuc > 0 else None, n_nuc, nmin, nmax,
               mode_code, float(threshold), int(nuc_capacity), out["count"].data_ptr(),
               out["sums"].data_ptr(), out["bbox"].data_ptr(), out["values"].data_ptr(),
               out["nuc"].data_ptr() if nuc is not None else None, ws.data_ptr(), wsb, flags,
               _capi.stream_ptr())
    return out


# pxsom_region_shape / pxsom_region_hull (K17)
REGION_FORCE_SEARCH = 1
REGION_MAX_SIDE = 64           # the device route of the hull: bounding boxes up to 64 x 64
CONCAVITY_DEFAULTS = {"small_concavity_minimum": 10, "max_compactness": 60, "large_concavity_minimum": 150}


def region_props(seg: torch.Tensor, keys: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                 sums: Optional[torch.Tensor] = None, bbox: Optional[torch.Tensor] = None,
                 small_concavity_minimum: float = 10, max_compactness: float = 60,
                 large_concavity_minimum: float = 150, force_search: bool = False) -> dict:
    """The raw integers of the morphology regionprops of a ``[H, W]`` HBM label image (any row stride), one row per key
    (default :func:`label_keys` of ``seg``): a dict of HBM tensors ``keys``, ``count`` [n] int64, ``sums`` [n, 2] int64,
    ``bbox`` [n, 4] int32 (taken from the arguments when :func:`cell_quantify` already produced all three, computed in
    the same pass otherwise), ``shape`` [n, 6] int64 (sum r^2, sum c^2, sum r c, and the border pixels of perimeter
    weight 1, sqrt 2 and (1 + sqrt 2) / 2), ``hull`` [n, 4] int64 (convex area, convex row sum, convex column sum,
    concavities) and ``left_out`` [n] int32: 1 for a cell whose bounding box is past 64 x 64, whose ``hull`` row is 0 and
    is the host route's to fill (regionprops_extraction.host_hull)."""
    h, w, ld = _label_image(seg, "seg")
    if keys is None:
        keys = label_keys(seg)
    kmin, kmax = _key_range(keys)
    n = keys.numel()
    if n and kmin <= 0:
        raise ValueError("keys must be positive")
    given = [t is not None for t in (count, sums, bbox)]
    if any(given) and not all(given):
        raise ValueError("count, sums and bbox go together (all three from cell_quantify, or none)")
    dev = seg.device
    have = all(given)
    if have:
        ok = (count.dtype == torch.int64 and tuple(count.shape) == (n,) and sums.dtype == torch.int64 and
              tuple(sums.shape) == (n, 2) and bbox.dtype == torch.int32 and tuple(bbox.shape) == (n, 4))
        if not ok or not all(t.is_cuda and t.is_contiguous() for t in (count, sums, bbox)):
            raise ValueError("count [n] int64, sums [n, 2] int64 and bbox [n, 4] int32 must be contiguous HBM tensors")
    else:
        count = torch.empty(n, dtype=torch.int64, device=dev)
        sums = torch.empty((n, 2), dtype=torch.int64, device=dev)
        bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    for name, v in (("small_concavity_minimum", small_concavity_minimum), ("max_compactness", max_compactness),
                    ("large_concavity_minimum", large_concavity_minimum)):
        if float(v) != float(v):
            raise ValueError("%s must not be NaN" % name)
    out = {"keys": keys, "count": count, "sums": sums, "bbox": bbox,
           "shape": torch.empty((n, 6), dtype=torch.int64, device=dev),
           "hull": torch.empty((n, 4), dtype=torch.int64, device=dev),
           "left_out": torch.empty(n, dtype=torch.int32, device=dev)}
    flags = REGION_FORCE_SEARCH if force_search else 0
    lib = _capi.lib()
    wsb = lib.pxsom_region_shape_workspace_bytes(n, kmin, kmax, flags)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    code = SEG_DTYPES[seg.dtype]
    _capi.call("pxsom_region_shape", seg.data_ptr(), code, ld, h, w, keys.data_ptr() if n else None, n, kmin, kmax,
               out["shape"].data_ptr(), None if have else count.data_ptr(),
               None if have else sums.data_ptr(), None if have else bbox.data_ptr(), ws.data_ptr(),
               wsb, flags, _capi.stream_ptr())
    _capi.call("pxsom_region_hull", seg.data_ptr(), code, ld, h, w, keys.data_ptr() if n else None, n, count.data_ptr(),
               bbox.data_ptr(), float(small_concavity_minimum), float(max_compactness),
               float(large_concavity_minimum), out["hull"].data_ptr(), out["left_out"].data_ptr(),
               _capi.stream_ptr())
    return out


def _region_keys(seg: torch.Tensor, keys: Optional[torch.Tensor]):
    """``(h, w, ld, keys, n, key_min, key_max)`` of a label image and its key table (default :func:`label_keys`)."""
    h, w, ld = _label_image(seg, "seg")
    if keys is None:
        keys = label_keys(seg)
    kmin, kmax = _key_range(keys)
    n = keys.numel()
    if n and kmin <= 0:
        raise ValueError("keys must be positive")
    return h, w, ld, keys, n, kmin, kmax


def region_moments(seg: torch.Tensor, keys: Optional[torch.Tensor] = None, force_search: bool = False) -> dict:
    """:func:`region_props` without the hull launch, for objects of any size (pxsom_region_shape streams the image and
    has no bounding-box limit; only the hull kernel has one): a dict of HBM tensors ``keys``, ``count`` [n] int64,
    ``sums`` [n, 2] int64, ``bbox`` [n, 4] int32 and ``shape`` [n, 6] int64, as :func:`region_props` describes them."""
    # the key, workspace and pxsom_region_shape half of region_props, which stays as it was: keep the two in step
    h, w, ld, keys, n, kmin, kmax = _region_keys(seg, keys)
    dev = seg.device
    out = {"keys": keys,
           "count": torch.empty(n, dtype=torch.int64, device=dev),
           "sums": torch.empty((n, 2), dtype=torch.int64, device=dev),
           "bbox": torch.empty((n, 4), dtype=torch.int32, device=dev),
           "shape": torch.empty((n, 6), dtype=torch.int64, device=dev)}
    flags = REGION_FORCE_SEARCH if force_search else 0
    wsb = _capi.lib().pxsom_region_shape_workspace_bytes(n, kmin, kmax, flags)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    _capi.call("pxsom_region_shape", seg.data_ptr(), SEG_DTYPES[seg.dtype], ld, h, w, keys.data_ptr() if n else None, n,
               kmin, kmax, out["shape"].data_ptr(), out["count"].data_ptr(), out["sums"].data_ptr(),
               out["bbox"].data_ptr(), ws.data_ptr(), wsb, flags, _capi.stream_ptr())
    return out


def region_euler(seg: torch.Tensor, keys: Optional[torch.Tensor] = None, force_search: bool = False,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pxsom_region_euler: per key (default :func:`label_keys` of ``seg``) the Euler number of ``seg == key`` under
    8-connectivity -- objects minus holes, the plane padded by a zero border -- as an ``[n]`` int64 HBM vector (``out``
    when given).  ``seg`` as for :func:`region_props`; ``force_search`` takes the binary-search route of the key table."""
    h, w, ld, keys, n, kmin, kmax = _region_keys(seg, keys)
    dev = seg.device
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or tuple(out.shape) != (n,) or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous [n] int64 HBM vector")
    flags = REGION_FORCE_SEARCH if force_search else 0
    wsb = _capi.lib().pxsom_region_euler_workspace_bytes(n, kmin, kmax, flags)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    _capi.call("pxsom_region_euler", seg.data_ptr(), SEG_DTYPES[seg.dtype], ld, h, w, keys.data_ptr() if n else None, n,
               kmin, kmax, out.data_ptr(), ws.data_ptr(), wsb, flags, _capi.stream_ptr())
    return out


# pxsom_nuclear_overlaps / pxsom_split_apply (K21)
NUCSPLIT_FORCE_SEARCH = 1


def _split_planes(cell: torch.Tensor, nuc: torch.Tensor, cell_keys, nuc_keys):
    """The shared arguments of the two K21 entries: shape, strides, dtype codes, the key tables and their ranges."""
    h, w, ldc = _label_image(cell, "cell")
    if tuple(nuc.shape) != (h, w):
        raise ValueError("cell and nuc must have one shape, got %s and %s" % (tuple(cell.shape), tuple(nuc.shape)))
    _, _, ldn = _label_image(nuc, "nuc")
    if nuc.device != cell.device:
        raise ValueError("cell and nuc must be on one device")
    if cell_keys is None:
        cell_keys = label_keys(cell)
    if nuc_keys is None:
        nuc_keys = label_keys(nuc)
    (cmin, cmax), (nmin, nmax) = _key_range(cell_keys), _key_range(nuc_keys)
    if (cell_keys.numel() and cmin <= 0) or (nuc_keys.numel() and nmin <= 0):
        raise ValueError("cell_keys and nuc_keys must be positive")
    return h, w, ldc, ldn, cell_keys, nuc_keys, (cell_keys.numel(), cmin, cmax), (nuc_keys.numel(), nmin, nmax)


def nuclear_overlaps(cell: torch.Tensor, nuc: torch.Tensor, cell_keys: Optional[torch.Tensor] = None,
                     nuc_keys: Optional[torch.Tensor] = None, force_search: bool = False, capacity: Optional[int] = None):
    """One streaming pass of pxsom_nuclear_overlaps over two ``[H, W]`` HBM label planes (uint8 .. int64 each, any row
    stride).  ``cell_keys`` / ``nuc_keys`` (default :func:`label_keys` of each plane) name the cells and the nuclei,
    sorted ascending, unique and positive.  Returns HBM tensors ``(keys, nuc_keys, best, inside, area)``: per cell the
    index in ``nuc_keys`` of the nucleus with the most pixels inside it (the smaller label on a tie, -1: none) and that
    count, both int32 ``[n_cells]``; per nucleus its pixels in the whole plane, int64 ``[n_nuc]``.  Two calls: the first
    counts the runs of the image, which is read back and sizes the pair table of the second (``capacity`` overrides the
    size: a table too small gives RuntimeError and writes nothing)."""
    h, w, ldc, ldn, cell_keys, nuc_keys, ck, nk = _split_planes(cell, nuc, cell_keys, nuc_keys)
    dev = cell.device
    flags = NUCSPLIT_FORCE_SEARCH if force_search else 0
    lib = _capi.lib()
    n = torch.empty(2, dtype=torch.int32, device=dev)
    best = torch.empty((max(ck[0], 1), 2), dtype=torch.int32, device=dev)
    area = torch.empty(max(nk[0], 1), dtype=torch.int64, device=dev)

    def call(area_ptr, best_ptr, cap, ws, wsb):
        rc = lib.pxsom_nuclear_overlaps(cell.data_ptr(), SEG_DTYPES[cell.dtype], ldc, nuc.data_ptr(), SEG_DTYPES[nuc.dtype],
                                        ldn, h, w, cell_keys.data_ptr() if ck[0] else None, *ck,
                                        nuc_keys.data_ptr() if nk[0] else None, *nk, area_ptr, best_ptr, cap, n.data_ptr(),
                                        ws, wsb, flags, _capi.stream_ptr())
        _capi.check(rc, "pxsom_nuclear_overlaps")

    if capacity is None:
        call(None, None, 0, None, 0)
        capacity = max(int(n[1].item()), 1)
    capacity = int(capacity)
    if not 1 <= capacity <= PAIR_CAPACITY_MAX:
        raise NotImplementedError("nuclear_overlaps: %d runs of label pairs are beyond the limit %d" % (capacity, PAIR_CAPACITY_MAX))
    wsb = lib.pxsom_nuclear_overlaps_workspace_bytes(capacity, *ck, *nk, flags)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    call(area.data_ptr(), best.data_ptr(), capacity, ws.data_ptr(), wsb)
    if int(n[0].item()) < 0:
        raise RuntimeError("nuclear_overlaps: %d runs of label pairs do not fit the capacity %d" % (int(n[1].item()), capacity))
    best = best[:ck[0]]
    return cell_keys, nuc_keys, best[:, 0], best[:, 1], area[:nk[0]]


def choose_splits(keys, nuc_keys, best, inside, area, cell_ids, min_size=15, small=5, first_new=None, dtype=None):
    """The choice of split_large_nuclei on the host over the tables of :func:`nuclear_overlaps` (host arrays).  Every
    entry of ``cell_ids``, in the caller's order and duplicates included, whose cell has a nucleus with
    ``area - inside > min_size`` takes the next new label (from ``first_new``, default ``max(nuc_keys) + 1``); a cell
    named twice keeps its last number, the earlier one stays without pixels.  The sizes after the split come from the
    tables -- a new label has ``inside`` pixels, a split nucleus keeps ``area`` minus the ``inside`` of the distinct cells
    that split it -- and every label below ``small`` pixels becomes 0 (``remove_small_objects`` on an integer plane: no
    connected components).  Returns ``(chosen, cell_value, nuc_value, n_splits)``, the three tables of
    :func:`split_nuclei_apply`: ``chosen`` int32 [n_cells], ``cell_value`` int64 [n_cells] (-1: the cell splits nothing),
    ``nuc_value`` int64 [n_nuc].  IndexError names a ``cell_ids`` entry that is no key; with the plane's numpy ``dtype``
    given, ValueError names it when the last new label does not fit it (the reference's numpy scalar wraps there)."""
    keys = np.asarray(keys, dtype=np.int64)
    nuc_keys = np.asarray(nuc_keys, dtype=np.int64)
    best = np.asarray(best, dtype=np.int64)
    inside = np.asarray(inside, dtype=np.int64)
    area = np.asarray(area, dtype=np.int64)
    ids = np.asarray(cell_ids).reshape(-1)
    if ids.size and ids.dtype.kind not in "iu":
        raise TypeError("cell_ids must be integers, got %s" % ids.dtype)
    ids = ids.astype(np.int64)
    seq = np.searchsorted(keys, ids)
    miss = keys[np.minimum(seq, keys.size - 1)] != ids if keys.size else np.ones(ids.size, dtype=bool)
    if miss.any():
        raise IndexError("split_large_nuclei: cell id %d is no label of the cell segmentation" % int(ids[miss][0]))
    if first_new is None:
        first_new = (int(nuc_keys[-1]) if nuc_keys.size else 0) + 1
    has = best >= 0
    outside = np.zeros(keys.size, dtype=np.int64)
    outside[has] = area[best[has]] - inside[has]
    splits = has & (outside > min_size)                            # per cell: would it split its nucleus?
    flag = splits[seq]
    number = int(first_new) - 1 + np.cumsum(flag)                  # per entry of cell_ids
    n_splits = int(flag.sum())
    if dtype is not None and n_splits and int(first_new) - 1 + n_splits > np.iinfo(dtype).max:
        raise ValueError("split_large_nuclei: %d new labels from %d on do not fit the nuclear plane's dtype %s"
                         % (n_splits, int(first_new), np.dtype(dtype)))
    cell_value = np.full(keys.size, -1, dtype=np.int64)
    np.maximum.at(cell_value, seq[flag], number[flag])             # the numbers ascend: the last entry of a cell wins
    done = cell_value >= 0
    remaining = area.copy()
    np.subtract.at(remaining, best[done], inside[done])
    nuc_value = np.where(remaining < small, 0, nuc_keys)
    cell_value[done & (inside < small)] = 0
    return best.astype(np.int32), cell_value, nuc_value.astype(np.int64), n_splits


def split_nuclei_apply(cell: torch.Tensor, nuc: torch.Tensor, cell_keys: torch.Tensor, nuc_keys: torch.Tensor,
                       chosen: torch.Tensor, cell_value: torch.Tensor, nuc_value: torch.Tensor,
                       out: Optional[torch.Tensor] = None, force_search: bool = False) -> torch.Tensor:
    """The write pass of pxsom_split_apply: ``out`` (the nuclear plane's dtype, any row stride, default a new plane) takes
    ``cell_value[c]`` where the pixel's cell ``c`` chose the pixel's nucleus (``chosen[c]``) and ``cell_value[c] >= 0``,
    else ``nuc_value[j]`` of its nucleus ``j``; a nuclear label outside ``nuc_keys`` is copied through."""
    h, w, ldc, ldn, cell_keys, nuc_keys, ck, nk = _split_planes(cell, nuc, cell_keys, nuc_keys)
    dev = cell.device
    for name, t, dtype, n in (("chosen", chosen, torch.int32, ck[0]), ("cell_value", cell_value, torch.int64, ck[0]),
                              ("nuc_value", nuc_value, torch.int64, nk[0])):
        if t.dtype != dtype or not t.is_cuda or t.dim() != 1 or not t.is_contiguous() or t.numel() != n:
            raise ValueError("%s must be a contiguous %s HBM vector of %d entries" % (name, str(dtype).replace("torch.", ""), n))
    out = _rows_plane(out, h, w, nuc.dtype, dev, "out")
    flags = NUCSPLIT_FORCE_SEARCH if force_search else 0
    lib = _capi.lib()
    wsb = lib.pxsom_split_apply_workspace_bytes(*ck, *nk, flags)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    _capi.call("pxsom_split_apply", cell.data_ptr(), SEG_DTYPES[cell.dtype], ldc, nuc.data_ptr(), SEG_DTYPES[nuc.dtype], ldn, h, w,
               cell_keys.data_ptr() if ck[0] else None, *ck, nuc_keys.data_ptr() if nk[0] else None, *nk,
               chosen.data_ptr() if ck[0] else None, cell_value.data_ptr() if ck[0] else None,
               nuc_value.data_ptr() if nk[0] else None, out.data_ptr(), _ld(out), ws.data_ptr(), wsb, flags,
               _capi.stream_ptr())
    return out


def split_large_nuclei(cell: torch.Tensor, nuc: torch.Tensor, cell_ids=None, min_size=15, small=5,
                       out: Optional[torch.Tensor] = None, force_search: bool = False) -> torch.Tensor:
    """The device chain of ``segmentation_utils.split_large_nuclei`` on two ``[H, W]`` HBM label planes -> the modified
    nuclear plane in HBM, in the nuclear plane's dtype.  For every id of ``cell_ids`` (default: every cell label
    ascending), in that order: the nucleus with the most pixels inside the cell (the smallest label on a tie) is
    renumbered inside the cell when more than ``min_size`` of its pixels lie outside it; then every label below ``small``
    pixels is removed.  Only the per-cell and per-nucleus tables are read back for the choice (:func:`choose_splits`);
    the planes stay in HBM.  ValueError when the new labels do not fit the nuclear plane's dtype (the reference's numpy
    scalar wraps there), raised before the write pass."""
    keys, nuc_keys, best, inside, area = nuclear_overlaps(cell, nuc, force_search=force_search)
    keys_h = keys.cpu().numpy()
    if cell_ids is None:
        cell_ids = keys_h
    chosen, cell_value, nuc_value, _ = choose_splits(keys_h, nuc_keys.cpu().numpy(), best.cpu().numpy(), inside.cpu().numpy(),
                                                     area.cpu().numpy(), cell_ids, min_size, small,
                                                     dtype=np.dtype(str(nuc.dtype).replace("torch.", "")))
    dev = cell.device
    return split_nuclei_apply(cell, nuc, keys, nuc_keys, torch.from_numpy(chosen).to(dev), torch.from_numpy(cell_value).to(dev),
                              torch.from_numpy(nuc_value).to(dev), out=out, force_search=force_search)
