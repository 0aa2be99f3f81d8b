"""The numpy statement of pxsom_nearest_type_means, as the reference writes it: per FOV
``cdist(c, c).astype(float32)``; per phenotype the columns of its cells, ``where(> 0)`` (zeros become NaN), ``np.sort`` of
every row (NaN last), ``[:, :k].mean(axis=1)``; a list of NaN when the phenotype has fewer than k columns
(ark/analysis/spatial_analysis_utils.py calc_dist_matrix + ark/analysis/cell_neighborhood_stats.py
calculate_mean_distance_to_cell_type).  The matrix is built a block of query rows at a time (every entry is one pair's
own value and every mean one row's own, so the blocks change nothing), which keeps 5 000-cell FOVs within a test's memory.

The slice of one phenotype's columns is made row-major before the sort.  That decides the order of the float32 sum:
``mean(axis=1)`` of a row-major [N, k] slice is numpy's pairwise sum of each row (what DESIGN.md K14 and the kernel state,
and what the g19 fixture holds), whereas numpy reduces the column-major array that ``dist[:, cols]`` returns as a plain
left-to-right fold, which differs in the last bits from k = 8 on.

Also ``row_sum_order``: numpy's order for a float32 row reduction written out term by term, which is the order the kernel
adds in."""
import numpy as np
from scipy.spatial.distance import cdist

ROW_BLOCK = 1024


def nearest_type_means_for(xy, types, seg, n_types, ks):
    """``{k: [n, n_types] float32}``: for cell i, per type, the mean of the k smallest non-zero float32 distances to the
    cells of that type in its FOV; NaN when fewer than k are non-zero.  ``seg`` [F + 1] offsets into the rows.  The
    matrix and its sorted slices are built once for all of ``ks``."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    types = np.asarray(types)
    out = {k: np.full((xy.shape[0], n_types), np.nan, dtype=np.float32) for k in ks}
    for a, b in zip(seg[:-1], seg[1:]):
        a, b = int(a), int(b)
        if b == a:
            continue
        pts = xy[a:b]
        members = [np.flatnonzero(types[a:b] == t) for t in range(n_types)]
        for r in range(0, b - a, ROW_BLOCK):
            dist = cdist(pts[r:r + ROW_BLOCK], pts).astype(np.float32)
            for t, cols in enumerate(members):
                if len(cols) < min(ks):
                    continue
                d = np.ascontiguousarray(dist[:, cols])      # row-major, as the fixture's DataArray stand-in selects
                d = np.sort(np.where(d > 0, d, np.float32(np.nan)), axis=1)
                for k in ks:
                    if len(cols) >= k:
                        out[k][a + r:a + r + len(d), t] = d[:, :k].mean(axis=1)
    return out


def nearest_type_means(xy, types, seg, n_types, k):
    """The [n, n_types] float32 means for one k."""
    return nearest_type_means_for(xy, types, seg, n_types, [k])[k]


def host_stand_in(xy, types, seg, n_types, k):
    """The signature of ark_analysis_amd.analysis.cell_neighborhood_stats._nearest_type_means_device."""
    return nearest_type_means(xy, types, seg, n_types, k)


def _pairwise(a):
    """numpy's pairwise sum of the float32 vector ``a`` (numpy/_core/src/umath/loops_utils.h.src), one float32 addition per
    statement."""
    n = len(a)
    if n < 8:
        res = np.float32(0)
        for v in a:
            res = np.float32(res + v)
        return res
    if n <= 128:
        r = [np.float32(v) for v in a[:8]]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = np.float32(r[j] + a[i + j])
            i += 8
        res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))
                         + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        for v in a[i:]:
            res = np.float32(res + v)
        return res
    half = n // 2
    half -= half % 8
    return np.float32(_pairwise(a[:half]) + _pairwise(a[half:]))


def row_sum_order(row):
    """float32 mean of one row in numpy's order: 0 + pairwise(row), divided by float32(len)."""
    row = np.asarray(row, dtype=np.float32)
    return np.float32(np.float32(np.float32(0) + _pairwise(row)) / np.float32(len(row)))
