"""Plain numpy statement of pxsom_segmask's contract (include/pxsom.h, "cell cluster masks"): border erosion as
skimage.segmentation.find_boundaries defines it (dilation != erosion under scipy's reflect border), the int32 wrap of
the label, the table lookup with a default, and numpy's casts into the output dtype.  Test infrastructure: the GPU tests
compare the device with it, array_equal, and the CPU tests pin it to the g15 fixtures of the reference."""
import numpy as np

_OFFSETS4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
_OFFSETS8 = _OFFSETS4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def boundaries(seg, connectivity=1, mode="thick", background=0):
    """find_boundaries(seg, connectivity, mode) of a 2-D label image: a pixel whose 4- (connectivity 1) or
    8-neighbourhood (>= 2) holds another label, compared in the image's dtype.  A neighbour outside the image reflects
    back into it ('edge' padding at distance 1), which never adds a label.  "inner" also needs seg != background."""
    if mode not in ("thick", "inner"):
        raise NotImplementedError(mode)
    seg = np.asarray(seg)
    h, w = seg.shape
    pad = np.pad(seg, 1, mode="edge")
    edge = np.zeros(seg.shape, dtype=bool)
    for dy, dx in (_OFFSETS8 if connectivity >= 2 else _OFFSETS4):
        edge |= pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != seg
    if mode == "inner":
        edge &= seg.astype(np.int64) != background
    return edge


def erode(seg, connectivity=1, mode="thick", background=0):
    """erode_mask: boundary pixels -> 0, in the image's own dtype."""
    seg = np.asarray(seg)
    return np.where(boundaries(seg, connectivity, mode, background), seg.dtype.type(0), seg)


def segmask(seg, erode_mode=None, connectivity=1, background=0, keys=None, values=None, unassigned=0, out_dtype=None):
    """The whole pass: optional erosion, then (with ``keys``) value of the int32-wrapped label in the sorted table or
    ``unassigned`` (values int32, or float64 for a float64 output), cast to ``out_dtype`` (default: the image's)."""
    seg = np.asarray(seg)
    out_dtype = np.dtype(out_dtype or seg.dtype)
    lab = seg if erode_mode is None else erode(seg, connectivity, erode_mode, background)
    if keys is None:
        return lab.astype(out_dtype)
    vdt = np.float64 if out_dtype == np.float64 else np.int32
    keys = np.asarray(keys, dtype=np.int32)
    values = np.asarray(values, dtype=vdt)
    k32 = lab.astype(np.int32)
    res = np.full(lab.shape, unassigned, dtype=vdt)
    if keys.size:
        idx = np.minimum(np.searchsorted(keys, k32), keys.size - 1)
        found = keys[idx] == k32
        res[found] = values[idx[found]]
    return res.astype(out_dtype)


def table_from_mapping(mapping):
    """A {label: value} dict as the sorted (keys, values) the library takes; keys wrap to int32, a later key wins."""
    keys = np.asarray(list(mapping.keys()), dtype=np.int64).astype(np.int32)
    values = np.asarray(list(mapping.values()))
    if keys.size == 0:
        return keys, values
    rev_keys, rev_first = np.unique(keys[::-1], return_index=True)
    return rev_keys, values[::-1][rev_first]


def voronoi_labels(h, w, n_cells, seed, dtype=np.int32, max_label=None):
    """A Voronoi-like whole-cell segmentation: every pixel takes the sparse label of its nearest of ``n_cells`` random
    seeds, and pixels nearly equidistant from two seeds are background 0 (the gaps between cells)."""
    from scipy.spatial import cKDTree
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.uniform(0, h, n_cells), rs.uniform(0, w, n_cells)], 1)
    labels = rs.choice(np.arange(1, (max_label or 3 * n_cells) + 1), size=n_cells, replace=False).astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    d, i = cKDTree(pts).query(np.stack([yy.ravel(), xx.ravel()], 1), k=2)
    out = labels[i[:, 0]]
    out[d[:, 1] - d[:, 0] < 0.7] = 0
    return out.reshape(h, w).astype(dtype)
