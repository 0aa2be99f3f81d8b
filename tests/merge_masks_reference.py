"""The numpy + scipy statement of the K18 contracts (include/pxsom.h "merging ez_seg object masks"): labelling regions
of equal value, the pair list, the choice of merge_masks_single as literal loops, and the write.  The CPU tests check it
against the g22 fixtures (made by the reference's own ``merge_masks_single``); the GPU tests compare the device entries
with it exactly."""
import numpy as np
import scipy.ndimage as ndi


def label_regions(seg, connectivity):
    """(labels int32, n, areas int64 [n + 1]): per distinct non-zero value scipy's components, then all components
    renumbered by their first pixel in raster order."""
    seg = np.asarray(seg)
    structure = ndi.generate_binary_structure(2, connectivity)
    flat = np.zeros(seg.shape, dtype=np.int64)
    total = 0
    for value in np.unique(seg[seg != 0]):
        part, n = ndi.label(seg == value, structure=structure)
        flat[part != 0] = part[part != 0] + total
        total += n
    labels = np.zeros(seg.shape, dtype=np.int32)
    if total:
        _, first = np.unique(flat.ravel(), return_index=True)       # first raster index of 0 (if any), 1, 2, ...
        first = first[1:] if (flat == 0).any() else first
        rank = np.empty(total + 1, dtype=np.int64)
        rank[0] = 0
        rank[1 + np.argsort(first)] = np.arange(1, total + 1)
        labels = rank[flat].astype(np.int32)
    return labels, int(total), np.bincount(labels.ravel(), minlength=total + 1)


def pair_overlaps(a, b, n_a=None, n_b=None):
    """[P, 3] int32 rows (a, b, pixels) of the pairs with 1 <= a <= n_a and 1 <= b <= n_b, sorted by (a, b)."""
    a, b = np.asarray(a).astype(np.int64).ravel(), np.asarray(b).astype(np.int64).ravel()
    n_a, n_b = (2 ** 31 - 1 if v is None else v for v in (n_a, n_b))
    keep = (a >= 1) & (a <= n_a) & (b >= 1) & (b <= n_b)
    keys, counts = np.unique(a[keep] * 2 ** 32 + b[keep], return_counts=True)
    return np.stack([keys >> 32, keys & (2 ** 32 - 1), counts], axis=1).astype(np.int32).reshape(-1, 3)


def region_tables(labels, n):
    """count [n], coordinate sums [n, 2] and closed boxes [n, 4] (row min, row max, column min, column max) of 1 .. n."""
    rows, cols = np.nonzero(labels)
    lab = labels[rows, cols].astype(np.int64) - 1
    count = np.bincount(lab, minlength=n)
    sums = np.stack([np.bincount(lab, weights=rows, minlength=n), np.bincount(lab, weights=cols, minlength=n)], axis=1)
    big = max(labels.shape)
    box = np.stack([np.full(n, big), np.full(n, -1), np.full(n, big), np.full(n, -1)], axis=1).astype(np.int64)
    np.minimum.at(box[:, 0], lab, rows)
    np.maximum.at(box[:, 1], lab, rows)
    np.minimum.at(box[:, 2], lab, cols)
    np.maximum.at(box[:, 3], lab, cols)
    return count, sums.astype(np.int64), box


def merge_masks(object_mask, cell_mask, overlap_thresh, expansion_factor, compare=None):
    """(merged, remaining) int32.  ``compare``: the two compares of the choice (for the tests that show a test case
    tells ``>`` from ``>=``); default the contract's strict ones."""
    object_mask, cell_mask = np.asarray(object_mask), np.asarray(cell_mask)
    if object_mask.shape != cell_mask.shape:
        raise ValueError("Both masks must have the same shape")
    better, over = compare or ((lambda x, y: x > y), (lambda x, y: x > y))
    objects, n_o, _ = label_regions(object_mask, 2)
    cells, n_c, areas = label_regions(cell_mask, 2)
    _, _, boxes = region_tables(objects, n_o)
    count, sums, _ = region_tables(cells, n_c)
    overlap = np.zeros((n_o + 1, n_c + 1), dtype=np.int64)
    for a, b, c in pair_overlaps(objects, cells):
        overlap[a, b] = c
    merged = objects.copy()
    removed = [0]
    for obj in range(1, n_o + 1):
        r0, r1, c0, c1 = boxes[obj - 1]
        best, chosen = 0, None
        for cell in range(1, n_c + 1):
            cy, cx = np.float64(sums[cell - 1, 0]) / np.float64(count[cell - 1]), np.float64(sums[cell - 1, 1]) / np.float64(count[cell - 1])
            if not (cy >= r0 - expansion_factor and cy <= r1 + expansion_factor and cx >= c0 - expansion_factor and
                    cx <= c1 + expansion_factor):
                continue
            ov = overlap[obj, cell]
            if better(ov, best) and over(ov / areas[cell], overlap_thresh / 100):
                best, chosen = ov, cell
        if chosen is not None:
            merged[cells == chosen] = obj
            removed.append(chosen)
    remaining = np.where(np.isin(cells, removed), 0, cells)
    return merged.astype(np.int32), remaining.astype(np.int32)


def disc(shape, centre, r2):
    """(r - r0)^2 + (c - c0)^2 < r2 as a bool image."""
    rr, cc = np.mgrid[:shape[0], :shape[1]]
    return (rr - centre[0]) ** 2 + (cc - centre[1]) ** 2 < r2


def random_masks(rs, h, w, n_cells, n_objects, cell_r=(2, 5), object_r=(3, 8)):
    """A cell mask of numbered discs (later ones paint over earlier ones: touching cells of different value, cells cut
    in pieces) and an object mask of fewer, larger numbered discs."""
    cells = np.zeros((h, w), dtype=np.int32)
    for i in range(n_cells):
        cells[disc((h, w), (rs.randint(h), rs.randint(w)), rs.randint(cell_r[0], cell_r[1] + 1) ** 2)] = rs.randint(1, n_cells + 1)
    objects = np.zeros((h, w), dtype=np.int32)
    for i in range(n_objects):
        objects[disc((h, w), (rs.randint(h), rs.randint(w)), rs.randint(object_r[0], object_r[1] + 1) ** 2)] = i + 1
    return objects, cells


def random_masks_windowed(rs, h, w, n_cells, n_objects, cell_r=(2, 5), object_r=(3, 8)):
    """:func:`random_masks`, draw for draw, with every disc painted inside its bounding window only: the cost of a disc
    no longer grows with the image (the field-size tests)."""
    def paint(plane, value, radii):
        cy, cx, r = rs.randint(h), rs.randint(w), rs.randint(radii[0], radii[1] + 1)
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, h), max(cx - r, 0), min(cx + r + 1, w)
        rr, cc = np.mgrid[y0:y1, x0:x1]
        plane[y0:y1, x0:x1][(rr - cy) ** 2 + (cc - cx) ** 2 < r ** 2] = value

    cells = np.zeros((h, w), dtype=np.int32)
    for i in range(n_cells):
        paint(cells, rs.randint(1, n_cells + 1), cell_r)        # (the value is drawn before the disc, as an assignment does)
    objects = np.zeros((h, w), dtype=np.int32)
    for i in range(n_objects):
        paint(objects, i + 1, object_r)
    return objects, cells
