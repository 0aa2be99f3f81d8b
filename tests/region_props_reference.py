"""Independent numpy / scipy statement of the morphology contract, per cell on its bounding-box crop:
float central moments and ``np.linalg.eigvalsh`` for the inertia tensor (and, for the minor axis alone, the smaller root
of its characteristic polynomial from exact integer moments at 120 digits: eigvalsh resolves l2 only to eps * l1, which
says nothing about a thin cell's minor axis at relative 1e-12); ``ndimage.binary_erosion``,
``ndimage.convolve`` and ``bincount`` for skimage.measure.perimeter's codes; ``scipy.spatial.ConvexHull`` (Qhull, not
a monotone chain) of the diamond points with an exact integer half-plane test on its vertices for the convex image;
``ndimage.label`` for the concavities.  A cell is every pixel of one label; other labels are background for it.

:func:`reference` returns the raw integers the device returns and the float columns the host derives from them;
:func:`compare` holds the tolerances, which are derived (both sides are a handful of binary64 operations on exact
integers), not measured."""
import decimal

import numpy as np
from scipy import ndimage
from scipy.spatial import ConvexHull

SQRT2 = np.sqrt(2.0)
WEIGHTS = np.zeros(50)
WEIGHTS[[5, 7, 15, 17, 25, 27]] = 1
WEIGHTS[[21, 33]] = SQRT2
WEIGHTS[[13, 23]] = (1 + SQRT2) / 2
CLASS = np.zeros(50, dtype=np.int64)
CLASS[[5, 7, 15, 17, 25, 27]] = 1
CLASS[[21, 33]] = 2
CLASS[[13, 23]] = 3
DEFAULTS = dict(small_concavity_minimum=10, max_compactness=60, large_concavity_minimum=150)


def perimeter_classes(mask):
    """(n1, n2, n3) as skimage.measure.perimeter(neighbourhood=4) histograms them."""
    mask = np.asarray(mask, dtype=bool)
    eroded = ndimage.binary_erosion(mask, ndimage.generate_binary_structure(2, 1), border_value=0)
    border = (mask & ~eroded).astype(np.int64)
    codes = ndimage.convolve(border, np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode="constant", cval=0)
    hist = np.bincount(codes.ravel(), minlength=50)
    return tuple(int(hist[CLASS == c].sum()) for c in (1, 2, 3))


def perimeter_value(n1, n2, n3):
    return n1 + n2 * SQRT2 + n3 * ((1 + SQRT2) / 2)


def convex_image(mask):
    """Centres inside or on the Qhull hull of the diamond points, decided in doubled integers."""
    mask = np.asarray(mask, dtype=bool)
    rr, cc = np.nonzero(mask)
    pts = np.concatenate([np.stack([2 * rr + dr, 2 * cc + dc], axis=1)
                          for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1))]).astype(np.int64)
    pts = np.unique(pts, axis=0)
    hull = ConvexHull(pts.astype(np.float64))
    v = pts[hull.vertices]                      # counter-clockwise in (first, second) coordinates
    gr, gc = np.mgrid[0:mask.shape[0], 0:mask.shape[1]]
    pr, pc = 2 * gr.astype(np.int64), 2 * gc.astype(np.int64)
    inside = np.ones(mask.shape, dtype=bool)
    for i in range(len(v)):
        (ar, ac), (br, bc) = v[i], v[(i + 1) % len(v)]
        inside &= (br - ar) * (pc - ac) - (bc - ac) * (pr - ar) >= 0
    return inside


def exact_minor_axis(lr, lc):
    """4 sqrt(l2) of the pixels (lr, lc) (int64, small offsets from the box origin), rounded once to binary64: with
    M20 = sum (n r - sum r)^2, M02 and M11 alike (integers, n^2 times the central moments), l2 is
    (M20 + M02 - sqrt((M20 - M02)^2 + 4 M11^2)) / (2 n^3) -- the textbook root, cancellation and all, at 120 digits,
    where it costs at most the ~50 digits that the largest integers here hold.  Exactly 0 for collinear pixels."""
    n = int(lr.size)
    dr, dc = n * lr - lr.sum(), n * lc - lc.sum()
    if n * max(int(lr.max()), int(lc.max()), 1) >= 2 ** 20:      # the squares' sum could pass int64
        dr, dc = dr.astype(object), dc.astype(object)
    m20, m02, m11 = int((dr * dr).sum()), int((dc * dc).sum()), int((dr * dc).sum())
    if m20 * m02 == m11 * m11:
        return 0.0
    with decimal.localcontext() as ctx:
        ctx.prec = 120
        root = decimal.Decimal((m20 - m02) ** 2 + 4 * m11 * m11).sqrt()
        l2 = (decimal.Decimal(m20 + m02) - root) / (2 * n ** 3)
        assert l2 > 0
        return float(4 * l2.sqrt())


class MarginError(AssertionError):
    """A concavity of the image sits on one of num_concavities' thresholds: the generator has to draw another image."""


def concavities(diff, small_concavity_minimum=10, max_compactness=60, large_concavity_minimum=150):
    """(count, margin ok): the components of ``diff`` that count; asserts that none sits on a threshold, so a flipped
    comparison cannot hide behind an ulp."""
    lab, n = ndimage.label(diff)
    total = 0
    for i, box in enumerate(ndimage.find_objects(lab), start=1):
        comp = lab[box] == i
        a = int(comp.sum())
        p = perimeter_value(*perimeter_classes(comp))
        if a == small_concavity_minimum or a == large_concavity_minimum:
            raise MarginError("a concavity's area sits on a threshold")
        if abs(p * p / a - max_compactness) < 1e-9:
            raise MarginError("a concavity's compactness sits on the threshold")
        if (a > small_concavity_minimum and p * p / a < max_compactness) or a > large_concavity_minimum:
            total += 1
    return total


def reference(seg, drop=False, **thresholds):
    """Per cell (labels ascending): the raw integers of som_device.region_props and the float columns.  A concavity on
    a threshold raises MarginError; with ``drop`` such a cell is cleared instead (cells do not see each other, so the
    rest is unchanged; at most one cell in twenty, asserted) and the result is (the cleared image, its reference)."""
    seg = np.asarray(seg)
    dropped = []
    thr = dict(DEFAULTS, **thresholds)
    keys = np.unique(seg)
    keys = keys[keys != 0].astype(np.int64)
    n = keys.size
    out = {"keys": keys, "count": np.zeros(n, np.int64), "sums": np.zeros((n, 2), np.int64),
           "bbox": np.zeros((n, 4), np.int64), "shape": np.zeros((n, 6), np.int64), "hull": np.zeros((n, 4), np.int64),
           "eigenvalues": np.zeros((n, 2)), "major_axis_length": np.zeros(n), "minor_axis_length": np.zeros(n),
           "eccentricity": np.zeros(n), "one_minus_ecc2": np.zeros(n), "equivalent_diameter": np.zeros(n),
           "perimeter": np.zeros(n), "major_minor_axis_ratio": np.zeros(n), "perim_square_over_area": np.zeros(n),
           "major_axis_equiv_diam_ratio": np.zeros(n), "convex_hull_resid": np.zeros(n), "centroid_dif": np.zeros(n)}
    dense = np.searchsorted(keys, seg.astype(np.int64)) + 1
    dense[seg == 0] = 0
    boxes = ndimage.find_objects(dense, max_label=n) if n else []
    for i, key in enumerate(keys):
        r0, r1, c0, c1 = boxes[i][0].start, boxes[i][0].stop - 1, boxes[i][1].start, boxes[i][1].stop - 1
        mask = seg[r0:r1 + 1, c0:c1 + 1] == key
        rows, cols = np.nonzero(mask)
        rr, cc = rows.astype(np.int64) + r0, cols.astype(np.int64) + c0
        area = rr.size
        out["count"][i] = area
        out["sums"][i] = (rr.sum(), cc.sum())
        out["bbox"][i] = (r0, r1, c0, c1)
        per = perimeter_classes(mask)
        out["shape"][i] = ((rr * rr).sum(), (cc * cc).sum(), (rr * cc).sum()) + per
        conv = convex_image(mask)
        assert conv[mask].all()
        cr, ccol = np.nonzero(conv)
        try:
            n_conc = concavities(conv & ~mask, **thr)
        except MarginError:
            if not drop:
                raise
            dropped.append(i)
            continue
        out["hull"][i] = (cr.size, (cr + r0).sum(), (ccol + c0).sum(), n_conc)
        # floats
        lr, lc = (rr - r0).astype(np.float64), (cc - c0).astype(np.float64)
        dr, dc = lr - lr.mean(), lc - lc.mean()
        mu20, mu02, mu11 = (dr * dr).sum(), (dc * dc).sum(), (dr * dc).sum()
        tensor = np.array([[mu02, -mu11], [-mu11, mu20]]) / area
        l2, l1 = np.clip(np.linalg.eigvalsh(tensor), 0, None)
        out["eigenvalues"][i] = (l1, l2)
        major, minor = 4 * np.sqrt(l1), exact_minor_axis(rr - r0, cc - c0)
        out["major_axis_length"][i], out["minor_axis_length"][i] = major, minor
        out["one_minus_ecc2"][i] = l2 / l1 if l1 > 0 else 1.0
        out["eccentricity"][i] = np.sqrt(1 - l2 / l1) if l1 > 0 else 0.0
        equiv = np.sqrt(4 * area / np.pi)
        out["equivalent_diameter"][i] = equiv
        p = perimeter_value(*per)
        out["perimeter"][i] = p
        out["major_minor_axis_ratio"][i] = major / minor if minor != 0 else np.nan
        out["perim_square_over_area"][i] = p * p / area
        out["major_axis_equiv_diam_ratio"][i] = major / equiv
        out["convex_hull_resid"][i] = (cr.size - area) / cr.size
        out["centroid_dif"][i] = np.hypot(lr.mean() - cr.mean(), lc.mean() - ccol.mean()) / np.sqrt(area)
    if drop:
        # clearing is for the odd cell: a generator that loses more than one cell in twenty no longer gives the image
        # its test describes (a lone drop is allowed in the smallest images)
        assert len(dropped) <= max(1, n // 20), "%d of %d cells have a concavity on a threshold" % (len(dropped), n)
        keep = np.setdiff1d(np.arange(n), dropped)
        return np.where(np.isin(seg, keys[dropped]), 0, seg).astype(seg.dtype), {k: v[keep] for k, v in out.items()}
    return out


def compare(raw, cols, ref):
    """``raw`` (the raw integers under test, host arrays) equal to the reference's; ``cols`` (the float columns derived
    from them, regionprops_extraction.morphology) within the derived tolerances."""
    for name in ("keys", "count", "sums", "bbox", "shape", "hull"):
        np.testing.assert_array_equal(np.asarray(raw[name]).astype(np.int64).reshape(ref[name].shape), ref[name],
                                      err_msg=name)
    if "left_out" in raw:
        assert not np.asarray(raw["left_out"]).any()
    l1 = ref["eigenvalues"][:, 0]
    assert np.all(np.abs(cols["eigenvalues"] - ref["eigenvalues"]) <= 1e-12 * l1[:, None]), "eigenvalues"
    for name in ("major_axis_length", "equivalent_diameter"):
        assert np.all(np.abs(cols[name] - ref[name]) <= 1e-12 * np.abs(ref[name])), name
    # minor_axis_length at relative 1e-12 for every cell, against the exact root (exact_minor_axis): eigvalsh's l2 is good
    # to eps * l1 only -- enough for the eigenvalue bound above, not for the length of a thin cell.  A cell whose
    # pixels are collinear (the determinant of the integer second moments is 0) has no minor axis: exactly 0.
    minor, want = cols["minor_axis_length"], ref["minor_axis_length"]
    assert np.all(np.abs(minor - want) <= 1e-12 * np.abs(want)), "minor_axis_length"
    n, (sr, sc) = ref["count"].astype(object), ref["sums"].astype(object).T
    srr, scc, src = ref["shape"][:, :3].astype(object).T
    collinear = np.array((n * srr - sr * sr) * (n * scc - sc * sc) - (n * src - sr * sc) ** 2 == 0, dtype=bool)
    np.testing.assert_array_equal(want == 0, collinear)
    assert np.all(minor[collinear] == 0), "minor_axis_length (collinear pixels)"
    # eccentricity as 1 - ecc^2 against l2 / l1: comparing eccentricity itself near a circle turns eps into sqrt(eps)
    assert np.all(np.abs((1 - cols["eccentricity"] ** 2) - ref["one_minus_ecc2"]) <= 1e-12), "eccentricity"
    for name in ("perimeter", "perim_square_over_area"):
        assert np.all(np.abs(cols[name] - ref[name]) <= 1e-13 * np.abs(ref[name])), name
    assert np.all(np.abs(cols["centroid_dif"] - ref["centroid_dif"]) <= 1e-12), "centroid_dif"
    for name in ("major_axis_equiv_diam_ratio", "convex_hull_resid"):
        assert np.all(np.abs(cols[name] - ref[name]) <= 1e-12 * np.abs(ref[name])), name
    ratio, want = cols["major_minor_axis_ratio"], ref["major_minor_axis_ratio"]
    np.testing.assert_array_equal(np.isnan(ratio), collinear)
    ok = ~collinear                   # a quotient of two lengths, each within 1e-12, and one rounding
    assert np.all(np.abs(ratio[ok] - want[ok]) <= 3e-12 * np.abs(want[ok])), "major_minor_axis_ratio"
    np.testing.assert_array_equal(cols["area"], ref["count"])
    np.testing.assert_array_equal(cols["convex_area"], ref["hull"][:, 0])
    np.testing.assert_array_equal(cols["num_concavities"], ref["hull"][:, 3])


def settled(make, seed, **thresholds):
    """(image, its reference) of ``make(seed)`` with every cell that has a concavity on a threshold cleared: a generator
    must not hand out an image without the margin the reference asserts."""
    return reference(make(seed), drop=True, **thresholds)


def voronoi(h, w, n_cells, seed=0, background=0.1, dtype=np.int32, first_label=1):
    """Per-pixel Voronoi cells of ``n_cells`` random sites (no coarse grid: concavity areas take every value, so a
    redraw clears a threshold hit); a fraction ``background`` of the cells is 0.  Labels shuffled from first_label."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    sites = np.stack([rng.uniform(0, h, n_cells), rng.uniform(0, w, n_cells)], axis=1)
    gy, gx = np.mgrid[0:h, 0:w]
    _, near = cKDTree(sites).query(np.stack([gy.ravel() + 0.5, gx.ravel() + 0.5], axis=1))
    labels = rng.permutation(n_cells).astype(np.int64) + first_label
    labels[rng.random(n_cells) < background] = 0
    return labels[near].reshape(h, w).astype(dtype)


# ---- shapes with answers counted by hand -------------------------------------------------------------------------
def ring(outer, inner):
    """A square ring: an ``outer`` x ``outer`` block with a centred ``inner`` x ``inner`` hole."""
    m = np.ones((outer, outer), dtype=bool)
    o = (outer - inner) // 2
    m[o:o + inner, o:o + inner] = False
    return m


def c_shape(outer, inner):
    """A C: the ring with its hole opened to the right edge."""
    m = ring(outer, inner)
    o = (outer - inner) // 2
    m[o:o + inner, o:] = False
    return m
