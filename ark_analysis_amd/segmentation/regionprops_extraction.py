"""The morphology columns of ``generate_cell_table(fast_extraction=False)`` (the reference's
ark/segmentation/regionprops_extraction.py and the skimage regionprops get_single_compartment_props asks for): the host
side of DESIGN.md K17.

The device (som_device.region_props) returns raw integers per cell -- pixel count, coordinate sums, the sums of r^2, c^2
and r c, the border pixels in each of skimage.measure.perimeter's three weight classes, the convex image's area and
coordinate sums, the number of concavities.  This module turns them into the float columns with a handful of binary64
operations (:func:`morphology`, :func:`props_frame`), and restates the integer geometry in numpy for the cells the
device leaves out (bounding box past 64 x 64: :func:`fill_left_out`) -- identical integers, by the same rules.

A cell is every pixel of one label, connected or not.  skimage is taken by its documented algorithms; parity with
skimage itself is not pinned."""
import math

import numpy as np
import pandas as pd

from ..host_utils import verify_in_list

REGIONPROPS_BASE = ["label", "area", "eccentricity", "major_axis_length", "minor_axis_length", "perimeter", "centroid",
                    "convex_area", "equivalent_diameter"]                                       # ark.settings
REGIONPROPS_SINGLE_COMP = ["major_minor_axis_ratio", "perim_square_over_area", "major_axis_equiv_diam_ratio",
                           "convex_hull_resid", "centroid_dif", "num_concavities"]
REGIONPROPS_MULTI_COMP = ["nc_ratio"]
REGIONPROPS_FUNCTION_NAMES = REGIONPROPS_SINGLE_COMP + REGIONPROPS_MULTI_COMP                   # REGIONPROPS_FUNCTION's keys
BUILT_BASE = ("area", "eccentricity", "major_axis_length", "minor_axis_length", "perimeter", "centroid",
              "convex_area", "equivalent_diameter", "orientation", "euler_number")
CONCAVITY_DEFAULTS = {"small_concavity_minimum": 10, "max_compactness": 60, "large_concavity_minimum": 150}
MAX_SIDE = 64          # the device route of the hull ends at a 64 x 64 bounding box

SQRT2 = math.sqrt(2.0)
HALF_1_SQRT2 = (1.0 + SQRT2) / 2.0


def resolve_lists(regionprops_base=None, regionprops_single_comp=None, regionprops_multi_comp=None):
    """The three property lists as compute_marker_counts arranges them: a list not given takes the reference's default;
    ``coords`` is dropped (never a column), ``label`` comes first, a centroid is required.  Unknown derived properties
    raise verify_in_list's error, a base property that is not built NotImplementedError."""
    base = list(REGIONPROPS_BASE if regionprops_base is None else regionprops_base)
    single = list(REGIONPROPS_SINGLE_COMP if regionprops_single_comp is None else regionprops_single_comp)
    multi = list(REGIONPROPS_MULTI_COMP if regionprops_multi_comp is None else regionprops_multi_comp)
    if len(single) > 0:
        verify_in_list(extras_props=single, props_options=REGIONPROPS_FUNCTION_NAMES)
    if len(multi) > 0:
        verify_in_list(nuclear_props=multi, props_options=REGIONPROPS_FUNCTION_NAMES)
    base = [p for p in base if p != "coords"]
    if not any("centroid" in p for p in base):
        base.append("centroid")
    base = ["label"] + [p for p in base if p != "label"]
    for p in base[1:]:
        if p not in BUILT_BASE:
            raise NotImplementedError("regionprops_base: %r is not implemented; the built base properties are %s"
                                      % (p, ", ".join(BUILT_BASE)))
    for p in single:
        if p == "nc_ratio":
            raise NotImplementedError("regionprops_single_comp: 'nc_ratio' takes two compartments "
                                      "(regionprops_multi_comp)")
    for p in multi:
        if p != "nc_ratio":
            raise NotImplementedError("regionprops_multi_comp: %r takes one compartment (regionprops_single_comp)" % p)
    return base, single, multi


def table_names(base, single):
    """The morphology columns of the cell table after ``label``: the base properties in list order with ``centroid``
    replaced by ``centroid-0``, ``centroid-1`` at the end of the base block, then the single-compartment ones."""
    names = [p for p in base if p not in ("label", "centroid")]
    if "centroid" in base:
        names += ["centroid-0", "centroid-1"]
    return names + list(single)


def concavity_thresholds(**kwargs):
    return {k: kwargs.get(k, v) for k, v in CONCAVITY_DEFAULTS.items()}


# ---- integer geometry on the host (the route of the cells the device leaves out) ---------------------------------
def _shift(a, dr, dc):
    """a[r + dr, c + dc] with False outside."""
    h, w = a.shape
    out = np.zeros_like(a)
    out[max(0, -dr):h - max(0, dr), max(0, -dc):w - max(0, dc)] = a[max(0, dr):h + min(0, dr), max(0, dc):w + min(0, dc)]
    return out


def perimeter_counts(mask):
    """(n1, n2, n3): the border pixels of a boolean image in skimage.measure.perimeter's weight classes 1, sqrt 2 and
    (1 + sqrt 2) / 2 (neighbourhood 4; outside the image is background)."""
    mask = np.asarray(mask, dtype=bool)
    inner = mask & _shift(mask, -1, 0) & _shift(mask, 1, 0) & _shift(mask, 0, -1) & _shift(mask, 0, 1)
    border = mask & ~inner
    b = border.astype(np.int64)
    n4 = _shift(b, -1, 0) + _shift(b, 1, 0) + _shift(b, 0, -1) + _shift(b, 0, 1)
    nd = _shift(b, -1, -1) + _shift(b, -1, 1) + _shift(b, 1, -1) + _shift(b, 1, 1)
    code = (1 + 2 * n4 + 10 * nd)[border]
    return (int(np.isin(code, (5, 7, 15, 17, 25, 27)).sum()), int(np.isin(code, (21, 33)).sum()),
            int(np.isin(code, (13, 23)).sum()))


def perimeter_from_counts(n1, n2, n3):
    """n1 + n2 sqrt 2 + n3 (1 + sqrt 2) / 2 in binary64, in that order."""
    return (np.asarray(n1, dtype=np.float64) + np.asarray(n2, dtype=np.float64) * SQRT2) \
        + np.asarray(n3, dtype=np.float64) * HALF_1_SQRT2


def convex_rows(mask):
    """Per row of a boolean image whose first and last rows are not empty, the interval [lo, hi] of columns whose centre
    lies inside or on the hull of the diamond points (r +- 1/2, c), (r, c +- 1/2) of its pixels (hi < lo: none).  Doubled
    integer coordinates, monotone chain over the extremes of the doubled rows."""
    mask = np.asarray(mask, dtype=bool)
    h = mask.shape[0]
    left, right = {}, {}
    for i in range(h):
        cols = np.flatnonzero(mask[i])
        if cols.size == 0:
            continue
        lo, hi = int(cols[0]), int(cols[-1])
        for y, xl, xr in ((2 * i, 2 * lo + 2, 2 * hi + 2), (2 * i + 1, 2 * lo + 1, 2 * hi + 3),
                          (2 * i + 2, 2 * lo + 2, 2 * hi + 2)):
            left[y] = min(left.get(y, xl), xl)
            right[y] = max(right.get(y, xr), xr)

    def chain(pts, sign):
        st = []
        for y in sorted(pts):
            x = pts[y]
            while len(st) >= 2:
                (ya, xa), (yb, xb) = st[-2], st[-1]
                if sign * ((xb - xa) * (y - ya) - (x - xa) * (yb - ya)) >= 0:
                    st.pop()
                else:
                    break
            st.append((y, x))
        return st
    lo_chain, hi_chain = chain(left, 1), chain(right, -1)

    def at(st, y):
        j = 0
        while j + 2 < len(st) and st[j + 1][0] < y:
            j += 1
        (ya, xa), (yb, xb) = st[j], st[j + 1]
        dy = yb - ya
        return xa * dy + (xb - xa) * (y - ya), dy
    lo = np.zeros(h, dtype=np.int64)
    hi = np.zeros(h, dtype=np.int64)
    for i in range(h):
        num, dy = at(lo_chain, 2 * i + 1)
        lo[i] = -((-num) // (2 * dy)) - 1
        num, dy = at(hi_chain, 2 * i + 1)
        hi[i] = num // (2 * dy) - 1
    return lo, hi


def count_concavities(diff, small_concavity_minimum=10, max_compactness=60, large_concavity_minimum=150):
    """The 4-connected components of a boolean image that count as concavities (num_concavities' rule)."""
    from scipy import ndimage
    lab, _ = ndimage.label(diff)
    total = 0
    for idx, sl in enumerate(ndimage.find_objects(lab), start=1):
        comp = lab[sl] == idx
        a = float(int(comp.sum()))
        p = float(perimeter_from_counts(*perimeter_counts(comp)))
        if (a > small_concavity_minimum and (p * p) / a < max_compactness) or a > large_concavity_minimum:
            total += 1
    return total


def host_hull(mask, r0=0, c0=0, **thresholds):
    """(convex area, convex row sum, convex column sum, concavities) of one cell from its bounding-box crop, whose top
    left pixel is (r0, c0) of the image: the integers pxsom_region_hull returns."""
    mask = np.asarray(mask, dtype=bool)
    lo, hi = convex_rows(mask)
    length = np.maximum(hi - lo + 1, 0)
    rows = np.arange(mask.shape[0], dtype=np.int64)
    area = int(length.sum())
    sum_r = int(((rows + r0) * length).sum())
    sum_c = int((c0 * length + (lo + hi) * length // 2).sum())
    cols = np.arange(mask.shape[1], dtype=np.int64)[None, :]
    convex = (cols >= lo[:, None]) & (cols <= hi[:, None])
    return area, sum_r, sum_c, count_concavities(convex & ~mask, **concavity_thresholds(**thresholds))


# 4 E's term of the four bits (top left, top right, bottom left, bottom right) = (bit 0 .. bit 3) of one label in one
# 2 x 2 window: one bit +1, three bits -1, two bits on a diagonal -2
_QUAD_TERM = np.array([0, 1, 1, 0, 1, 0, -2, -1, 1, -2, 0, -1, 0, -1, -1, 0], dtype=np.int64)


def euler_numbers(seg, keys):
    """Per key, the Euler number of ``seg == key`` under 8-connectivity (objects minus holes, the plane padded by a zero
    border) by bit quads, as pxsom_region_euler states it: [n] int64."""
    seg = np.asarray(seg)
    keys = np.asarray(keys, dtype=np.int64)
    total = np.zeros(keys.size, dtype=np.int64)
    if keys.size == 0:
        return total
    p = np.zeros((seg.shape[0] + 2, seg.shape[1] + 2), dtype=np.int64)
    p[1:-1, 1:-1] = seg
    quad = [p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]]
    mixed = (quad[0] != quad[1]) | (quad[0] != quad[2]) | (quad[0] != quad[3])
    quad = [q[mixed] for q in quad]
    for i, lab in enumerate(quad):
        first = lab != 0                                  # every distinct label once, at its first position
        for earlier in quad[:i]:
            first &= earlier != lab
        bits = np.zeros(lab.size, dtype=np.int64)
        for j, other in enumerate(quad):
            bits |= (other == lab).astype(np.int64) << j
        pos = np.minimum(np.searchsorted(keys, lab), keys.size - 1)
        named = first & (keys[pos] == lab)
        np.add.at(total, pos[named], _QUAD_TERM[bits[named]])
    if np.any(total % 4):
        raise AssertionError("bit-quad totals must be multiples of 4")
    return total // 4


def host_raw(seg, keys=None, euler=False, **thresholds):
    """The contract of som_device.region_props as host arrays, computed in numpy for every cell (``left_out`` all 0):
    the statement the CPU tests put in the device's place, and the route of :func:`fill_left_out`."""
    seg = np.asarray(seg)
    if keys is None:
        keys = np.unique(seg)
        keys = keys[keys != 0]
    keys = np.asarray(keys, dtype=np.int64)
    n = keys.size
    out = {"keys": keys.astype(np.int32), "count": np.zeros(n, np.int64), "sums": np.zeros((n, 2), np.int64),
           "bbox": np.tile(np.array([2**31 - 1, -1, 2**31 - 1, -1], np.int32), (n, 1)),
           "shape": np.zeros((n, 6), np.int64), "hull": np.zeros((n, 4), np.int64), "left_out": np.zeros(n, np.int32)}
    if euler:           # som_device.region_euler's integers, which only the euler_number column needs
        out["euler"] = euler_numbers(seg, keys)
    if n == 0:
        return out
    from scipy import ndimage
    pos = np.searchsorted(keys, seg.astype(np.int64))
    pos = np.where((pos < n) & (keys[np.minimum(pos, n - 1)] == seg), pos + 1, 0)
    for i, sl in enumerate(ndimage.find_objects(pos, max_label=n)):
        if sl is None:
            continue
        r0, c0 = sl[0].start, sl[1].start
        mask = pos[sl] == i + 1
        rr, cc = np.nonzero(mask)
        rr, cc = rr.astype(np.int64) + r0, cc.astype(np.int64) + c0
        out["count"][i] = rr.size
        out["sums"][i] = (rr.sum(), cc.sum())
        out["bbox"][i] = (r0, sl[0].stop - 1, c0, sl[1].stop - 1)
        out["shape"][i] = ((rr * rr).sum(), (cc * cc).sum(), (rr * cc).sum()) + perimeter_counts(mask)
        out["hull"][i] = host_hull(mask, r0, c0, **thresholds)
    return out


def fill_left_out(raw, seg, **thresholds):
    """Fills the ``hull`` rows of the cells the device left out (``left_out`` == 1) by the host route; ``raw`` holds
    host arrays and is changed in place."""
    seg = np.asarray(seg)
    for i in np.flatnonzero(np.asarray(raw["left_out"])):
        r0, r1, c0, c1 = (int(v) for v in raw["bbox"][i])
        mask = seg[r0:r1 + 1, c0:c1 + 1] == raw["keys"][i]
        raw["hull"][i] = host_hull(mask, r0, c0, **thresholds)
        raw["left_out"][i] = 0
    return raw


# ---- the float columns from the raw integers --------------------------------------------------------------------
def _ints(a):
    return [int(v) for v in np.asarray(a).ravel()]


def morphology(raw, orientation=False):
    """Every built column (base and single-compartment) of the cells of ``raw`` as a dict of arrays; ``euler_number``
    when ``raw`` holds ``euler`` (the integers of som_device.region_euler) and ``orientation`` on request (one atan2 per
    cell, which only that column needs).  The central second
    moments come from exact integer numerators (n sum r^2 - (sum r)^2 and its siblings, Python integers) with one
    rounding per quotient; the eigenvalues of the inertia tensor [[mu02, -mu11], [-mu11, mu20]] / n are l1 from the
    trace and the discriminant and l2 = det / l1, the determinant again one exact integer quotient."""
    n = _ints(raw["count"])
    sums = np.asarray(raw["sums"], dtype=np.int64).reshape(-1, 2)
    shape = np.asarray(raw["shape"], dtype=np.int64).reshape(-1, 6)
    hull = np.asarray(raw["hull"], dtype=np.int64).reshape(-1, 4)
    m = len(n)
    a = np.zeros(m)
    d = np.zeros(m)
    b = np.zeros(m)
    det = np.zeros(m)
    theta = np.zeros(m)
    for i in range(m):
        ni, sr, sc = n[i], int(sums[i, 0]), int(sums[i, 1])
        if ni == 0:
            continue
        srr, scc, src = int(shape[i, 0]), int(shape[i, 1]), int(shape[i, 2])
        num_a, num_d, num_b = ni * scc - sc * sc, ni * srr - sr * sr, ni * src - sr * sc
        a[i], d[i], b[i] = num_a / (ni * ni), num_d / (ni * ni), -num_b / (ni * ni)
        # skimage 0.19 RegionProperties.orientation over the inertia tensor [[a, b], [b, d]], b by float negation: a zero
        # mu11 gives -0.0, the sign skimage's -mu11 / mu00 has (math.atan2: one libm call per cell, no SIMD variant)
        if orientation:
            b_neg = -(num_b / (ni * ni))
            if a[i] == d[i]:
                theta[i] = -math.pi / 4 if b_neg < 0 else math.pi / 4
            else:
                theta[i] = 0.5 * math.atan2(-2 * b_neg, d[i] - a[i])
        det[i] = (num_a * num_d - num_b * num_b) / (ni ** 4)
    area = np.asarray(n, dtype=np.float64)
    l1 = np.maximum((a + d) / 2 + np.sqrt(((a - d) / 2) ** 2 + b * b), 0.0)
    l2 = np.maximum(np.divide(det, l1, out=np.zeros(m), where=l1 > 0), 0.0)
    l2 = np.minimum(l2, l1)
    major, minor = 4 * np.sqrt(l1), 4 * np.sqrt(l2)
    ecc = np.sqrt(1 - np.divide(l2, l1, out=np.ones(m), where=l1 > 0))
    perimeter = perimeter_from_counts(shape[:, 3], shape[:, 4], shape[:, 5])
    equiv = np.sqrt(4 * area / np.pi)
    convex = hull[:, 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cent = np.stack([sums[:, 0] / area, sums[:, 1] / area], axis=1)
        ccent = np.stack([hull[:, 1] / convex, hull[:, 2] / convex], axis=1)
        dif = cent - ccent
        out = {
            "area": np.asarray(n, dtype=np.int64), "eccentricity": ecc, "major_axis_length": major,
            "minor_axis_length": minor, "perimeter": perimeter, "centroid-0": cent[:, 0], "centroid-1": cent[:, 1],
            "convex_area": hull[:, 0].copy(), "equivalent_diameter": equiv,
            "major_minor_axis_ratio": np.where(minor == 0, np.nan, major / np.where(minor == 0, 1.0, minor)),
            "perim_square_over_area": np.square(perimeter) / area,
            "major_axis_equiv_diam_ratio": major / equiv,
            "convex_hull_resid": (convex - area) / convex,
            "centroid_dif": np.sqrt(dif[:, 0] * dif[:, 0] + dif[:, 1] * dif[:, 1]) / np.sqrt(area),
            "num_concavities": hull[:, 3].copy(),
            "eigenvalues": np.stack([l1, l2], axis=1),
        }
    if orientation:
        out["orientation"] = theta
    if "euler" in raw:
        out["euler_number"] = np.asarray(raw["euler"], dtype=np.int64).copy()
    return out


def props_frame(raw, base, single):
    """get_single_compartment_props' frame (without ``coords``): the base properties in list order, ``centroid`` as
    ``centroid-0`` and ``centroid-1`` in its place, then the single-compartment ones; one row per cell, labels ascending."""
    names = []
    for p in base:
        names += ["centroid-0", "centroid-1"] if p == "centroid" else [p]
    names += list(single)
    cols = morphology(raw, orientation="orientation" in names)
    cols["label"] = np.asarray(raw["keys"], dtype=np.int64)
    return pd.DataFrame({name: cols[name] for name in names}, columns=names)
