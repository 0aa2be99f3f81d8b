"""The statement of K28 (include/pxsom.h "K28"): skimage 0.19's ``watershed(image, markers)`` at its defaults, as recalled,
in two forms.

:func:`watershed` is the sequential form, a priority flood over ``heapq`` keyed ``(value, age)``: connectivity 1, no mask,
no compactness, no watershed line; a pixel is labelled when it is pushed.  What is recalled and not pinned by an installed
skimage is named in ``fiber_segmentation.RECALLED_WATERSHED``: markers of one value pop in raster order (skimage gives all
of them age 0 and leaves equal keys to its binary heap), and the neighbours are visited in the order -W, -1, +1, +W.

:func:`watershed_rounds` computes the same labels the way csrc/pxsom_watershed.hip does: level by level, and inside a level
in rounds that pop the whole frontier at once -- claims by the smallest key ``8 i + k``, basins below the level taken whole
with their rim claimed at ``8 i + 4``, ordered emission into the next frontier and the pending list.  ``shuffle`` (a
RandomState) orders equal keys at random: the labels must not depend on it.  Its equality with the heap form is a test."""
import heapq

import numpy as np

from ark_analysis_amd.segmentation import fiber_segmentation as fs

G28_NAMES = ("bars", "bars_small", "speckle", "disc", "blob_hole", "borders", "wide", "tall")   # g28's (elevation, markers) pairs
BASIN_CASES = ("ring_basin", "basin_in_basin", "basin_two_labels", "basin_two_labels_swapped", "rim_basin_first",
               "rim_direct_first", "int32_range")              # the hand_cases() that take the basin path
NEIGHBOUR_ORDERS = {"-W,-1,+1,+W": ((-1, 0), (0, -1), (0, 1), (1, 0)), "+W,+1,-1,-W": ((1, 0), (0, 1), (0, -1), (-1, 0))}


def _rules(recalled):
    rules = dict(fs.RECALLED_WATERSHED, **(recalled or {}))
    for name, value in rules.items():
        if value not in fs.WATERSHED_CHOICES.get(name, ()):
            raise ValueError("RECALLED_WATERSHED: %s=%r is not one of %s" % (name, value, fs.WATERSHED_CHOICES.get(name)))
    return rules


def _planes(image, markers):
    image, markers = np.asarray(image), np.asarray(markers)
    if image.ndim != 2 or image.shape != markers.shape or image.size == 0:
        raise ValueError("image and markers must be non-empty [H, W] arrays of one shape")
    return image.astype(np.int32), markers.astype(np.int32)


def _neighbours(i, h, w, steps):
    y, x = divmod(i, w)
    for k, (dy, dx) in enumerate(steps):
        if 0 <= y + dy < h and 0 <= x + dx < w:
            yield k, (y + dy) * w + x + dx


def watershed(image, markers, recalled=None):
    """The heap form: int32 ``[H, W]`` labels.  Any non-zero marker value is a label; a plane without a marker returns all
    zeros."""
    rules = _rules(recalled)
    image, markers = _planes(image, markers)
    h, w = image.shape
    steps = NEIGHBOUR_ORDERS[rules["neighbours"]]
    out = markers.ravel().copy()
    v = image.ravel()
    heap, age = [], 0
    first = np.flatnonzero(out)
    for i in (first if rules["marker_ties"] == "raster" else first[::-1]):
        heap.append((int(v[i]), age, int(i)))
        age += 1
    heapq.heapify(heap)
    while heap:
        _, _, i = heapq.heappop(heap)
        for _, n in _neighbours(i, h, w, steps):
            if out[n] == 0:
                out[n] = out[i]
                heapq.heappush(heap, (int(v[n]), age, n))
                age += 1
    return out.reshape(h, w)


def _components(member, h, w):
    """The 4-connected components of the pixel set ``member`` as lists of pixels."""
    seen, comps = set(), []
    for start in sorted(member):
        if start in seen:
            continue
        seen.add(start)
        comp, stack = [], [start]
        while stack:
            p = stack.pop()
            comp.append(p)
            for _, n in _neighbours(p, h, w, NEIGHBOUR_ORDERS["-W,-1,+1,+W"]):
                if n in member and n not in seen:
                    seen.add(n)
                    stack.append(n)
        comps.append(comp)
    return comps


def watershed_rounds(image, markers, shuffle=None, stats=None):
    """The round form: the labels of :func:`watershed` under the default switches.  ``stats``: a dict that receives
    ``rounds``, ``levels``, ``descents`` (rounds that took the basin path) and ``labelled`` (pixels the flood labelled)."""
    image, markers = _planes(image, markers)
    h, w = image.shape
    total = h * w
    steps = NEIGHBOUR_ORDERS["-W,-1,+1,+W"]
    out = markers.ravel().copy()
    v = image.ravel()
    pending = [int(i) for i in np.flatnonzero(out)]                      # the markers in raster order
    rounds = levels = descents = labelled = 0
    while pending:
        level = min(int(v[p]) for p in pending)
        frontier = [p for p in pending if v[p] == level]
        pending = [p for p in pending if v[p] != level]
        levels += 1
        assert levels <= total + 1
        while frontier:
            rounds += 1
            assert rounds <= total + 1
            claim = {}
            for i, p in enumerate(frontier):                              # 1. direct claims
                for k, n in _neighbours(p, h, w, steps):
                    if out[n] == 0:
                        claim[n] = min(claim.get(n, 8 * i + k), 8 * i + k)
            basin = {}
            if any(v[n] < level for n in claim):                          # 2. descents
                descents += 1
                below = {p for p in range(total) if out[p] == 0 and v[p] < level}
                for comp in _components(below, h, w):
                    keys = [claim[p] for p in comp if p in claim]
                    if not keys:
                        continue
                    parent = min(keys) >> 3
                    for p in comp:
                        basin[p] = parent
                        for _, n in _neighbours(p, h, w, steps):
                            if out[n] == 0 and v[n] >= level:
                                claim[n] = min(claim.get(n, 8 * parent + 4), 8 * parent + 4)
            winners = [(key, n) for n, key in claim.items() if v[n] >= level]
            for key, n in winners:                                        # 3. labelling
                out[n] = out[frontier[key >> 3]]
            for p, parent in basin.items():
                out[p] = out[frontier[parent]]
            labelled += len(winners) + len(basin)
            tie = {n: (shuffle.random_sample() if shuffle is not None else n) for _, n in winners}
            winners.sort(key=lambda kn: (kn[0], tie[kn[1]]))              # 4. next lists, by key
            frontier = [n for _, n in winners if v[n] == level]
            pending += [n for _, n in winners if v[n] > level]
    if stats is not None:
        stats.update(rounds=rounds, levels=levels, descents=descents, labelled=labelled)
    return out.reshape(h, w)


# ---- the rest of segment_fibers behind the watershed, as numpy / scipy state it ---------------------------------------------
def filtered_labels(elevation, markers, min_fiber_size):
    """``watershed(...) - 1`` (the pixels of marker class 2), ``ndi.label`` (4-connected), the components under
    ``min_fiber_size`` pixels removed and not renumbered: int32."""
    from scipy import ndimage as ndi
    labels, _ = ndi.label(watershed(elevation, markers) == 2)
    areas = np.bincount(labels.ravel())
    keep = areas >= min_fiber_size
    keep[0] = False
    return np.where(keep[labels], labels, 0).astype(np.int32)


# ---- planes for the tests and the fixture -------------------------------------------------------------------------------------
def ring(h, w, wall=9, inside=-2, outside=0):
    """A one-pixel wall around a lower inside, one pixel in from the border: a basin the flood can only enter over the wall."""
    image = np.full((h, w), outside, np.int32)
    image[1:h - 1, 1:w - 1] = wall
    image[2:h - 2, 2:w - 2] = inside
    return image


def hand_cases():
    """name -> (image, markers): the planes made by hand for the fixture and the GPU tests, small enough to read."""
    cases = {}
    flat = np.zeros((5, 9), np.int32)
    m = np.zeros((5, 9), np.int32)
    m[2, 0], m[2, 8] = 1, 2
    cases["flat_two_labels"] = (flat, m)                                 # the middle column is a tie: the earlier marker's
    m = np.zeros((5, 9), np.int32)
    m[2, 0], m[2, 8] = 2, 1
    cases["flat_two_labels_swapped"] = (flat, m)
    # a ring wall with a lower basin inside: one descent
    image = ring(9, 11)
    m = np.zeros_like(image)
    m[0, 0] = 5
    cases["ring_basin"] = (image, m)
    # a basin inside a basin
    image = ring(13, 13, wall=9, inside=3)
    image[4:9, 4:9] = 6
    image[5:8, 5:8] = -4
    m = np.zeros_like(image)
    m[0, 6] = 7
    cases["basin_in_basin"] = (image, m)
    # one basin entered in the same round from two labels: a corridor of zeros leads each label to the basin's wall gap
    for name, (a, b) in (("basin_two_labels", (1, 2)), ("basin_two_labels_swapped", (2, 1))):
        image = np.full((7, 9), 5, np.int32)
        image[3, :] = 0                                                  # the corridor row
        image[2:5, 3:6] = -3                                             # the basin, open to the corridor on both sides
        m = np.zeros_like(image)
        m[3, 0], m[3, 8] = a, b
        cases[name] = (image, m)
    # a rim pixel claimed directly by one label and through a basin by another in one round
    # in both orders: the basin's parent first (the rim claim 8 * 0 + 4 wins), and the direct claimant first (8 * 0 + 2 wins)
    for name, cols in (("rim_basin_first", slice(2, 4)), ("rim_direct_first", slice(3, 5))):
        image = np.zeros((5, 7), np.int32)
        image[1:4, cols] = -2                                            # the basin, entered from the marker beside it
        m = np.zeros_like(image)
        m[2, 1], m[2, 5] = 1, 2                                          # the other marker claims the rim pixel between
        cases[name] = (image, m)
    # a 40-level staircase with a marker at both ends
    image = np.repeat(np.arange(40, dtype=np.int32)[None, :], 3, axis=0)
    m = np.zeros_like(image)
    m[1, 0], m[1, 39] = 3, 4
    cases["staircase"] = (image, m)
    # the int32 range, negative elevations
    image = np.array([[-2 ** 31, 2 ** 31 - 1, -5, 0, 7], [3, -2 ** 31, 2 ** 31 - 1, -1, 2], [0, 0, -7, 2 ** 31 - 1, -2 ** 31]], np.int32)
    m = np.zeros_like(image)
    m[0, 4], m[2, 0] = 1, 2
    cases["int32_range"] = (image, m)
    # negative and large marker values
    image = (np.arange(42, dtype=np.int32).reshape(6, 7) * 5) % 7
    m = np.zeros_like(image)
    m[0, 0], m[5, 6], m[2, 3] = -3, 2 ** 31 - 1, -2 ** 31
    cases["marker_values"] = (image, m)
    return cases


def serpentine(h=33, w=130):
    """A corridor of zeros that winds through walls of 9, a marker at its start: about ``h w / 2`` rounds."""
    image = np.full((h, w), 9, np.int32)
    for y in range(0, h, 2):
        image[y, :] = 0
        if y + 1 < h:
            image[y + 1, w - 1 if (y // 2) % 2 == 0 else 0] = 0
    m = np.zeros_like(image)
    m[0, 0] = 1
    return image, m


def shape_cases(h, w):
    """name -> (image, markers) for one shape: the cases that exist at any size, and the basins where they fit."""
    rs = np.random.RandomState(1000 * h + w)
    yy, xx = np.mgrid[:h, :w]
    zeros = np.zeros((h, w), np.int32)
    noise = rs.randint(-1, 3, (h, w)).astype(np.int32)
    cases = {"no_marker": (noise, zeros)}
    m = zeros.copy()
    m[h // 2, w // 3] = 4
    cases["one_marker"] = (noise, m)
    cases["one_marker_flat"] = (zeros, m)
    cases["all_markers"] = (noise, rs.randint(1, 4, (h, w)).astype(np.int32))
    if h * w > 1:
        for name, (a, b) in (("flat_two_labels", (1, 2)), ("flat_two_labels_swapped", (2, 1))):
            m = zeros.copy()
            m[0, 0], m[h - 1, w - 1] = a, b
            cases[name] = (zeros, m)
    cases["checkerboard"] = (noise, (((yy + xx) % 2) * (1 + yy % 3)).astype(np.int32))
    sparse = ((rs.random_sample((h, w)) < 0.03) * rs.randint(1, 4, (h, w))).astype(np.int32)
    sparse[rs.randint(h), rs.randint(w)] = 3
    cases["levels"] = ((rs.randint(0, 4, (h, w)) * 3 - 4).astype(np.int32), sparse)
    if h >= 5 and w >= 5:
        m = zeros.copy()
        m[0, 0], m[h - 1, w - 1] = 5, 6
        cases["ring_basin"] = (ring(h, w), m)
    if h >= 9 and w >= 9:
        image = ring(h, w, wall=9, inside=3)
        image[4:h - 4, 4:w - 4] = 6
        image[5:h - 5, 5:w - 5] = -4 if h >= 11 and w >= 11 else 6
        m = zeros.copy()
        m[0, w // 2] = 7
        cases["basin_in_basin"] = (image, m)
    return cases


def random_case(rs, max_side=8):
    """A small random plane: up to four levels, scaled by -3 .. 3, marker density 0.05 .. 0.4, three labels."""
    h, w = rs.randint(1, max_side + 1), rs.randint(1, max_side + 1)
    image = (rs.randint(0, rs.randint(1, 5), (h, w)) * rs.randint(-3, 4)).astype(np.int32)
    m = (rs.random_sample((h, w)) < rs.uniform(0.05, 0.4)) * rs.randint(1, 4, (h, w))
    return image, m.astype(np.int32)
