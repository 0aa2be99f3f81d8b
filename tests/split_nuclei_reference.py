"""Numpy statements of split_large_nuclei and the planes its tests run on.

``split_loop`` is the reference's loop written out (ark/segmentation/segmentation_utils.py:41-90): regionprops' coords
are a cell's pixels in raster order (cell_table_reference.cell_coords), ``remove_small_objects`` on an integer array is a
size table over the label values -- no connected components.  ``split_vec`` computes the same plane from the counts of
the (cell, nucleus) pairs, the way the device chain does, without sharing code with it."""
import numpy as np

from tests import cell_table_reference as ctr


def remove_small(plane, small=5):
    """skimage.morphology.remove_small_objects(ar, min_size=small) for an integer ``ar``: every pixel whose label value
    occurs fewer than ``small`` times becomes 0."""
    _, inverse, counts = np.unique(plane, return_inverse=True, return_counts=True)
    return np.where((counts < small)[inverse.reshape(plane.shape)], 0, plane).astype(plane.dtype)


def split_loop(cell, nuc, cell_ids, min_size=15, small=5):
    """(modified nuclear plane, number of splits): the reference's loop, literally.  The running maximum is a Python
    int: the statement is defined where the new labels fit the plane's dtype."""
    out = np.copy(nuc)
    top = int(np.max(nuc))
    coords = ctr.cell_coords(cell)
    n_splits = 0
    for c in cell_ids:
        co = coords[int(c)]
        ids, counts = np.unique(nuc[tuple(co.T)], return_counts=True)
        if ids[ids != 0].size == 0:
            continue
        nuc_id = ids[ids != 0][np.argmax(counts[ids != 0])]
        nuc_count = np.sum(nuc[tuple(co.T)] == nuc_id)
        nuc_mask = nuc == nuc_id
        if np.sum(nuc_mask) - nuc_count > min_size:
            top += 1
            n_splits += 1
            out[np.logical_and(cell == c, nuc_mask)] = top
    return remove_small(out, small), n_splits


def pair_tables(cell, nuc):
    """(cell labels, nuclear labels, best [n_cells], inside [n_cells], area [n_nuc]): per cell the index of the nuclear
    label with the most pixels inside it (the smaller on a tie, -1: none) and that count; per nucleus its pixels."""
    ck = np.unique(cell)
    ck = ck[ck != 0].astype(np.int64)
    nk, area = np.unique(nuc[nuc != 0], return_counts=True)
    nk = nk.astype(np.int64)
    best = np.full(ck.size, -1, np.int64)
    inside = np.zeros(ck.size, np.int64)
    both = (cell != 0) & (nuc != 0)
    if both.any():
        ci, ni = np.searchsorted(ck, cell[both]), np.searchsorted(nk, nuc[both])
        pairs, counts = np.unique(ci.astype(np.int64) * nk.size + ni, return_counts=True)
        pc, pn = pairs // nk.size, pairs % nk.size
        order = np.lexsort((pn, -counts, pc))              # by cell, then more pixels first, then the smaller nucleus
        first = np.ones(order.size, bool)
        first[1:] = pc[order][1:] != pc[order][:-1]
        best[pc[order][first]] = pn[order][first]
        inside[pc[order][first]] = counts[order][first]
    return ck, nk, best, inside, area.astype(np.int64)


def split_vec(cell, nuc, cell_ids, min_size=15, small=5):
    """(modified nuclear plane, number of splits) from the pair counts: a new label has ``inside`` pixels, a split nucleus
    keeps its area minus the ``inside`` of the distinct cells that split it, an id named twice leaves its earlier number
    without pixels."""
    ck, nk, best, inside, area = pair_tables(cell, nuc)
    top = int(nk[-1]) if nk.size else 0
    where = {int(c): i for i, c in enumerate(ck)}
    new_label, n_splits = {}, 0
    for c in cell_ids:                                       # the caller's order, duplicates included
        i = where[int(c)]                                    # KeyError: no label of the cell plane
        if best[i] >= 0 and area[best[i]] - inside[i] > min_size:
            top += 1
            n_splits += 1
            new_label[i] = top
    remaining = area.copy()
    for i in new_label:
        remaining[best[i]] -= inside[i]
    nuc_value = np.where(remaining < small, 0, nk)
    cell_value = np.full(ck.size, -1, np.int64)
    for i, lab in new_label.items():
        cell_value[i] = lab if inside[i] >= small else 0
    ci = np.where(cell != 0, np.searchsorted(ck, cell), -1) if ck.size else np.full(cell.shape, -1)
    ni = np.where(nuc != 0, np.searchsorted(nk, nuc), -1) if nk.size else np.full(nuc.shape, -1)
    ci_safe, ni_safe = np.maximum(ci, 0), np.maximum(ni, 0)
    out = nuc.astype(np.int64)
    if nk.size:
        out = np.where(ni >= 0, nuc_value[ni_safe], out)
    if ck.size and nk.size:
        takes = (ci >= 0) & (ni >= 0) & (best[ci_safe] == ni) & (cell_value[ci_safe] >= 0)
        out = np.where(takes, cell_value[ci_safe], out)
    return out.astype(nuc.dtype), n_splits


# ---- planes -------------------------------------------------------------------------------------------------------
def nuclei(h, w, n_cells, seed, shift=3):
    """Nuclei for ``ctr.voronoi_labels(h, w, n_cells, seed=seed)``: the Voronoi field of the same seed without background,
    shifted by ``shift`` pixels and eroded by 2, so that most nuclei straddle a cell border and a cytoplasm ring remains."""
    v = ctr.voronoi_labels(h + shift, w + shift, n_cells, seed=seed, background=0.0)[shift:shift + h, shift:shift + w]
    keep = np.ones_like(v, bool)
    for dy, dx in ((2, 0), (-2, 0), (0, 2), (0, -2)):
        keep &= np.roll(v, (dy, dx), (0, 1)) == v
    return np.where(keep, v, 0)


def facts(cell, nuc, cell_ids, min_size=15, small=5):
    """What happens on a case: splits, labels removed as small (remnants of a split nucleus, new pieces), cells without
    a nucleus, nuclei chosen by two cells or more, and the outside counts ``area - inside`` of the cells with a nucleus."""
    ck, nk, best, inside, area = pair_tables(cell, nuc)
    out, n_splits = split_vec(cell, nuc, cell_ids, min_size, small)
    top = int(nk[-1]) if nk.size else 0
    before_small = split_vec(cell, nuc, cell_ids, min_size, small=0)[0]
    gone = np.setdiff1d(np.unique(before_small), np.unique(out))
    chosen = best[best >= 0]
    return dict(splits=n_splits, dropped_remnants=int((gone <= top).sum()), dropped_new=int((gone > top).sum()),
                cells_without_nucleus=int((best < 0).sum()), nuclei=int(nk.size), cells=int(ck.size),
                shared_nuclei=int((np.bincount(chosen, minlength=max(nk.size, 1)) >= 2).sum()),
                outside=area[chosen] - inside[best >= 0])


def voronoi_case(h, w, n_cells, seed, dtype=np.int32):
    """(cell, nuc): the Voronoi cells and their shifted nuclei, one cell's nuclear pixels cleared (a cell without a
    nucleus) -- the largest cell's, so that its neighbours' nuclei are cut too and leave small pieces behind."""
    cell = ctr.voronoi_labels(h, w, n_cells, seed=seed)
    nuc = nuclei(h, w, n_cells, seed)
    labels, counts = np.unique(cell[cell != 0], return_counts=True)
    nuc = np.where(cell == labels[np.argmax(counts)], 0, nuc)
    return cell.astype(dtype), nuc.astype(dtype)


def ids_of(kind, cell, rng):
    """The ``cell_ids`` orders the tests use: every label ascending, reversed, a shuffled half, with duplicates."""
    ids = np.unique(cell)
    ids = ids[ids != 0].astype(np.int64)
    if kind == "ascending":
        return ids
    if kind == "reversed":
        return ids[::-1].copy()
    if kind == "subset":
        return rng.permutation(ids)[:max(1, ids.size // 2)]
    if kind == "duplicates":
        return np.concatenate([ids[:ids.size // 2], ids[::-1], ids[ids.size // 3:]])
    raise ValueError(kind)


ID_KINDS = ("ascending", "reversed", "subset", "duplicates")
LABEL_DTYPES = (np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64)
FUZZ_SIZES = ((40, 64), (64, 64), (71, 129), (96, 130), (130, 67))
FUZZ_LAYOUTS = ("contiguous", "offset", "padded")
FUZZ_MIN_SIZES = ("zero", "default", "edge")


def edge_min_size(outside):
    """A ``min_size`` that puts one cell of the case exactly on the strict compare (``area - inside == min_size``: no
    split) while a cell with more pixels outside still splits: the second largest distinct outside count."""
    values = np.unique(outside)
    return int(values[-2]) if values.size >= 2 else 0


def fuzz_case(index):
    """Case ``index`` of the seeded sweep: dict(cell, nuc, cell_ids, min_size, layout, force_search).  The classes
    (size, dtype pair, layout, min_size kind, cell_ids kind) are dealt round robin with co-prime strides so that 60 cases
    meet every value of every class; the planes of a case are redrawn, by seed, until the case contains a split."""
    h, w = FUZZ_SIZES[index % len(FUZZ_SIZES)]
    cell_dtype = LABEL_DTYPES[index % len(LABEL_DTYPES)]
    nuc_dtype = LABEL_DTYPES[(index // 6 + index) % len(LABEL_DTYPES)]          # every pair within 36 cases
    layout = FUZZ_LAYOUTS[(index // 5) % len(FUZZ_LAYOUTS)]
    min_kind = FUZZ_MIN_SIZES[(index // 3 + index) % len(FUZZ_MIN_SIZES)]
    id_kind = ID_KINDS[(index // 7 + index) % len(ID_KINDS)]
    n_cells = 10 + (index * 7) % 23
    for attempt in range(50):
        seed = 1000 * index + attempt
        rng = np.random.default_rng(seed)
        cell, nuc = voronoi_case(h, w, n_cells, seed)
        ids = ids_of(id_kind, cell, rng)
        ck, _, best, inside, area = pair_tables(cell, nuc)
        named = np.isin(ck, ids) & (best >= 0)
        outside = area[best[named]] - inside[named]
        min_size = {"zero": 0, "default": 15, "edge": edge_min_size(outside)}[min_kind]
        if outside.size and (outside > min_size).any() and (min_kind != "edge" or (outside == min_size).any()):
            return dict(cell=cell.astype(cell_dtype), nuc=nuc.astype(nuc_dtype), cell_ids=ids, min_size=min_size,
                        layout=layout, force_search=bool(index & 1), min_kind=min_kind, id_kind=id_kind)
    raise AssertionError("fuzz case %d: no plane with a split in 50 draws" % index)


N_FUZZ = 60


# ---- the hand-built plane -----------------------------------------------------------------------------------------
def hand_plane():
    """(cell, nuc, notes) on 24 x 70: runs that cross the 64-pixel group and the row end, with every decision on its
    edge (min_size 15, small 5).  Cells are horizontal bands of 2 rows; ``notes`` names what each is there for."""
    h, w = 24, 70
    cell = np.zeros((h, w), np.int32)
    nuc = np.zeros((h, w), np.int32)
    notes = {}

    def band(label, r0, rows=2, c0=0, c1=w):
        cell[r0:r0 + rows, c0:c1] = label

    def paint(label, r, c0, n):
        """n pixels of a nucleus in raster order from (r, c0), wrapping at the row end"""
        flat = nuc.reshape(-1)
        flat[r * w + c0:r * w + c0 + n] = label
    # cell 1 (rows 0-1): nucleus 11 has 20 pixels inside (flat 120 .. 139: across the 64-pixel group boundary at 128) and
    # exactly 15 outside (in the background row 2): no split
    band(1, 0)
    paint(11, 1, 50, 20)
    paint(11, 2, 0, 15)
    notes["no_split_at_min_size"] = (1, 11)
    # cell 2 (rows 3-4): nucleus 12 has 20 inside, 16 outside (background row 5): split; its run inside the cell goes
    # over the row end (row 3 column 60 .. row 4 column 9)
    band(2, 3)
    paint(12, 3, 60, 20)
    paint(12, 5, 0, 16)
    notes["split_at_min_size_plus_1"] = (2, 12)
    # cell 3 (rows 6-7): nucleus 13, 30 inside; outside: 4 pixels in cell 4 (the remnant ... see below) + 16 in background
    # cells 3 and 4 share nucleus 13; cell 5 takes it too: one nucleus taken by three cells
    band(3, 6)
    band(4, 8, rows=1)
    band(5, 9, rows=1)
    paint(13, 7, 20, 30)           # cell 3: 30
    paint(13, 8, 20, 25)           # cell 4: 25
    paint(13, 9, 20, 21)           # cell 5: 21
    paint(13, 10, 20, 4)           # background: 4 -> the remnant after three splits has 4 pixels: dropped
    notes["nucleus_taken_by_three_cells_remnant_4"] = (3, 4, 5, 13)
    # cell 6 (rows 11-12): nucleus 14, 20 inside, 16 + 5 outside, of which 16 in cell 7 (which prefers 14 as well) and 5
    # in the background: the remnant has 5 pixels: kept
    band(6, 11)
    band(7, 13, rows=1)
    paint(14, 12, 5, 20)
    paint(14, 13, 5, 16)
    paint(14, 14, 5, 5)
    notes["remnant_5_kept"] = (6, 7, 14)
    # cell 8 (row 15, columns 0-34): new piece of 4 pixels of nucleus 15 (30 outside): the piece is dropped
    # cell 9 (row 15, columns 35-69): new piece of 5 pixels of nucleus 16 (30 outside): kept
    band(8, 15, rows=1, c0=0, c1=35)
    band(9, 15, rows=1, c0=35, c1=w)
    paint(15, 15, 10, 4)
    paint(15, 16, 0, 30)
    paint(16, 15, 40, 5)
    paint(16, 16, 35, 30)
    notes["new_piece_4_dropped"] = (8, 15)
    notes["new_piece_5_kept"] = (9, 16)
    # cell 10 (rows 17-18): a tie of nuclei 17 and 18, 10 pixels each inside; 17 has 16 outside (splits), 18 has 3
    band(10, 17)
    paint(17, 17, 0, 10)
    paint(18, 17, 30, 10)
    paint(17, 19, 0, 16)
    paint(18, 19, 30, 3)
    notes["tie_smaller_label_splits"] = (10, 17, 18)
    # nucleus 19 over background only (row 20); cell 11 (rows 21-22) has no nucleus
    paint(19, 20, 10, 12)
    band(11, 21)
    notes["nucleus_over_background"] = 19
    notes["cell_without_nucleus"] = 11
    return cell, nuc, notes
