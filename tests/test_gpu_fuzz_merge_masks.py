"""Randomised sweep of K18 (som_device.label_regions, pair_overlaps, merge_apply and the chain merge_masks) against the
numpy + scipy statement of tests/merge_masks_reference.py; the comparison is exact.  Case i takes class i % R of the table
CLASSES -- a size class, the mask dtype, a layout, a kind of overlap_thresh and a kind of expansion_factor, every value of
every factor visited -- and draws the rest (seeded).  A default run is max(12, R) cases and skips none.
``PXSOM_FUZZ_SEED`` as in test_gpu_fuzz_parity.py; ``PXSOM_FUZZ_CASES`` widens the run.  The generator is device-free.

The statement loops objects x cells in Python, so every layout keeps the product of the two region counts in the
low ten thousands.  A "tie" threshold is built from the statement's own pair list: ``overlap / area`` of one pair equals
``thresh / 100`` in binary64, and the statement decides differently once its threshold compare is ``>=``."""
import os

import numpy as np
import pytest

from tests import merge_masks_reference as mmr

DEFAULT_SEED = 20261018
SEED = int(os.environ.get("PXSOM_FUZZ_SEED", str(DEFAULT_SEED)))
SIZES = ["small", "tile", "tiles", "wide"]
DTYPES = ["uint8", "int16", "uint16", "int32", "uint32", "int64"]
LAYOUTS = ["discs", "dense", "stripes", "pieces"]
THRESHOLDS = ["zero", "middle", "hundred", "tie"]
GROWS = ["zero", "three", "huge"]
CLASSES = [(SIZES[i % 4], DTYPES[i % 6], LAYOUTS[(i + i // 4) % 4], THRESHOLDS[(i + i // 2) % 4], GROWS[(i // 4) % 3])
           for i in range(12)]
R = len(CLASSES)
CASES = max(int(os.environ.get("PXSOM_FUZZ_CASES", "0")), 12, R)
T = 64
STRICT = (lambda x, y: x > y), (lambda x, y: x > y)
LOOSE = (lambda x, y: x > y), (lambda x, y: x >= y)          # the threshold compare of the choice as >=


def _blocks(rs, h, w, top, most):
    """randint(0, top) in square blocks, the block edge the smallest that keeps the blocks at or below ``most``."""
    edge = 1
    while -(-h // edge) * -(-w // edge) > most:
        edge += 1
    coarse = rs.randint(0, top, size=(-(-h // edge), -(-w // edge)))
    return np.repeat(np.repeat(coarse, edge, axis=0), edge, axis=1)[:h, :w].astype(np.int64)


def _layout(rs, kind, h, w):
    """(objects, cells) as int64 planes of small non-negative values."""
    if kind == "discs":
        objects, cells = mmr.random_masks_windowed(rs, h, w, min(150, max(2, h * w // 60)), min(40, max(1, h * w // 400)))
        return objects.astype(np.int64), cells.astype(np.int64)
    if kind == "dense":
        # every pixel drawn on its own inside a patch (across a tile corner where the image has one), blocks elsewhere
        objects, cells = _blocks(rs, h, w, 4, 100), _blocks(rs, h, w, 5, 110)
        ph, pw = min(h, 10), min(w, 10)
        y0 = min(max(T - ph // 2, 0), h - ph) if h > T else int(rs.randint(0, h - ph + 1))
        x0 = min(max(T - pw // 2, 0), w - pw) if w > T else int(rs.randint(0, w - pw + 1))
        objects[y0:y0 + ph, x0:x0 + pw] = rs.randint(0, 4, size=(ph, pw))
        cells[y0:y0 + ph, x0:x0 + pw] = rs.randint(0, 5, size=(ph, pw))
        return objects, cells
    yy, xx = np.mgrid[:h, :w]
    if kind == "stripes":
        # cells: vertical stripes whose borders lie on a tile edge or one pixel beside it; objects: horizontal ones of
        # half the width, every third a gap
        off_c, off_o = int(rs.randint(-1, 2)), int(rs.randint(-1, 2))
        cells = ((xx + off_c + T) // T) % 2 + 1
        objects = ((yy + off_o + T) // (T // 2)) % 3
        if h < T // 2:                                     # a low image: the objects cut the stripes along x instead
            objects = ((xx + off_o + T) // 24) % 3
        cells[yy % 37 == 36] = 0                           # the stripes cut into lengths that the object stripes cover
        objects[xx % 90 == 89] = 0                         # in part, in full or not at all
        return objects.astype(np.int64), cells.astype(np.int64)
    assert kind == "pieces"
    cells = np.zeros((h, w), dtype=np.int64)               # one value in several separate places
    values = min(40, max(2, h * w // 50))
    for _ in range(3 * values):
        y, x = int(rs.randint(h)), int(rs.randint(w))
        cells[y:y + rs.randint(1, 7), x:x + rs.randint(1, 7)] = rs.randint(1, values + 1)
    objects = np.zeros((h, w), dtype=np.int64)
    for i in range(min(30, max(1, h * w // 300))):
        y, x = int(rs.randint(h)), int(rs.randint(w))
        objects[y:y + rs.randint(2, 25), x:x + rs.randint(2, 25)] = i // 2 + 1     # an object value twice, too
    return objects, cells


def _as_dtype(plane, name):
    """The plane in the mask dtype, 0 kept and distinct values kept distinct; uint32 and int64 values lie past int32."""
    if name == "uint32":
        return np.where(plane != 0, plane + 2 ** 31 + 5, 0).astype(np.uint32)
    if name == "int64":
        return np.where(plane % 2 == 1, -plane, plane) * (2 ** 33 + 1)
    return plane.astype(name)


def reference_pairs(objects, cells, grow):
    """The statement's candidate list: rows (object, cell, overlap, cell area, centroid inside the grown box)."""
    ol, n_o, _ = mmr.label_regions(objects, 2)
    cl, n_c, areas = mmr.label_regions(cells, 2)
    pairs = mmr.pair_overlaps(ol, cl)
    if not len(pairs):
        return np.zeros((0, 5), dtype=np.int64)
    _, _, boxes = mmr.region_tables(ol, n_o)
    count, sums, _ = mmr.region_tables(cl, n_c)
    cy, cx = sums[:, 0] / count.astype(np.float64), sums[:, 1] / count.astype(np.float64)
    o, c = pairs[:, 0].astype(np.int64) - 1, pairs[:, 1].astype(np.int64) - 1
    inside = (cy[c] >= boxes[o, 0] - grow) & (cy[c] <= boxes[o, 1] + grow) & (cx[c] >= boxes[o, 2] - grow) & \
        (cx[c] <= boxes[o, 3] + grow)
    return np.stack([pairs[:, 0], pairs[:, 1], pairs[:, 2], areas[pairs[:, 1]], inside], axis=1).astype(np.int64)


def _tie_threshold(objects, cells, grow):
    """An overlap_thresh on which one pair of the statement's list lies exactly, and which the statement tells from its
    neighbour: ``>=`` merges that pair, ``>`` does not.  None if the masks hold no such pair."""
    rows = reference_pairs(objects, cells, grow)
    rows = rows[(rows[:, 4] != 0) & (rows[:, 2] < rows[:, 3])]
    if not len(rows):
        return None
    best = np.zeros(int(rows[:, 0].max()) + 1, dtype=np.int64)
    np.maximum.at(best, rows[:, 0], rows[:, 2])
    rows = rows[rows[:, 2] == best[rows[:, 0]]]             # the pairs an object would choose were they all eligible
    rows = rows[np.argsort(rows[:, 2] / rows[:, 3], kind="stable")][:12].tolist()
    plain = mmr.label_regions(cells, 2)[0]
    for merging in (True, False):                          # first a threshold under which other pairs still merge
        tried = set()
        for obj, cell, ov, area, _ in rows:
            thresh = 100 * ov // area if 100 * ov % area == 0 else 100.0 * ov / area
            if thresh in tried or ov / area != thresh / 100:
                continue
            tried.add(thresh)
            strict, loose = (mmr.merge_masks(objects, cells, thresh, grow, compare=c) for c in (STRICT, LOOSE))
            if not np.array_equal(strict[1], loose[1]) and (not merging or not np.array_equal(strict[1], plain)):
                return thresh
    return None


def gen_case(i, seed=SEED):
    size, dtype, layout, thresh_kind, grow_kind = CLASSES[i % R]
    for attempt in range(16):                              # (a tie case draws again until its masks hold a tie)
        rs = np.random.RandomState((seed + 104729 * i + 7919 * attempt) % (2 ** 32))
        if size == "wide":
            h, w = int(rs.randint(1, 4)), int(rs.randint(300, 5001))
            h, w = (h, w) if rs.randint(2) else (w, h)
        else:
            lo, hi = {"small": (1, 20), "tile": (40, 70), "tiles": (65, 200)}[size]
            h, w = int(rs.randint(lo, hi + 1)), int(rs.randint(lo, hi + 1))
        objects, cells = (_as_dtype(p, dtype) for p in _layout(rs, layout, h, w))
        grow = {"zero": 0, "three": 3, "huge": max(h, w) + 5}[grow_kind]
        thresh = {"zero": 0, "middle": [10, 25, 33.3, 50][rs.randint(4)], "hundred": 100, "tie": None}[thresh_kind]
        if thresh_kind == "tie":
            thresh = _tie_threshold(objects, cells, grow)
            if thresh is None:
                continue
        table = int(rs.randint(1, 60))                     # merge_apply: tables of any length, labels outside them
        winner = (rs.randint(0, 3, size=table) * rs.randint(1, 5000, size=table)).astype(np.int32)
        removed = ((rs.rand(table) < 0.5) * rs.randint(1, 9, size=table)).astype(np.int32)
        return dict(objects=objects, cells=cells, thresh=thresh, grow=grow, winner=winner, removed=removed, cls=CLASSES[i % R])
    raise AssertionError("case %d: no tie in 16 draws of %r" % (i, CLASSES[i % R]))


def reference_outcome(c):
    """(cells merged, candidate pairs refused) by the statement for a case."""
    rows = reference_pairs(c["objects"], c["cells"], c["grow"])
    refused = int(((rows[:, 4] == 0) | ~(rows[:, 2] / np.maximum(rows[:, 3], 1) > c["thresh"] / 100)).sum())
    _, remaining = mmr.merge_masks(c["objects"], c["cells"], c["thresh"], c["grow"])
    n_c = mmr.label_regions(c["cells"], 2)[1]
    return n_c - (len(np.unique(remaining[remaining != 0]))), refused


def test_classes_cover_every_value():
    for pos, values in enumerate((SIZES, DTYPES, LAYOUTS, THRESHOLDS, GROWS)):
        assert {c[pos] for c in CLASSES} == set(values)
    assert CASES >= max(12, R)
    from ark_analysis_amd import _capi
    assert "pxsom_label_regions" in _capi.SYMBOLS and "pxsom_pair_overlaps" in _capi.SYMBOLS and \
        "pxsom_merge_apply" in _capi.SYMBOLS


def test_generator_meets_its_conditions():
    """Without a device: the default run exercises the choice (at least half its cases merge a cell and refuse a
    candidate), every tie case holds a pair on its threshold that ``>=`` decides differently, the dtypes carry what they
    are there for, and the statement stays cheap."""
    both = 0
    for i in range(max(12, R)):
        c = gen_case(i, DEFAULT_SEED)                      # (the conditions are those of the default run)
        size, dtype, layout, thresh_kind, grow_kind = c["cls"]
        again = gen_case(i, DEFAULT_SEED)
        assert all(np.array_equal(c[k], again[k]) for k in ("objects", "cells", "winner", "removed")) and c["thresh"] == again["thresh"]
        assert c["objects"].dtype == np.dtype(dtype) and c["cells"].dtype == np.dtype(dtype) and c["objects"].shape == c["cells"].shape
        h, w = c["cells"].shape
        assert {"small": max(h, w) <= 20, "tile": 40 <= min(h, w) and max(h, w) <= 70, "tiles": 65 <= min(h, w) and max(h, w) <= 200,
                "wide": min(h, w) <= 3 and 300 <= max(h, w) <= 5000}[size]
        if dtype in ("uint32", "int64"):
            assert max(np.abs(c["cells"].astype(np.float64)).max(), np.abs(c["objects"].astype(np.float64)).max()) > 2 ** 31
        n_o, n_c = mmr.label_regions(c["objects"], 2)[1], mmr.label_regions(c["cells"], 2)[1]
        assert n_o * n_c <= 40000, (i, n_o, n_c)
        if layout == "pieces" and size != "small":
            assert n_c > len(np.unique(c["cells"])) - 1          # one value in several regions
        merged, refused = reference_outcome(c)
        both += merged > 0 and refused > 0
        if thresh_kind == "tie":
            rows = reference_pairs(c["objects"], c["cells"], c["grow"])
            assert ((rows[:, 2] / rows[:, 3] == c["thresh"] / 100) & (rows[:, 4] != 0)).any(), i
            strict, loose = (mmr.merge_masks(c["objects"], c["cells"], c["thresh"], c["grow"], compare=k) for k in (STRICT, LOOSE))
            assert not np.array_equal(strict[1], loose[1]), i    # >= merges a cell that > leaves
        if thresh_kind == "hundred":
            assert merged == 0
    assert 2 * both >= max(12, R), both


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(CASES))
def test_fuzz_merge_masks(gpu, i):
    import torch
    from ark_analysis_amd import som_device
    c = gen_case(i)
    what = repr((i, c["cls"], c["cells"].shape, c["thresh"], c["grow"]))
    relabelled = []
    for plane in (c["objects"], c["cells"]):
        for connectivity in (1, 2):
            labels, n, areas = som_device.label_regions(torch.from_numpy(plane).to(gpu), connectivity)
            want_labels, want_n, want_areas = mmr.label_regions(plane, connectivity)
            n = int(n.item())
            assert n == want_n, what
            assert np.array_equal(labels.cpu().numpy(), want_labels), what
            areas = areas.cpu().numpy()
            assert np.array_equal(areas[:n + 1], want_areas) and not areas[n + 1:].any(), what
        relabelled.append(want_labels)                     # (connectivity 2, the statement's)
    a, b = relabelled
    at, bt = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    assert np.array_equal(som_device.pair_overlaps(at, bt).cpu().numpy(), mmr.pair_overlaps(a, b)), what
    table = len(c["winner"])
    inside = b < table                                     # (labels are >= 0)
    safe = np.where(inside, b, 0)
    merged, remaining = som_device.merge_apply(at, bt, torch.from_numpy(c["winner"]).to(gpu), torch.from_numpy(c["removed"]).to(gpu))
    assert np.array_equal(merged.cpu().numpy(), np.where(inside & (c["winner"][safe] != 0), c["winner"][safe], a)), what
    assert np.array_equal(remaining.cpu().numpy(), np.where(inside & (c["removed"][safe] != 0), 0, b)), what
    got = som_device.merge_masks(torch.from_numpy(c["objects"]).to(gpu), torch.from_numpy(c["cells"]).to(gpu), c["thresh"], c["grow"])
    want = mmr.merge_masks(c["objects"], c["cells"], c["thresh"], c["grow"])
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]), what
