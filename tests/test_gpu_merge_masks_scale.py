"""pxsom_pair_overlaps, pxsom_merge_apply and the chain som_device.merge_masks at the size of a real field of view (the
"cap" shape of test_gpu_label_scale.py: more pixels than one trip of a grid-stride loop covers), against the numpy + scipy
statement of tests/merge_masks_reference.py; every comparison is exact.  The small-shape tests stop at 130 x 130: a pair
table of 2^16 slots, one trip through merge_apply_kernel, bitonic_step_kernel and emit_pairs_kernel."""
import functools

import numpy as np
import pytest
import torch

from tests import merge_masks_reference as mmr
from tests.test_gpu_label_scale import cap_shape
from tests.test_gpu_merge_masks import _merge, _pairs, _strided

pytestmark = pytest.mark.gpu


def _grid_cap():
    return torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256     # flat_grid of csrc/pxsom_plane.h


def _every():
    h, w = cap_shape()
    every = np.arange(1, h * w + 1, dtype=np.int32).reshape(h, w)       # the pair changes at every pixel
    return every, every[::-1, ::-1].copy()


@functools.lru_cache(maxsize=None)
def _discs(seed):
    h, w = cap_shape()
    return mmr.random_masks_windowed(np.random.RandomState(seed), h, w, 400, 60, cell_r=(6, 14), object_r=(10, 30))


def _planes(kind):
    h, w = cap_shape()
    if kind == "every":
        return _every()
    if kind == "dense":
        rs = np.random.RandomState(4)
        masks = rs.randint(0, 4, size=(h, w)).astype(np.int32), rs.randint(0, 5, size=(h, w)).astype(np.int32)
    else:
        masks = _discs(0)
    return tuple(mmr.label_regions(m, 2)[0] for m in masks)


def _slots(capacity):
    slots = 64
    while slots < 2 * capacity:
        slots *= 2
    return slots


@pytest.mark.parametrize("kind", ["every", "dense", "discs"])
def test_pair_overlaps(gpu, kind):
    from ark_analysis_amd import _capi
    h, w = cap_shape()
    a, b = _planes(kind)
    want = mmr.pair_overlaps(a, b)
    if kind == "every":
        # runs = H W: the table and the sort are as large as this image can make them, and a step of the sort covers
        # more pairs of slots than one trip of its grid; through the entry itself, so that the test cannot go quiet
        lib = _capi.lib()
        n = torch.zeros(2, dtype=torch.int32, device=gpu)
        at, bt = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
        assert lib.pxsom_pair_overlaps(at.data_ptr(), w, bt.data_ptr(), w, h, w, 2 ** 31 - 1, 2 ** 31 - 1, None, 0,
                                       n.data_ptr(), None, 0, _capi.stream_ptr()) == 0
        assert int(n[1].item()) == h * w == len(want)
        slots = _slots(h * w)
        assert lib.pxsom_pair_overlaps_workspace_bytes(h * w) == slots * 12
        assert slots >= 1 << 22 and slots // 2 > _grid_cap() and h * w > _grid_cap()
    if kind == "dense":
        assert len(want) > 100000
    if kind == "discs":
        assert 30 <= len(want) < 2000
    got = _pairs(gpu, a, b)
    assert np.array_equal(got, want)
    assert _pairs(gpu, a, b).tobytes() == got.tobytes(), "second run"


def test_pair_overlaps_capacity_one_below_the_runs(gpu):
    """Through the C entry: a list one row too short for the runs says -1 and stays untouched."""
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    h, w = cap_shape()
    a, b = _every()
    at, bt = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    capacity = h * w - 1
    wsb = lib.pxsom_pair_overlaps_workspace_bytes(capacity)
    ws = torch.empty(wsb, dtype=torch.uint8, device=gpu)
    pairs = torch.full((capacity + 2, 3), -7, dtype=torch.int32, device=gpu)
    n = torch.full((4,), -7, dtype=torch.int32, device=gpu)
    assert lib.pxsom_pair_overlaps(at.data_ptr(), w, bt.data_ptr(), w, h, w, h * w, h * w, pairs[1:].data_ptr(), capacity,
                                   n[1:].data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [-7, -1, h * w, -7]
    assert bool((pairs == -7).all())


def test_merge_apply_tables_shorter_than_the_labels(gpu):
    from ark_analysis_amd import som_device
    h, w = cap_shape()
    rs = np.random.RandomState(11)
    a = rs.randint(0, 900, size=(h, w)).astype(np.int32)
    b = rs.randint(-2, 1400, size=(h, w)).astype(np.int32)          # -2, -1 and 1200 .. 1399 lie outside the tables
    b[h - 1, w - 1], b[0, 0], b[h // 2, 3] = 2 ** 31 - 1, -2 ** 31, 1200
    table = 1200
    winner = (rs.randint(0, 3, size=table) * rs.randint(1, 5000, size=table)).astype(np.int32)
    removed = (rs.rand(table) < 0.5).astype(np.int32) * rs.randint(1, 9, size=table).astype(np.int32)
    inside = (b >= 0) & (b < table)
    safe = np.where(inside, b, 0)
    want_merged = np.where(inside & (winner[safe] != 0), winner[safe], a)
    want_remaining = np.where(inside & (removed[safe] != 0), 0, b)
    bufs = [torch.full((h + 2, w + 3 + i), -7, dtype=torch.int32, device=gpu) for i in range(2)]
    merged, remaining = som_device.merge_apply(_strided(gpu, a, 4, 5), _strided(gpu, b, 9, 6), torch.from_numpy(winner).to(gpu),
                                               torch.from_numpy(removed).to(gpu), merged=bufs[0][1:h + 1, 2:w + 2],
                                               remaining=bufs[1][1:h + 1, 2:w + 2])
    assert np.array_equal(merged.cpu().numpy(), want_merged) and np.array_equal(remaining.cpu().numpy(), want_remaining)
    for buf in bufs:
        whole = buf.cpu().numpy()
        whole[1:h + 1, 2:w + 2] = -7
        assert (whole == -7).all()


@pytest.mark.parametrize("thresh,grow", [(0, 3), (25, 0), (60, 20)])
def test_merge_masks(gpu, thresh, grow):
    """60 objects and 400 cells that span several tiles each (the statement loops objects x cells in Python)."""
    objects, cells = _discs(thresh + grow)
    want = mmr.merge_masks(objects, cells, thresh, grow)
    n_cells = mmr.label_regions(cells, 2)[1]
    left = len(np.unique(want[1])) - 1
    assert 0 < left < n_cells, "the statement merges no cell, or every cell"
    got = _merge(gpu, objects, cells, thresh, grow)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
