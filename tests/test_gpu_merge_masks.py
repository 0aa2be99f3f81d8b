"""pxsom_pair_overlaps, pxsom_merge_apply and the chain som_device.merge_masks on the GPU against the numpy + scipy
statement of tests/merge_masks_reference.py, every pixel and every row compared exactly; and the mirror
merge_masks_seq on the device against the statement chained on the host."""
import json
import os

import numpy as np
import pytest
import torch

from tests import merge_masks_reference as mmr
from tests import test_merge_masks as cpu

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 130), (63, 65), (64, 64), (65, 129), (130, 130)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _strided(gpu, plane, pad, fill):
    h, w = plane.shape
    padded = np.full((h + 2, w + pad), fill, dtype=plane.dtype)
    padded[1:h + 1, 1:w + 1] = plane
    return torch.from_numpy(padded).to(gpu)[1:h + 1, 1:w + 1]


def _pairs(gpu, a, b, **kw):
    from ark_analysis_amd import som_device
    got = som_device.pair_overlaps(_strided(gpu, a, 4, 5), _strided(gpu, b, 7, 6), **kw)
    assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 3
    return got.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_pair_overlaps_equals_unique(gpu, shape):
    h, w = shape
    rs = np.random.RandomState(h * 131 + w)
    zero, ones = np.zeros(shape, np.int32), np.ones(shape, np.int32)
    every = np.arange(1, h * w + 1, dtype=np.int32).reshape(shape)               # the pair changes at every pixel
    planes = [(zero, ones), (ones, zero), (ones * 3, ones * 9), (every, every[::-1, ::-1].copy()),
              (rs.randint(0, 4, size=shape).astype(np.int32), rs.randint(0, 5, size=shape).astype(np.int32)),
              (np.repeat(rs.randint(0, 30, size=(h, (w + 6) // 7)), 7, axis=1)[:, :w].astype(np.int32),
               np.repeat(rs.randint(0, 50, size=((h + 4) // 5, w)), 5, axis=0)[:h].astype(np.int32)),
              (rs.randint(-5, 2 ** 31 - 1, size=shape).astype(np.int32), ones)]
    for i, (a, b) in enumerate(planes):
        want = mmr.pair_overlaps(a, b)
        got = _pairs(gpu, a, b)
        assert np.array_equal(got, want), (shape, i)
        assert np.array_equal(_pairs(gpu, a, b), got), (shape, i, "second run")
    a, b = planes[4]
    assert np.array_equal(_pairs(gpu, a, b, n_a=2, n_b=3), mmr.pair_overlaps(a, b, 2, 3))
    assert len(_pairs(gpu, a, b, n_a=0, n_b=3)) == 0


def test_pair_overlaps_c_entry_between_sentinels(gpu):
    """Labels outside 1 .. n are counted nowhere and index nothing; rows past the count and the words around the list
    stay as they were; a capacity below the runs writes nothing and says -1."""
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    h, w = 65, 129
    rs = np.random.RandomState(3)
    a = rs.randint(-4, 9, size=(h, w)).astype(np.int32)
    b = rs.randint(-4, 12, size=(h, w)).astype(np.int32)
    a[5, 7], b[5, 7], a[9, 9], b[60, 100] = 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1
    at, bt = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    want = mmr.pair_overlaps(a, b, 6, 8)
    n = torch.full((4,), -7, dtype=torch.int32, device=gpu)

    def call(pairs, capacity, ws, wsb, n_a=6, n_b=8, hh=h, lda=w):
        return lib.pxsom_pair_overlaps(at.data_ptr(), lda, bt.data_ptr(), w, hh, w, n_a, n_b, pairs, capacity,
                                       n[1:].data_ptr(), ws, wsb, _capi.stream_ptr())
    assert call(None, 0, None, 0) == 0
    runs = int(n[2].item())
    assert n.tolist()[0] == -7 and n.tolist()[3] == -7 and int(n[1].item()) == 0 and len(want) <= runs <= h * w
    for capacity in (runs, runs + 100, runs - 1):
        wsb = lib.pxsom_pair_overlaps_workspace_bytes(capacity)
        ws = torch.full((wsb + 512,), 0x5A, dtype=torch.uint8, device=gpu)
        pairs = torch.full((capacity + 2, 3), -7, dtype=torch.int32, device=gpu)
        assert call(pairs[1:].data_ptr(), capacity, ws[256:].data_ptr(), wsb) == 0
        torch.cuda.synchronize()
        got, count = pairs.cpu().numpy(), int(n[1].item())
        assert (ws[:256] == 0x5A).all() and (ws[256 + wsb:] == 0x5A).all()
        if capacity < runs:
            assert count == -1 and (got == -7).all()
        else:
            assert count == len(want) and np.array_equal(got[1:1 + count], want)
            assert (got[0] == -7).all() and (got[1 + count:] == -7).all()
    wsb = lib.pxsom_pair_overlaps_workspace_bytes(runs)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=gpu)
    pairs = torch.zeros((runs, 3), dtype=torch.int32, device=gpu)
    for bad in (dict(hh=0), dict(lda=w - 1), dict(n_a=-1), dict(n_b=-1)):
        assert call(pairs.data_ptr(), runs, ws.data_ptr(), wsb, **bad) == -1, bad
    assert call(pairs.data_ptr(), 0, ws.data_ptr(), wsb) == -1
    assert call(pairs.data_ptr(), (1 << 27) + 1, ws.data_ptr(), wsb) == -1
    assert b"134217728" in lib.pxsom_last_error()                       # the limit is in the message
    assert call(pairs.data_ptr(), runs, ws.data_ptr(), wsb - 1) == -1
    assert call(pairs.data_ptr(), runs, None, wsb) == -1
    assert lib.pxsom_pair_overlaps_workspace_bytes(0) == 0 and lib.pxsom_pair_overlaps_workspace_bytes((1 << 27) + 1) == 0


def test_merge_apply_tables_and_strides(gpu):
    from ark_analysis_amd import _capi, som_device
    rs = np.random.RandomState(11)
    h, w = 65, 129
    a = rs.randint(0, 9, size=(h, w)).astype(np.int32)
    b = rs.randint(-2, 14, size=(h, w)).astype(np.int32)           # -2, -1, 12 and 13 lie outside the tables
    winner = rs.randint(0, 3, size=12).astype(np.int32) * 50
    removed = (rs.rand(12) < 0.5).astype(np.int32)
    inside = (b >= 0) & (b < 12)
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
    lib = _capi.lib()
    assert lib.pxsom_merge_apply(None, w, None, w, h, w, None, None, 12, None, w, None, w, None) == -1
    t = torch.zeros((4, 4), dtype=torch.int32, device=gpu)
    tab = torch.zeros(4, dtype=torch.int32, device=gpu)
    for bad in (dict(h=0), dict(ld=3), dict(table=0)):
        kw = dict(h=4, ld=4, table=4)
        kw.update(bad)
        assert lib.pxsom_merge_apply(t.data_ptr(), kw["ld"], t.data_ptr(), 4, kw["h"], 4, tab.data_ptr(), tab.data_ptr(),
                                     kw["table"], t.data_ptr(), 4, t.data_ptr(), 4, _capi.stream_ptr()) == -1, bad


def _merge(gpu, objects, cells, thresh, grow):
    from ark_analysis_amd import som_device
    merged, remaining = som_device.merge_masks(torch.from_numpy(np.ascontiguousarray(objects)).to(gpu),
                                               torch.from_numpy(np.ascontiguousarray(cells)).to(gpu), thresh, grow)
    assert merged.dtype == torch.int32 and remaining.dtype == torch.int32
    return merged.cpu().numpy(), remaining.cpu().numpy()


def test_merge_masks_equals_the_fixtures(gpu):
    g22 = np.load(os.path.join(GOLDEN, "g22_merge_masks.npz"))
    for c in json.loads(str(g22["cases"])):
        name = c["name"]
        objects, cells = g22["objects_" + name], g22["cells_" + name]
        if objects.dtype.kind == "f":
            objects, cells = objects.astype(np.int32), cells.astype(np.int32)
        merged, remaining = _merge(gpu, objects, cells, c["overlap_thresh"], c["expansion_factor"])
        assert np.array_equal(merged, g22["merged_" + name]) and np.array_equal(remaining, g22["remaining_" + name]), name


@pytest.mark.parametrize("name", sorted(cpu.quirks()))
def test_merge_masks_hand_built_cases(gpu, name):
    objects, cells, thresh, grow = cpu.quirks()[name]
    want = mmr.merge_masks(objects, cells, thresh, grow)
    got = _merge(gpu, objects, cells, thresh, grow)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


def test_merge_masks_shape_mismatch(gpu):
    with pytest.raises(ValueError, match="Both masks must have the same shape"):
        _merge(gpu, np.zeros((4, 5), np.int32), np.zeros((5, 4), np.int32), 10, 0)


@pytest.mark.parametrize("shape", [(63, 65), (65, 129), (130, 130)])
def test_merge_masks_random(gpu, shape):
    rs = np.random.RandomState(shape[0] + shape[1])
    for thresh, grow in ((0, 3), (25, 0), (60, 20)):
        objects, cells = mmr.random_masks(rs, shape[0], shape[1], shape[0] * shape[1] // 60, shape[0] * shape[1] // 400)
        want = mmr.merge_masks(objects, cells, thresh, grow)
        got = _merge(gpu, objects, cells, thresh, grow)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (shape, thresh, grow)
        assert (want[0] != mmr.label_regions(objects, 2)[0]).any() or thresh == 60
    dense = rs.randint(0, 4, size=(33, 70)).astype(np.int32), rs.randint(0, 5, size=(33, 70)).astype(np.int32)
    want = mmr.merge_masks(dense[0], dense[1], 10, 2)
    got = _merge(gpu, dense[0], dense[1], 10, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), shape


def test_merge_masks_seq_on_the_device(gpu, tmp_path, capsys):
    from ark_analysis_amd.segmentation.ez_seg import merge_masks as mm
    cpu.run_merge_masks_seq(mm, tmp_path, capsys)


def test_renumber_masks_on_the_device(gpu, tmp_path):
    from ark_analysis_amd import image_io
    from ark_analysis_amd.segmentation.ez_seg import ez_seg_utils
    from tests.test_ez_seg_host_mirrors import literal_renumber
    rs = np.random.RandomState(2)
    images = {}
    for name, dtype in (("a.tiff", np.int32), ("b.tiff", np.uint16), ("c.tiff", np.uint8)):
        image_io.write_image(str(tmp_path / name), rs.randint(0, 9, size=(65, 70)).astype(dtype))
    image_io.write_image(str(tmp_path / "d.tiff"), np.array([[1, 30, 0], [30, 1, 0]], dtype=np.int16))   # 30 is handed out
    for path in tmp_path.rglob("*.tiff"):
        images[path.name] = image_io.read_image(str(path))
    want = literal_renumber(images)
    ez_seg_utils.renumber_masks(str(tmp_path))
    for name, before in images.items():
        got = image_io.read_image(str(tmp_path / name))
        assert got.dtype == before.dtype and np.array_equal(got, want[name]), name
