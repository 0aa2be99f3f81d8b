"""pxsom_label_regions on the GPU (som_device.label_regions) against the scipy statement of
tests/merge_masks_reference.py: exact equality of labels, count and areas for connectivity 1 and 2, read through a row
stride wider than the image and written into a slice of a sentinel buffer.  The shapes sit around the kernel's tile edge
(64); the patterns put borders between values on tile edges and one pixel either side."""
import numpy as np
import pytest
import torch

from tests import merge_masks_reference as mmr
from tests import object_mask_reference as omr

pytestmark = pytest.mark.gpu

SENTINEL = -77
SHAPES = [(1, 1), (1, 130), (63, 65), (64, 64), (65, 129), (130, 130)]
T = 64


def _device(gpu, seg, connectivity):
    """labels, n, areas of one call: the plane read from a wider buffer at an offset, the labels written into a slice."""
    from ark_analysis_amd import som_device
    h, w = seg.shape
    padded = np.full((h + 2, w + 5), 3, dtype=seg.dtype)
    padded[1:h + 1, 2:w + 2] = seg
    src = torch.from_numpy(padded).to(gpu)
    buf = torch.full((h + 3, w + 9), SENTINEL, dtype=torch.int32, device=gpu)
    out = buf[2:h + 2, 4:w + 4]
    labels, n, areas = som_device.label_regions(src[1:h + 1, 2:w + 2], connectivity, out=out)
    torch.cuda.synchronize()
    assert labels.data_ptr() == out.data_ptr()
    whole = buf.cpu().numpy()
    inner = whole[2:h + 2, 4:w + 4].copy()
    whole[2:h + 2, 4:w + 4] = SENTINEL
    assert (whole == SENTINEL).all(), "labels written outside the slice"
    return inner, int(n.item()), areas.cpu().numpy()


def _check(gpu, seg, what, connectivities=(1, 2)):
    h, w = seg.shape
    counts = {}
    for connectivity in connectivities:
        labels, n, areas = _device(gpu, seg, connectivity)
        want_labels, want_n, want_areas = mmr.label_regions(seg, connectivity)
        tag = "%s %dx%d %s connectivity %d" % (what, h, w, seg.dtype, connectivity)
        assert n == want_n, tag
        assert np.array_equal(labels, want_labels), tag
        assert areas.size == h * w + 1, tag
        assert np.array_equal(areas[:n + 1], want_areas), tag
        assert not areas[n + 1:].any() and int(areas.sum()) == h * w, tag
        counts[connectivity] = n
    return counts


@pytest.mark.parametrize("shape", SHAPES)
def test_one_value_equals_label_components(gpu, shape):
    from ark_analysis_amd import som_device
    rs = np.random.RandomState(shape[0] * 1000 + shape[1])
    mask = (rs.rand(*shape) < 0.55).astype(np.uint8)
    for connectivity in (1, 2):
        want = som_device.label_components(torch.from_numpy(mask).to(gpu), connectivity)
        for value, dtype in ((1, np.uint8), (-9, np.int32), (70000, np.int64)):
            got = som_device.label_regions(torch.from_numpy((mask.astype(dtype) * value)).to(gpu), connectivity,
                                           capacity=want[2].numel())
            for g, w_ in zip(got, want):
                assert torch.equal(g, w_), (shape, connectivity, value)
    _check(gpu, mask, "one value")


@pytest.mark.parametrize("shape", SHAPES)
def test_two_value_checkerboard(gpu, shape):
    h, w = shape
    board = (omr.checkerboard(h, w).astype(np.int32) + 1) * 5           # values 5 and 10, no zero
    counts = _check(gpu, board, "checkerboard")
    assert counts[1] == h * w                                           # every pixel its own region: the capacity bound
    assert counts[2] == (2 if h > 1 and w > 1 else h * w)


@pytest.mark.parametrize("shape", SHAPES)
def test_stripes_on_and_beside_tile_edges(gpu, shape):
    """Stripes of alternating values whose borders fall on a tile edge and one pixel either side; and one value on both
    sides of every tile edge."""
    h, w = shape
    yy, xx = np.mgrid[:h, :w]
    for offset in (-1, 0, 1):
        for axis, name in ((xx, "vertical"), (yy, "horizontal")):
            for width in (T, 32, 1):
                stripes = (((axis + offset + T) // width) % 2 + 1).astype(np.int32)
                counts = _check(gpu, stripes, "%s stripes %d%+d" % (name, width, offset))
                line = np.arange(w if axis is xx else h)
                assert counts[1] == counts[2] == len(np.unique((line + offset + T) // width))
    same = np.full(shape, 7, dtype=np.uint16)
    assert _check(gpu, same, "one region over every tile edge") == {1: 1, 2: 1}


def test_values_meeting_diagonally_at_a_tile_corner(gpu):
    h, w = 130, 130
    for y, x in ((T, T), (2 * T, T)):
        for s in (1, 5):
            for anti in (False, True):
                for first, second, joined in ((3, 3, True), (3, 4, False)):
                    seg = np.zeros((h, w), dtype=np.int32)
                    if anti:                                  # up-right / down-left
                        seg[y - s:y, x:x + s] = first
                        seg[y:y + s, x - s:x] = second
                    else:                                     # up-left / down-right
                        seg[y - s:y, x - s:x] = first
                        seg[y:y + s, x:x + s] = second
                    counts = _check(gpu, seg, "corner")
                    assert counts[1] == 2 and counts[2] == (1 if joined else 2)
    # a foreign value filling the other two quadrants must not bridge or block the diagonal
    seg = np.full((h, w), 9, dtype=np.int32)
    seg[:T, :T] = seg[T:, T:] = 2
    assert _check(gpu, seg, "quadrants") == {1: 4, 2: 2}
    # diagonal touches of equal and of different values across one vertical and one horizontal edge, off the corners
    seg = np.zeros((h, w), dtype=np.int32)
    seg[10, T - 1] = seg[11, T] = 1
    seg[21, T - 1] = seg[20, T] = 2
    seg[T - 1, 30] = seg[T, 31] = 3
    seg[T - 1, 41] = seg[T, 40] = 4
    seg[50, T - 1], seg[51, T] = 5, 6
    seg[T - 1, 50], seg[T, 51] = 5, 6
    assert _check(gpu, seg, "edge diagonals") == {1: 12, 2: 8}


@pytest.mark.parametrize("pattern", ["spiral", "serpentine"])
def test_long_chains_beside_a_second_value(gpu, pattern):
    for shape in ((65, 129), (130, 130)):
        path = getattr(omr, pattern)(*shape).astype(np.int32)
        seg = np.where(path != 0, 4, 11).astype(np.int32)     # the gaps between the turns hold another value
        _check(gpu, seg, pattern)
        _check(gpu, np.ascontiguousarray(seg.T), pattern + " transposed")


@pytest.mark.parametrize("shape", SHAPES)
def test_random_values(gpu, shape):
    rs = np.random.RandomState(shape[0] * 7 + shape[1])
    _check(gpu, rs.randint(0, 4, size=shape).astype(np.uint8), "randint 4")
    _check(gpu, rs.randint(0, 40, size=shape).astype(np.int16), "randint 40")
    _check(gpu, rs.randint(-3, 3, size=shape).astype(np.int64) * (2 ** 33 + 1), "negative and wide values")
    _check(gpu, rs.randint(0, 3, size=shape).astype(np.uint32) * np.uint32(2 ** 31 + 5), "uint32 past int32")


def test_two_runs_give_equal_bits(gpu):
    seg = np.random.RandomState(7).randint(0, 3, size=(130, 130)).astype(np.int32)
    for connectivity in (1, 2):
        a = _device(gpu, seg, connectivity)
        b = _device(gpu, seg, connectivity)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_arguments_are_checked_before_any_launch(gpu):
    from ark_analysis_amd import _capi, som_device
    lib = _capi.lib()
    seg = torch.zeros((4, 4), dtype=torch.int32, device=gpu)
    labels = torch.zeros((4, 4), dtype=torch.int32, device=gpu)
    n = torch.zeros(1, dtype=torch.int32, device=gpu)
    areas = torch.zeros(17, dtype=torch.int32, device=gpu)
    wsb = lib.pxsom_label_regions_workspace_bytes(4, 4)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=gpu)
    code = som_device.SEG_DTYPES[torch.int32]

    def call(h=4, w=4, ld=4, conn=1, ldo=4, cap=17, bytes_=wsb, segp=seg.data_ptr(), dtype=code):
        return lib.pxsom_label_regions(segp, dtype, h, w, ld, conn, labels.data_ptr(), ldo, n.data_ptr(), areas.data_ptr(), cap,
                                       ws.data_ptr(), bytes_, _capi.stream_ptr())
    assert call() == 0
    for bad in (dict(h=0), dict(ld=3), dict(ldo=3), dict(conn=3), dict(conn=0), dict(cap=0), dict(bytes_=wsb - 1),
                dict(segp=None), dict(dtype=99), dict(dtype=-1)):
        assert call(**bad) == -1, bad
    assert call(h=1 << 16, w=1 << 16, ld=1 << 16, ldo=1 << 16) == -2
    assert lib.pxsom_label_regions_workspace_bytes(1 << 16, 1 << 16) == 0
    with pytest.raises(ValueError):
        som_device.label_regions(seg, 3)
    with pytest.raises(ValueError):
        som_device.label_regions(seg.to(torch.float32), 1)
