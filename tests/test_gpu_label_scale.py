"""pxsom_label_components, pxsom_label_regions, pxsom_components_select and pxsom_binarize_plane at the sizes of a real
field of view, against the scipy statements of tests/object_mask_reference.py and tests/merge_masks_reference.py; every
comparison is exact.  The small-shape tests stop at 130 x 195, where several branches of these kernels never run:

  scan      513 x 512        1026 chunks of 256 pixels: a thread of ccl_scan_kernel owns two counts, some threads none
  boundary  512 x 512        exactly 1024 chunks: one count per thread, every thread used
  ragged    520 x 530        81 tiles: 11 per XCD and 7 idle workgroups in xcd_contiguous
  row       2 x 140 000      2188 tiles side by side, no row edge, 2 x 2187 column-edge pixels
  column    140 000 x 2      the same, transposed
  cap       ~1032 x 1090     more pixels than one trip of a grid-stride loop covers (computed from the device)

The helpers are those of the small-shape tests: the input read through a wider row stride, the labels written into a
slice of a sentinel buffer, the areas summing to H W."""
import functools

import numpy as np
import pytest
import torch

from tests import merge_masks_reference as mmr
from tests import object_mask_reference as omr
from tests import test_gpu_label_components as small_components
from tests import test_gpu_label_regions as small_regions

pytestmark = pytest.mark.gpu

FIXED = {"scan": (513, 512), "boundary": (512, 512), "ragged": (520, 530), "row": (2, 140000), "column": (140000, 2)}
SHAPES = list(FIXED) + ["cap"]
T = 64


@functools.lru_cache(maxsize=None)
def cap_shape():
    """The smallest 1090-wide image with a ragged last tile row that is more than one tile row past the cap of the flat
    grids.  16 and 256 restate flat_grid of csrc/pxsom_plane.h: at most 16 workgroups of 256 threads per CU."""
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256
    w = 1090
    h = -(-cap // w) + 70
    while h % T == 0:
        h += 1
    assert h * w > cap + T * w
    return h, w


def shape_of(name):
    return cap_shape() if name == "cap" else FIXED[name]


def pattern(name, h, w):
    """A 0 / 1 plane of the named pattern; "<name>_t" is the pattern laid out down the columns."""
    if name.endswith("_t"):
        return np.ascontiguousarray(pattern(name[:-2], w, h).T)
    if name == "foreground":
        return np.ones((h, w), np.uint8)
    if name == "background":
        return np.zeros((h, w), np.uint8)
    if name == "random":
        return (np.random.RandomState(h * 31 + w).rand(h, w) < 0.55).astype(np.uint8)
    return getattr(omr, name)(h, w)


# the spiral's generator is a Python loop over its pixels: on the three small shapes only
PATTERNS = [(s, p) for s in SHAPES for p in ("foreground", "background", "checkerboard", "serpentine", "serpentine_t",
                                             "spiral", "nested_rings", "random")
            if p != "spiral" or s in ("scan", "boundary", "ragged")]


@pytest.mark.parametrize("shape,name", PATTERNS)
def test_label_components(gpu, shape, name):
    h, w = shape_of(shape)
    mask = pattern(name, h, w)
    counts = small_components._check(gpu, mask, "%s %s" % (shape, name))
    if name == "foreground":
        assert counts == {(1, False): 1, (2, False): 1, (1, True): 0, (2, True): 0}
    if name == "background":
        assert counts == {(1, False): 0, (2, False): 0, (1, True): 1, (2, True): 1}
    if name == "checkerboard":                            # the capacity bound, met exactly
        assert counts[1, False] == (h * w + 1) // 2 and counts[1, True] == h * w // 2
    if name.startswith("serpentine") or name == "spiral":
        assert counts[1, False] == 1 and counts[2, False] == 1        # one chain through every tile


@pytest.mark.parametrize("shape,name", PATTERNS)
def test_label_regions_of_two_values(gpu, shape, name):
    """The patterns as planes of two values (the checkerboard without a zero: every pixel in a region)."""
    h, w = shape_of(shape)
    mask = pattern(name, h, w)
    if name == "foreground":
        seg = np.full((h, w), 7, dtype=np.uint16)
    elif name == "background":
        seg = np.zeros((h, w), dtype=np.int32)
    elif name == "checkerboard":
        seg = (mask.astype(np.int32) + 1) * 5
    else:
        seg = np.where(mask != 0, 4, 11).astype(np.int32)     # the gaps hold another value
    counts = small_regions._check(gpu, seg, "%s %s" % (shape, name))
    if name == "foreground":
        assert counts == {1: 1, 2: 1}                     # (its area, H W, is compared in _check)
    if name == "background":
        assert counts == {1: 0, 2: 0}
    if name == "checkerboard":
        assert counts[1] == h * w                         # the capacity bound
        assert counts[2] == (2 if h > 1 and w > 1 else h * w)


@pytest.mark.parametrize("kind", ["randint 4 uint8", "randint 40 int16", "wide int64"])
@pytest.mark.parametrize("shape", SHAPES)
def test_label_regions_of_random_values(gpu, shape, kind):
    h, w = shape_of(shape)
    rs = np.random.RandomState(h * 7 + w)
    if kind == "randint 4 uint8":
        seg = rs.randint(0, 4, size=(h, w)).astype(np.uint8)
    elif kind == "randint 40 int16":
        seg = rs.randint(0, 40, size=(h, w)).astype(np.int16)
    else:
        seg = rs.randint(-3, 3, size=(h, w)).astype(np.int64) * (2 ** 33 + 1)
    small_regions._check(gpu, seg, "%s %s" % (shape, kind))


@pytest.mark.parametrize("axis", ["vertical", "horizontal"])
@pytest.mark.parametrize("shape", SHAPES)
def test_label_regions_of_stripes_on_and_beside_tile_edges(gpu, shape, axis):
    h, w = shape_of(shape)
    yy, xx = np.mgrid[:h, :w]
    along = xx if axis == "vertical" else yy
    for offset in (-1, 0, 1):
        stripes = (((along + offset + T) // T) % 2 + 1).astype(np.int32)
        counts = small_regions._check(gpu, stripes, "%s %s stripes %+d" % (shape, axis, offset))
        line = np.arange(w if axis == "vertical" else h)
        assert counts[1] == counts[2] == len(np.unique((line + offset + T) // T))


# ---- selection and binarisation past the grid cap ----------------------------------------------------------------------
def _strided(gpu, plane, pad, fill):
    h, w = plane.shape
    padded = np.full((h + 2, w + pad), fill, dtype=plane.dtype)
    padded[1:h + 1, 1:w + 1] = plane
    return torch.from_numpy(padded).to(gpu)[1:h + 1, 1:w + 1]


def _slice_of(gpu, h, w, dtype, sentinel):
    buf = torch.full((h + 3, w + 9), sentinel, dtype=dtype, device=gpu)
    return buf, buf[2:h + 2, 4:w + 4]


def _inner(buf, h, w, sentinel):
    whole = buf.cpu().numpy()
    inner = whole[2:h + 2, 4:w + 4].copy()
    whole[2:h + 2, 4:w + 4] = sentinel
    assert (whole == sentinel).all(), "written outside the slice"
    return inner


@functools.lru_cache(maxsize=None)
def _select_inputs():
    h, w = cap_shape()
    return (np.random.RandomState(16).rand(h, w) < 0.55).astype(np.uint8)


def test_components_select_fill(gpu):
    """The labels and areas are the reference's own: the pass is checked on its own, not behind the device labeller."""
    from ark_analysis_amd import som_device
    fg = _select_inputs()
    h, w = fg.shape
    holes, n, areas = omr.label_components(fg, 1, invert=True)
    areas_dev = torch.from_numpy(areas.astype(np.int32)).to(gpu)
    for threshold in (0, 2, 5, h * w):
        buf, out = _slice_of(gpu, h, w, torch.uint8, 99)
        got = som_device.components_select(_strided(gpu, holes, 6, -5), areas_dev, "fill", fg=_strided(gpu, fg, 3, 1),
                                           area_threshold=threshold, out=out)
        assert got.data_ptr() == out.data_ptr()
        want = omr.fill_holes(fg, threshold)
        assert np.array_equal(_inner(buf, h, w, 99), want), threshold
    filled = omr.fill_holes(fg, 5)
    assert (filled != fg).any() and not filled.all()      # some holes are below 5 pixels, some are not


def test_components_select_keep(gpu):
    from ark_analysis_amd import som_device
    fg = _select_inputs()
    h, w = fg.shape
    labels, n, areas = omr.label_components(fg, 2)
    areas_dev = torch.from_numpy(areas.astype(np.int32)).to(gpu)
    kept = []
    for lo, hi in ((0, h * w), (2, 6), (3, 3), (7, None)):
        buf, out = _slice_of(gpu, h, w, torch.int32, -77)
        som_device.components_select(_strided(gpu, labels, 6, -5), areas_dev, "keep", min_area=lo, max_area=hi, out=out)
        want = omr.keep_by_area(labels, areas, lo, h * w if hi is None else hi)
        assert np.array_equal(_inner(buf, h, w, -77), want), (lo, hi)
        kept.append(len(np.unique(want)))
    assert len(set(kept)) == len(kept)                    # every range keeps another set


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_binarize_plane(gpu, dtype):
    """The three predicates through the C entry, which takes the row stride of the output.  The plane holds zeros,
    negatives and many values equal to the level."""
    from ark_analysis_amd import _capi, som_device
    lib = _capi.lib()
    h, w = cap_shape()
    rs = np.random.RandomState(5)
    plane = (rs.randint(-3, 20, size=(h, w)) * (rs.rand(h, w) < 0.7)).astype(dtype) * dtype(0.1)
    block = 9
    local = omr.blur(plane, (block - 1) / 6.0, "reflect")
    level = np.percentile(plane[plane != 0], 40)
    assert (plane == dtype(level)).any()
    plane_dev, local_dev = torch.from_numpy(plane).to(gpu), torch.from_numpy(local).to(gpu)
    for mode, thresh in ((som_device.BIN_POSITIVE, None), (som_device.BIN_LEVEL, 40), (som_device.BIN_LOCAL, "auto")):
        buf, out = _slice_of(gpu, h, w, torch.uint8, 99)
        rc = lib.pxsom_binarize_plane(plane_dev.data_ptr(), som_device.PLANE_MODE_DTYPES[plane_dev.dtype], h, w, mode,
                                      float(level), local_dev.data_ptr() if mode == som_device.BIN_LOCAL else None,
                                      out.data_ptr(), out.stride(0), _capi.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        want = omr.foreground(plane, thresh, block).astype(np.uint8)
        assert np.array_equal(_inner(buf, h, w, 99), want), (dtype, mode)
        assert 0 < want.mean() < 1


def test_object_mask_chain(gpu):
    from ark_analysis_amd import som_device
    h, w = cap_shape()
    rs = np.random.RandomState(8)
    img = ((rs.rand(h, w) < 0.03) * rs.gamma(2.0, 20.0, size=(h, w))).astype(np.float32)
    want = omr.object_mask(img, 2, 60, 30, 5, 400)
    got = som_device.object_mask(torch.from_numpy(img).to(gpu), 2, 60, 30, 5, 400)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    kept = len(np.unique(want)) - 1
    assert 100 < kept < len(np.unique(omr.object_mask(img, 2, 60, 30, 0, h * w))) - 1    # objects kept, objects dropped
