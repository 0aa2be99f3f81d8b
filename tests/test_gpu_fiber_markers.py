"""From the ridge map to the watershed's inputs on the GPU (K25): every entry equal to its scipy / numpy statement
(tests/fiber_markers_reference.py) -- the distance transform and its squares over the sizes at which the kernels' cases
differ (fewer rows than column stretches, one and several workgroups per row and per column band, padded rows) and the
patterns that exercise the "no background in this column" value; the histogram against np.histogram with values on the
edges; the Sobel magnitude bit for bit from 1 x 1 up; the markers with values on the thresholds; then the chain against
every g28 case."""
import json
import os

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from tests import fiber_markers_reference as fmr
from tests import test_fiber_markers as tfm

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 33), (64, 65), (65, 64), (33, 130), (5, 1100), (200, 230)]
PADDED = (200, 230)                      # this shape runs on row-padded inputs and outputs inside sentinel-filled buffers
IDS = ["%dx%d" % s for s in SHAPES]


def padded_in(plane, gpu, pad, fill=0):
    """The plane as a view of a wider device buffer."""
    h, w = plane.shape
    buf = torch.full((h, w + pad), fill, dtype=torch.from_numpy(plane[:0]).dtype, device=gpu)
    buf[:, :w] = torch.from_numpy(plane).to(gpu)
    return buf[:, :w]


def sentinel_out(h, w, dtype, gpu, pad, value):
    buf = torch.full((h + 2, w + pad), value, dtype=dtype, device=gpu)
    return buf, buf[1:h + 1, 3:w + 3]


def guard_intact(buf, h, w, value):
    b = buf.cpu().numpy().copy()
    b[1:h + 1, 3:w + 3] = value
    return bool((b == value).all())


# ---- the distance transform -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_edt_equals_scipy(gpu, shape):
    from ark_analysis_amd import som_device
    h, w = shape
    for name, fg in fmr.patterns(h, w).items():
        want = ndi.distance_transform_edt(fg)
        want_sq = np.rint(want * want).astype(np.int32)               # exact: want is the rounded root of an integer
        if h * w <= 33 * 130:
            assert np.array_equal(want_sq, fmr.squared_distances(fg)), name
        if shape == PADDED:
            t = padded_in(fg, gpu, 13, fill=0)
            buf, out = sentinel_out(h, w, torch.float64, gpu, 29, -7.0)
            buf_sq, out_sq = sentinel_out(h, w, torch.int32, gpu, 11, -7)
        else:
            t, out, out_sq = torch.from_numpy(fg).to(gpu), None, None
        got = som_device.distance_transform_edt(t, out=out)
        got_sq = som_device.distance_transform_edt(t, out=out_sq, squared=True)
        assert got.dtype == torch.float64 and got_sq.dtype == torch.int32 and got.shape == got_sq.shape == (h, w)
        assert np.array_equal(got_sq.cpu().numpy(), want_sq), name
        assert np.array_equal(got.cpu().numpy(), want), name
        if name == "all_background":
            assert not want.any()
        if shape == PADDED:
            assert got.data_ptr() == out.data_ptr() and guard_intact(buf, h, w, -7.0) and guard_intact(buf_sq, h, w, -7), name


def test_edt_inputs_and_refusals(gpu):
    from ark_analysis_amd import _capi, som_device
    fg = fmr.patterns(17, 33)["noise_0.97"]
    want = ndi.distance_transform_edt(fg)
    t = torch.from_numpy(fg).to(gpu)
    assert np.array_equal(som_device.distance_transform_edt(t != 0).cpu().numpy(), want)        # a bool plane
    assert np.array_equal(som_device.distance_transform_edt(t * 200).cpu().numpy(), want)       # any non-zero byte
    for shape in ((1, 1), (4, 9), (70, 3)):
        full = torch.ones(shape, dtype=torch.uint8, device=gpu)
        for squared in (False, True):
            with pytest.raises(ValueError, match="no background pixel"):
                som_device.distance_transform_edt(full, squared=squared)
        # the C entry's defined answer for that plane
        assert bool(torch.isinf(som_device.distance_transform_edt(full, check=False)).all())
        assert bool((som_device.distance_transform_edt(full, squared=True, check=False) == 2 ** 31 - 1).all())
    # the size limit: refused before any launch, by the wrapper and by the entry (a [1, 46341] plane is 46 KB)
    long_row = torch.zeros((1, 46341), dtype=torch.uint8, device=gpu)
    with pytest.raises(NotImplementedError, match="beyond int32"):
        som_device.distance_transform_edt(long_row)
    out = torch.zeros((1, 46341), dtype=torch.float64, device=gpu)
    ws = torch.zeros(8, dtype=torch.uint8, device=gpu)
    with pytest.raises(_capi.PxsomError, match="PXSOM_ERR_UNSUPPORTED"):
        _capi.call("pxsom_distance_transform_edt", long_row.data_ptr(), 1, 46341, 46341, out.data_ptr(), 46341, None, 46341,
                   ws.data_ptr(), 8, _capi.stream_ptr())
    assert not bool(out.any())
    assert som_device.distance_transform_edt(long_row[:, :46340]).shape == (1, 46340)           # the largest row taken
    for bad in (t.to(torch.int32), t.cpu(), t[:0], t.t()):
        with pytest.raises(ValueError):
            som_device.distance_transform_edt(bad)
    with pytest.raises(ValueError, match="out must be"):
        som_device.distance_transform_edt(t, out=torch.zeros((17, 33), dtype=torch.float32, device=gpu))


# ---- minimum, maximum and the histogram ---------------------------------------------------------------------------------------
def histogram_planes():
    rs = np.random.RandomState(77)
    edges = np.linspace(-1.25, 3.5, 257)
    on_edges = np.concatenate([edges, (edges[:-1] + edges[1:]) / 2, np.nextafter(edges[1:], -np.inf), [3.5] * 7])
    out = {"on_edges": on_edges.reshape(1, -1), "two_bins": (rs.random_sample((9, 14)) < 0.3).astype(np.float64) * 5.0,
           "constant": np.full((3, 4), 2.5), "one_pixel": np.array([[-3.0]]), "row_5x1100": rs.standard_normal((5, 1100)),
           "negative_zero": np.array([[-0.0, 0.0, 1.0, -1.0]]), "small_range": 1.0 + rs.randint(0, 300, (20, 31)) * 2.0 ** -40,
           "large_200x230": np.abs(rs.standard_normal((200, 230))) * 1e6}
    dist = fmr.blur(ndi.distance_transform_edt(fmr.bars(96, 96, rs, 8)), 1)      # the workload's own distribution
    out["distance_map"] = dist
    return out


@pytest.mark.parametrize("nbins", [256, 1, 7, 1024])
def test_histogram_and_minmax_equal_numpy(gpu, nbins):
    from ark_analysis_amd import som_device
    for name, plane in histogram_planes().items():
        t = padded_in(plane, gpu, 5, fill=9e9) if name in ("large_200x230", "two_bins") else torch.from_numpy(plane).to(gpu)
        lo, hi = som_device.plane_minmax(t)
        assert lo == plane.min() and hi == plane.max(), name
        counts, edges = som_device.plane_histogram(t, nbins)
        want, want_edges = np.histogram(plane, nbins, (plane.min(), plane.max()))
        assert counts.dtype == torch.int64 and counts.shape == (nbins,)
        assert np.array_equal(edges, want_edges), name
        assert np.array_equal(counts.cpu().numpy(), want), name
        assert int(counts.sum().item()) == plane.size
    # a caller's range: what lies outside is counted nowhere
    plane = histogram_planes()["row_5x1100"]
    counts, edges = som_device.plane_histogram(torch.from_numpy(plane).to(gpu), nbins, (-0.5, 1.0))
    want, want_edges = np.histogram(plane, nbins, (-0.5, 1.0))
    assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(edges, want_edges) and want.sum() < plane.size


def test_histogram_refusals(gpu):
    from ark_analysis_amd import som_device
    plane = torch.from_numpy(np.array([[0.0, np.nan], [1.0, 2.0]])).to(gpu)
    with pytest.raises(ValueError, match="NaN"):
        som_device.plane_minmax(plane)
    with pytest.raises(ValueError, match="NaN"):
        som_device.plane_histogram(plane)
    with pytest.raises(ValueError, match="not finite"):
        som_device.plane_histogram(torch.from_numpy(np.array([[0.0, np.inf]])).to(gpu))
    good = torch.zeros((3, 3), dtype=torch.float64, device=gpu)
    for nbins in (0, 1025):
        with pytest.raises(ValueError, match="nbins"):
            som_device.plane_histogram(good, nbins)
    for bad in (good.to(torch.float32), good.cpu(), good[:0], torch.zeros((4, 4), dtype=torch.float64, device=gpu).t()):
        with pytest.raises(ValueError):
            som_device.plane_minmax(bad)


# ---- the Sobel magnitude ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sobel_equals_scipy(gpu, shape):
    from ark_analysis_amd import som_device
    h, w = shape
    rs = np.random.RandomState(h * 1000 + w)
    fg = fmr.patterns(h, w)["noise_0.97"]
    planes = {"normal": rs.standard_normal((h, w)) * 40, "distance_map": fmr.blur(ndi.distance_transform_edt(fg), 1) * 9,
              "integers": rs.randint(-50, 50, (h, w)).astype(np.float64), "constant": np.full((h, w), 3.25),
              "ramp": np.add.outer(np.arange(h) * 8.0, np.arange(w) * 6.0)}
    for name, plane in planes.items():
        want = fmr.sobel_magnitude(plane)
        a, b = fmr.sobel_separable(plane)
        assert np.array_equal(want, np.sqrt((a * a + b * b) / 2)), name       # scipy.ndimage.sobel is the two stages
        if shape == PADDED:
            t = padded_in(plane, gpu, 3, fill=1e300)
            buf, out = sentinel_out(h, w, torch.float64, gpu, 9, -7.0)
            buf_i, out_i = sentinel_out(h, w, torch.int32, gpu, 17, -7)
        else:
            t, out, out_i = torch.from_numpy(plane).to(gpu), None, None
        got = som_device.sobel_magnitude(t, out=out)
        got_i = som_device.sobel_magnitude(t, out=out_i, as_int32=True)
        assert got.dtype == torch.float64 and got_i.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), want), name
        assert np.array_equal(got_i.cpu().numpy(), want.astype(np.int32)), name
        if name == "constant" or (h, w) == (1, 1):
            assert not want.any()
        if shape == PADDED:
            assert guard_intact(buf, h, w, -7.0) and guard_intact(buf_i, h, w, -7), name
    assert planes["ramp"].shape == (1, 1) or fmr.sobel_magnitude(planes["ramp"]).astype(np.int32).max() >= 4


def test_sobel_refusals(gpu):
    from ark_analysis_amd import _capi, som_device
    t = torch.zeros((6, 6), dtype=torch.float64, device=gpu)
    with pytest.raises(_capi.PxsomError, match="overlaps the plane"):
        som_device.sobel_magnitude(t, out=t)
    for bad in (t.to(torch.float32), t.cpu(), t[:0]):
        with pytest.raises(ValueError):
            som_device.sobel_magnitude(bad)
    with pytest.raises(ValueError, match="out must be"):
        som_device.sobel_magnitude(t, out=torch.zeros((6, 6), dtype=torch.float64, device=gpu), as_int32=True)


# ---- the markers and the cut --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (65, 64), (5, 1100), (200, 230)], ids=lambda s: "%dx%d" % s)
def test_markers_and_greater_equal_numpy(gpu, shape):
    from ark_analysis_amd import som_device
    h, w = shape
    rs = np.random.RandomState(h + w)
    t0, t1 = 0.75, 2.0 + 2.0 ** -40
    plane = rs.choice([0.0, t0, np.nextafter(t0, 0), np.nextafter(t0, 9), 1.0, t1, np.nextafter(t1, 0), np.nextafter(t1, 9), 5.0,
                       np.nan, -0.0], size=(h, w))
    plane.flat[0] = t0
    plane.flat[-1] = t1
    padded = shape == (200, 230)
    t = padded_in(plane, gpu, 7, fill=9.0) if padded else torch.from_numpy(plane).to(gpu)
    buf, out = sentinel_out(h, w, torch.int32, gpu, 5, -7) if padded else (None, None)
    got = som_device.class_markers(t, t0, t1, out=out)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), fmr.class_markers(plane, t0, t1))
    # thresholds the wrong way round: the `> t1` assignment is applied last
    assert np.array_equal(som_device.class_markers(t, t1, t0).cpu().numpy(), fmr.class_markers(plane, t1, t0))
    buf8, out8 = sentinel_out(h, w, torch.uint8, gpu, 5, 7) if padded else (None, None)
    above = som_device.plane_greater(t, t0, out=out8)
    assert above.dtype == torch.uint8 and np.array_equal(above.cpu().numpy(), (plane > t0).astype(np.uint8))
    if padded:
        assert guard_intact(buf, h, w, -7) and guard_intact(buf8, h, w, 7)
    with pytest.raises(ValueError, match="NaN"):
        som_device.class_markers(t, float("nan"), 1.0)
    with pytest.raises(ValueError, match="NaN"):
        som_device.plane_greater(t, float("nan"))


# ---- the chain ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g28():
    return np.load(os.path.join(tfm.GOLDEN, tfm.FIXTURE))


def test_chain_equals_every_fixture(gpu, g28):
    from ark_analysis_amd import som_device
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    cutoff, sobel_blur = float(g28["cutoff"]), float(g28["sobel_blur"])
    for name in json.loads(str(g28["names"])):
        fg = g28["fg_" + name]
        ridges = fmr.ridge_plane(fg, cutoff)
        t = torch.from_numpy(ridges).to(gpu)
        assert np.array_equal(som_device.plane_greater(t, cutoff).cpu().numpy(), fg), name
        assert np.array_equal(som_device.distance_transform_edt(torch.from_numpy(fg).to(gpu), squared=True).cpu().numpy(),
                              g28["sq_" + name]), name
        dist, (t0, t1), markers, elevation = som_device.watershed_inputs(t, cutoff, sobel_blur)
        assert np.array_equal(dist.cpu().numpy(), g28["dist_" + name]), name
        assert np.array_equal(som_device.plane_histogram(dist)[0].cpu().numpy(), g28["counts_" + name]), name
        assert [t0, t1] == g28["thr_" + name][0].tolist(), name
        assert markers.dtype == torch.int32 and np.array_equal(markers.cpu().numpy(), g28["markers_" + name]), name
        assert elevation.dtype == torch.int32 and np.array_equal(elevation.cpu().numpy(), g28["elevation_" + name]), name
        smooth = som_device.gaussian_blur_plane_mode(dist, sobel_blur, "reflect")
        assert np.array_equal(som_device.sobel_magnitude(smooth).cpu().numpy(), g28["elev_" + name]), name
        # the public host function, through its device entry
        got = fs.fiber_watershed_inputs(ridges, cutoff, sobel_blur)
        assert np.array_equal(got.distance_transformed, g28["dist_" + name]) and np.array_equal(got.markers, g28["markers_" + name])
        assert np.array_equal(got.thresholds, g28["thr_" + name][0]) and np.array_equal(got.elevation_map, g28["elevation_" + name])


def test_chain_refusals(gpu):
    from ark_analysis_amd import som_device
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    with pytest.raises(ValueError, match="no background pixel"):
        fs.fiber_watershed_inputs(np.full((6, 7), 3.0))
    with pytest.raises(ValueError, match="only 1 different values"):
        fs.fiber_watershed_inputs(np.zeros((6, 7)))
    with pytest.raises(ValueError, match="only 1 different values"):
        fs.fiber_watershed_inputs(np.full((6, 7), np.nan))
    t = torch.zeros((6, 7), dtype=torch.float64, device=gpu)
    with pytest.raises(NotImplementedError, match="sigma 17"):
        som_device.watershed_inputs(t, 0.1, 17)
    for bad in (t.to(torch.float32), t.cpu(), t[:0], t.t()):
        with pytest.raises(ValueError, match="ridges must be"):
            som_device.watershed_inputs(bad, 0.1, 1)
    # the caller's own choice of thresholds reaches the markers
    ridges = fmr.ridge_plane(fmr.bars(30, 41, np.random.RandomState(2), 3))
    dist, t01, markers, _ = som_device.watershed_inputs(torch.from_numpy(ridges).to(gpu), 0.1, 1, thresholds=lambda c, e: (0.25, 1.5))
    assert t01 == (0.25, 1.5) and np.array_equal(markers.cpu().numpy(), fmr.class_markers(dist.cpu().numpy(), 0.25, 1.5))
