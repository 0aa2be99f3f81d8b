"""The Frangi ridge filter on the GPU (K26): som_device.frangi equal, bit for bit, to the numpy / scipy statement of
tests/frangi_reference.py -- over the sizes at which np.gradient's border rules meet (a side of 2, 3, 4 or 5: every pixel
within two of a border), one and several 64 x 4 workgroups along either axis, and sizes that are no multiple of the tile;
over four sigma sets, among them the widest radius the blur takes (64, on planes far smaller than it); on every pattern
class of the g29 fixture and a plane with a NaN pixel; always on row-padded inputs and outputs inside sentinel-filled
buffers.  Then the single-scale entry against the fixture's per-scale planes and its accumulating form, the chain against
the two chained fixture cases, and the host function against every fixture case."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fiber_markers_reference as fmr
from tests import frangi_reference as fr
from tests.test_gpu_fiber_markers import guard_intact, padded_in, sentinel_out

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(2, 2), (2, 7), (7, 2), (3, 3), (4, 5), (5, 4), (17, 33), (64, 65), (65, 64), (33, 130), (5, 300)]
IDS = ["%dx%d" % s for s in SHAPES]
SIGMA_SETS = [(1,), (1, 3, 5, 7, 9), (0.5, 2.5), (16,)]
SENTINEL = -7.0


@pytest.fixture(scope="module")
def g29():
    return np.load(os.path.join(HERE, "golden", "g29_frangi.npz"))


def planes_at(h, w):
    """The fixture's pattern classes at this size, and bars with one NaN pixel."""
    planes = fr.patterns(h, w)
    with_nan = planes["bars"].copy()
    with_nan[h // 2, w // 2] = np.nan
    planes["nan_pixel"] = with_nan
    return planes


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_frangi_equals_the_statement(gpu, shape):
    from ark_analysis_amd import som_device
    h, w = shape
    run = 0
    for sigmas in SIGMA_SETS:
        for name, plane in planes_at(h, w).items():
            scale = (1.0, 10000.0)[run % 2]
            run += 1
            want = fr.frangi(plane, sigmas, scale=scale)
            t = padded_in(plane, gpu, 1 + run % 7, fill=1e300)
            buf, out = sentinel_out(h, w, torch.float64, gpu, 4 + run % 5, SENTINEL)
            got = som_device.frangi(t, sigmas, scale=scale, out=out)
            assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float64 and got.shape == (h, w)
            assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), (name, sigmas, scale)
            assert guard_intact(buf, h, w, SENTINEL), (name, sigmas)
            assert np.array_equal(t.cpu().numpy(), plane, equal_nan=True)                      # the input is left as it was
            if name == "nan_pixel":
                assert np.isnan(want[h // 2, w // 2])
            elif name == "constant":
                assert not want.any()
            else:
                assert not np.isnan(want).any()
    assert run == len(SIGMA_SETS) * 9


def test_defaults_beta_gamma_and_a_new_output(gpu):
    from ark_analysis_amd import som_device
    plane = fr.patterns(33, 47)["bars"]
    t = torch.from_numpy(plane).to(gpu)
    got = som_device.frangi(t)
    assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), fr.frangi(plane, (1, 3, 5, 7, 9), 0.5, 15, 1.0))
    got = som_device.frangi(t, range(1, 4), beta=0.8, gamma=2.5, scale=3.0)
    assert np.array_equal(got.cpu().numpy(), fr.frangi(plane, (1, 2, 3), 0.8, 2.5, 3.0))
    # a caller's out that held something else is overwritten, not folded into
    out = torch.full((33, 47), 9.0, dtype=torch.float64, device=gpu)
    assert np.array_equal(som_device.frangi(t, (2,), out=out).cpu().numpy(), fr.frangi(plane, (2,)))


def test_scale_entry_equals_the_fixture_scales_and_accumulates(gpu, g29):
    from ark_analysis_amd import _capi, som_device
    sigmas, bsq, gsq = g29["sigmas"].tolist(), 2.0 * float(g29["beta"]) ** 2, 2.0 * float(g29["gamma"]) ** 2
    for name, plane in fr.fixture_planes().items():
        if "scales_" + name not in g29.files:
            continue
        h, w = plane.shape
        t = torch.from_numpy(plane).to(gpu)
        for i, sigma in enumerate(sigmas):
            g = som_device.gaussian_blur_plane_mode(t, sigma, "reflect")
            buf, out = sentinel_out(h, w, torch.float64, gpu, 5, SENTINEL)
            _capi.call("pxsom_frangi_scale", g.data_ptr(), w, h, w, sigma ** 2, bsq, gsq, 1, 1.0, out.data_ptr(), out.stride(0),
                       _capi.stream_ptr())
            v = g29["scales_" + name][i]
            assert np.array_equal(out.cpu().numpy(), v), (name, sigma)
            # the accumulating form on a caller's plane: values above, below and equal to v, and a NaN
            prev = np.where((np.add.outer(np.arange(h), np.arange(w)) % 3) == 0, v * 2.0 + 1e-9, v * 0.5)
            prev[0, 0], prev[h - 1, w - 1] = np.nan, v[h - 1, w - 1]
            out.copy_(torch.from_numpy(prev).to(gpu))
            _capi.call("pxsom_frangi_scale", g.data_ptr(), w, h, w, sigma ** 2, bsq, gsq, 0, 10000.0, out.data_ptr(), out.stride(0),
                       _capi.stream_ptr())
            assert np.array_equal(out.cpu().numpy(), np.maximum(prev, v) * 10000.0, equal_nan=True), (name, sigma)
            assert guard_intact(buf, h, w, SENTINEL)


def test_chain_equals_the_chained_fixture_cases(gpu, g29):
    from ark_analysis_amd import som_device
    cutoff, sobel_blur = float(g29["cutoff"]), float(g29["sobel_blur"])
    planes = fr.fixture_planes()
    chained = [n for n in json.loads(str(g29["names"])) if "dist_" + n in g29.files]
    assert len(chained) == 2
    for name in chained:
        t = torch.from_numpy(planes[name]).to(gpu)
        ridges, dist, (t0, t1), markers, elevation = som_device.ridge_watershed_inputs(t, g29["sigmas"], cutoff, sobel_blur)
        assert ridges.is_cuda and np.array_equal(ridges.cpu().numpy(), g29["ridges_" + name]), name
        assert np.array_equal(som_device.plane_greater(ridges, cutoff).cpu().numpy(), g29["fg_" + name]), name
        assert np.array_equal(dist.cpu().numpy(), g29["dist_" + name]), name
        assert np.array_equal(som_device.plane_histogram(dist)[0].cpu().numpy(), g29["counts_" + name]), name
        assert [t0, t1] == g29["thr_" + name].tolist(), name
        assert markers.dtype == torch.int32 and np.array_equal(markers.cpu().numpy(), g29["markers_" + name]), name
        assert elevation.dtype == torch.int32 and np.array_equal(elevation.cpu().numpy(), g29["elevation_" + name]), name
        smooth = som_device.gaussian_blur_plane_mode(dist, sobel_blur, "reflect")
        assert np.array_equal(som_device.sobel_magnitude(smooth).cpu().numpy(), g29["elev_" + name]), name
        # the caller's thresholds, beta and gamma reach their stages
        got = som_device.ridge_watershed_inputs(t, (1, 3), cutoff, sobel_blur, thresholds=lambda c, e: (0.25, 1.5), beta=0.7, gamma=9.0)
        want = fr.frangi(planes[name], (1, 3), 0.7, 9.0, 10000.0)
        assert np.array_equal(got[0].cpu().numpy(), want) and got[2] == (0.25, 1.5)
        assert np.array_equal(got[3].cpu().numpy(), fmr.class_markers(got[1].cpu().numpy(), 0.25, 1.5))


def test_host_functions_equal_the_fixture(gpu, g29):
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    planes = fr.fixture_planes()
    for name, plane in planes.items():
        got = fs.frangi_ridges(plane)
        assert got.dtype == np.float64 and np.array_equal(got, g29["ridges_" + name]), name
    for name in ("bars", "disc"):
        inputs, ridges = fs.fiber_watershed_inputs_from_contrast(planes[name])
        assert np.array_equal(ridges, g29["ridges_" + name]) and np.array_equal(inputs.markers, g29["markers_" + name])
        assert np.array_equal(inputs.distance_transformed, g29["dist_" + name])
        assert np.array_equal(inputs.thresholds, g29["thr_" + name]) and np.array_equal(inputs.elevation_map, g29["elevation_" + name])


def test_refusals(gpu):
    from ark_analysis_amd import som_device
    t = torch.zeros((6, 7), dtype=torch.float64, device=gpu)
    for shape in ((1, 7), (7, 1), (1, 1)):
        with pytest.raises(ValueError, match=fr.TOO_SMALL):
            som_device.frangi(torch.zeros(shape, dtype=torch.float64, device=gpu))
    for bad in (t.to(torch.float32), t.cpu(), t[:0], t.t()):
        with pytest.raises(ValueError, match="plane"):
            som_device.frangi(bad)
    with pytest.raises(ValueError, match="must not share memory"):
        som_device.frangi(t, out=t)
    wide = torch.zeros((6, 16), dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError, match="must not share memory"):
        som_device.frangi(wide[:, :7], out=wide[:, 5:12])
    with pytest.raises(ValueError, match="out must be"):
        som_device.frangi(t, out=torch.zeros((6, 7), dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError, match="at least one sigma"):
        som_device.frangi(t, ())
    with pytest.raises(ValueError, match="less than zero"):
        som_device.frangi(t, (1, -1))
    with pytest.raises(ValueError, match="sigma 0"):
        som_device.frangi(t, (0,))
    with pytest.raises(NotImplementedError, match="sigma 17"):
        som_device.frangi(t, (1, 17))
    with pytest.raises(NotImplementedError, match="black_ridges"):
        som_device.frangi(t, black_ridges=True)
    with pytest.raises(NotImplementedError, match="gamma=None"):
        som_device.frangi(t, gamma=None)
    with pytest.raises(ValueError, match="beta and gamma"):
        som_device.frangi(t, beta=0)
    with pytest.raises(ValueError, match="scale must be finite"):
        som_device.frangi(t, scale=float("inf"))
    assert not bool(t.any())
