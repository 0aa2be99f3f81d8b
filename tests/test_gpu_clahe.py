"""Adaptive histogram equalisation on the GPU (K27): som_device.equalize_adapthist equal, bit for bit, to the numpy statement
of tests/clahe_reference.py -- the float64 result and, through maps_out and raw_out, the tile maps and the uint16 plane
before the last rescale -- over sizes from 2 x 2 (one pixel per tile, one tile in all), a single tile with every corner
clamped to it, odd tile sides on sizes that are no multiple of them, more than one 64 x 4 workgroup along either axis and
tiles of 1024 pixels (sixteen trips of a wave) and, with k = 33 and 64, larger ones (a workgroup per tile); on every
pattern class of the g30 fixture under the three clip limits (the default, 0.003 and none); always on row-padded inputs
and outputs inside sentinel-filled buffers.  Then the chain from a raw channel against the chained fixture case, and the
host functions against the fixture."""
import json
import os

import numpy as np
import pytest
import torch

from tests import clahe_reference as cr
from tests.test_gpu_fiber_markers import guard_intact, padded_in, sentinel_out

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [((2, 2), 1), ((2, 2), 2), ((3, 5), 2), ((3, 5), 3), ((8, 8), 8), ((9, 7), 7), ((16, 24), 8), ((17, 33), 4),
         ((17, 33), 5), ((33, 130), 8), ((40, 90), 7), ((64, 64), 32), ((64, 96), 32), ((128, 128), 8), ((33, 130), 33),
         ((70, 66), 64)]
IDS = ["%dx%d_k%d" % (s[0], s[1], k) for s, k in CASES]
CLIP_LIMITS = (0.01, 0.003, 0.0)
SENTINEL = -7.0
GUARD, GUARD_VALUE = 64, 0xABCD


@pytest.fixture(scope="module")
def g30():
    return np.load(os.path.join(HERE, "golden", "g30_clahe.npz"))


def u16_plane_out(h, w, gpu, pad):
    """A uint16 [h, w] view inside a guard-filled device buffer (torch has no fill for uint16: numpy makes it)."""
    buf = torch.from_numpy(np.full((h + 2, w + pad), GUARD_VALUE, np.uint16)).to(gpu)
    return buf, buf[1:h + 1, 3:w + 3]


def u16_maps_out(nty, ntx, gpu):
    """A contiguous uint16 [nty, ntx, 256] view with a guard on either side."""
    n = nty * ntx * 256
    buf = torch.from_numpy(np.full(n + 2 * GUARD, GUARD_VALUE, np.uint16)).to(gpu)
    return buf, buf[GUARD:GUARD + n].view(nty, ntx, 256)


def maps_guard_intact(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == GUARD_VALUE).all() and (b[-GUARD:] == GUARD_VALUE).all())


def run_equalize(gpu, call, plane, k, pad):
    """call(t, out, maps_out, raw_out) inside sentinel buffers -> the three host arrays, the guards checked."""
    h, w = plane.shape
    nty, ntx = -(-h // k), -(-w // k)
    t = padded_in(plane, gpu, pad, fill=1e300)
    obuf, out = sentinel_out(h, w, torch.float64, gpu, 4 + pad % 5, SENTINEL)
    rbuf, raw = u16_plane_out(h, w, gpu, 5 + pad % 3)
    mbuf, maps = u16_maps_out(nty, ntx, gpu)
    got = call(t, out, maps, raw)
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float64 and got.shape == (h, w)
    assert guard_intact(obuf, h, w, SENTINEL) and guard_intact(rbuf, h, w, GUARD_VALUE) and maps_guard_intact(mbuf)
    assert np.array_equal(t.cpu().numpy(), plane)                                          # the input is left as it was
    return got.cpu().numpy(), maps.cpu().numpy(), raw.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_equalize_adapthist_equals_the_statement(gpu, case):
    from ark_analysis_amd import som_device
    (h, w), k = case
    run = 0
    for name, plane in cr.patterns(h, w).items():
        for clip_limit in CLIP_LIMITS:
            run += 1
            want, _, want_maps, want_raw = cr.equalize_adapthist(plane, k, clip_limit)
            lo_hi = (float(plane.min()), float(plane.max())) if run % 2 else None
            got, maps, raw = run_equalize(
                gpu, lambda t, out, m, r: som_device.equalize_adapthist(t, k, clip_limit, out=out, lo_hi=lo_hi, maps_out=m, raw_out=r),
                plane, k, 1 + run % 7)
            assert np.array_equal(maps, want_maps), (name, clip_limit, "maps")
            assert np.array_equal(raw, want_raw), (name, clip_limit, "raw")
            assert np.array_equal(got, want), (name, clip_limit)
            assert got.min() >= 0.0 and got.max() <= 1.0
    assert run == 18


def test_defaults_a_new_output_and_a_float_kernel_size(gpu):
    from ark_analysis_amd import som_device
    plane = cr.patterns(40, 56)["fibres"]
    t = torch.from_numpy(plane).to(gpu)
    got = som_device.equalize_adapthist(t, 8)
    assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), cr.equalize_adapthist(plane, 8)[0])
    assert np.array_equal(som_device.equalize_adapthist(t, 5.9, clip_limit=0.02).cpu().numpy(), cr.equalize_adapthist(plane, 5, 0.02)[0])
    # a caller's out that held something else is overwritten
    out = torch.full((40, 56), 9.0, dtype=torch.float64, device=gpu)
    assert np.array_equal(som_device.equalize_adapthist(t, 8, out=out).cpu().numpy(), cr.equalize_adapthist(plane, 8)[0])


def test_fixture_cases(gpu, g30):
    from ark_analysis_amd import som_device
    for name, (plane, k, clip_limit) in cr.fixture_cases().items():
        got = som_device.equalize_adapthist(torch.from_numpy(plane).to(gpu), k, clip_limit)
        assert np.array_equal(got.cpu().numpy(), g30["result_" + name]), name


def test_contrast_adjust_and_the_chain_equal_the_chained_case(gpu, g30):
    from ark_analysis_amd import som_device
    channel = cr.chain_channel()
    blur, k = float(g30["chain_blur"]), int(g30["chain_k"])
    cutoff, sobel_blur = float(g30["cutoff"]), float(g30["sobel_blur"])
    got, maps, raw = run_equalize(gpu, lambda t, out, m, r: som_device.contrast_adjust(t.contiguous(), blur, k, out=out, maps_out=m, raw_out=r),
                                  channel, k, 3)
    assert np.array_equal(maps, g30["chain_maps"]) and np.array_equal(raw, g30["chain_raw"])
    assert np.array_equal(got, g30["chain_contrast"])
    t = torch.from_numpy(channel).to(gpu)
    contrast, ridges, dist, (t0, t1), markers, elevation = som_device.channel_watershed_inputs(t, blur, k, (1, 3, 5, 7, 9), cutoff,
                                                                                             sobel_blur)
    assert contrast.is_cuda and np.array_equal(contrast.cpu().numpy(), g30["chain_contrast"])
    assert np.array_equal(ridges.cpu().numpy(), g30["chain_ridges"])
    assert np.array_equal(som_device.plane_greater(ridges, cutoff).cpu().numpy(), g30["chain_fg"])
    assert np.array_equal(dist.cpu().numpy(), g30["chain_dist"])
    assert np.array_equal(som_device.plane_histogram(dist)[0].cpu().numpy(), g30["chain_counts"])
    assert [t0, t1] == g30["chain_thr"].tolist()
    assert markers.dtype == torch.int32 and np.array_equal(markers.cpu().numpy(), g30["chain_markers"])
    assert elevation.dtype == torch.int32 and np.array_equal(elevation.cpu().numpy(), g30["chain_elevation"])
    assert np.array_equal(t.cpu().numpy(), channel)
    # contrast_adjust on every fixture channel: the blur, the division and the quantisation over min / max, 1.0
    for name, (raw_channel, kk, clip_limit) in cr.fixture_channels().items():
        got = som_device.contrast_adjust(torch.from_numpy(raw_channel).to(gpu), 2, kk, clip_limit)
        assert np.array_equal(got.cpu().numpy(), g30["result_" + name]), name


def test_host_functions_equal_the_fixture(gpu, g30):
    from ark_analysis_amd.segmentation import fiber_segmentation as fs
    for name, (channel, k, clip_limit) in cr.fixture_channels().items():
        if clip_limit != 0.01:
            continue
        got = fs.contrast_adjusted_channel(channel, blur=2, contrast_scaling_divisor=channel.shape[0] / (k + 0.5))
        assert got.dtype == np.float64 and np.array_equal(got, g30["result_" + name]), name
    channel = cr.chain_channel()
    divisor = channel.shape[0] / int(g30["chain_k"])
    inputs, ridges, contrast = fs.fiber_watershed_inputs_from_channel(channel, contrast_scaling_divisor=divisor)
    assert np.array_equal(contrast, g30["chain_contrast"]) and np.array_equal(ridges, g30["chain_ridges"])
    assert np.array_equal(inputs.distance_transformed, g30["chain_dist"]) and np.array_equal(inputs.thresholds, g30["chain_thr"])
    assert np.array_equal(inputs.markers, g30["chain_markers"]) and np.array_equal(inputs.elevation_map, g30["chain_elevation"])
    assert json.loads(str(g30["names"])) == list(cr.fixture_channels())


def test_refusals(gpu):
    from ark_analysis_amd import som_device
    t = torch.full((6, 7), 0.5, dtype=torch.float64, device=gpu)
    for bad in (t.to(torch.float32), t.cpu(), t[:0], t.t()):
        with pytest.raises(ValueError, match="plane"):
            som_device.equalize_adapthist(bad, 2)
    with pytest.raises(ValueError, match="H, W >= 2"):
        som_device.equalize_adapthist(t[:1], 1)
    with pytest.raises(ValueError, match="must not share memory"):
        som_device.equalize_adapthist(t, 2, out=t)
    with pytest.raises(ValueError, match="out must be"):
        som_device.equalize_adapthist(t, 2, out=torch.zeros((6, 7), dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError, match="maps_out"):
        som_device.equalize_adapthist(t, 2, maps_out=torch.zeros((3, 3, 256), dtype=torch.int16, device=gpu))
    with pytest.raises(NotImplementedError, match="beyond the shorter side"):
        som_device.equalize_adapthist(t, 7)
    with pytest.raises(NotImplementedError, match="256 bins"):
        som_device.equalize_adapthist(t, 2, nbins=128)
    with pytest.raises(ValueError, match="at least 1"):
        som_device.equalize_adapthist(t, 0.5)
    with pytest.raises(ValueError, match="clip_limit must be finite"):
        som_device.equalize_adapthist(t, 2, clip_limit=float("nan"))
    with_nan = t.clone()
    with_nan[2, 3] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        som_device.equalize_adapthist(with_nan, 2)
    with pytest.raises(ValueError, match="finite plane"):
        som_device.equalize_adapthist(t, 2, lo_hi=(0.0, float("inf")))
    with pytest.raises(ValueError, match="positive maximum"):
        som_device.contrast_adjust(torch.zeros((6, 7), dtype=torch.float64, device=gpu), 2, 2)
    with pytest.raises(ValueError, match="positive maximum"):
        som_device.contrast_adjust(-t, 2, 2)
    with pytest.raises(NotImplementedError, match="sigma 17"):
        som_device.contrast_adjust(t, 17, 2)
    with pytest.raises(ValueError, match="contiguous"):
        som_device.contrast_adjust(torch.zeros((6, 9), dtype=torch.float64, device=gpu)[:, :7], 2, 2)
    assert bool((t == 0.5).all())
