"""Seeded fuzz of the K25 entries against tests/fiber_markers_reference.py, twelve cases dealt over the route classes:
size class (fewer rows than the 16 column stretches of the distance transform's first pass; one workgroup; several
workgroups per row or column band), foreground density (sparse bars, even noise, nearly full, a single background pixel),
row stride (contiguous or padded) and ``sobel_blur`` (0: the blur is skipped; 0.6; 1; 2.5).  Every caller-owned output is
a view inside a sentinel-filled buffer whose guard must come back intact.  Every case ends in comparisons: none is
skipped."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from tests import fiber_markers_reference as fmr
from tests.test_gpu_fiber_markers import guard_intact, padded_in, sentinel_out

pytestmark = pytest.mark.gpu

CASES, SEED = 12, 2025
SIZE_CLASSES = ("few_rows", "one_workgroup", "several")
DENSITIES = ("bars", "noise", "nearly_full", "single_background")
SOBEL_BLURS = (0, 0.6, 1, 2.5)


def fuzz_cases(seed=SEED, count=CASES):
    rs = np.random.RandomState(seed)
    cases = []
    for i in range(count):
        size, density = SIZE_CLASSES[i % 3], DENSITIES[i % 4]
        if size == "few_rows":
            h, w = int(rs.randint(1, 16)), int(rs.randint(1, 400))
        elif size == "one_workgroup":
            h, w = int(rs.randint(16, 65)), int(rs.randint(2, 65))
        else:
            h, w = int(rs.randint(65, 180)), int(rs.randint(65, 300))
        if density == "bars":
            fg = fmr.bars(h, w, rs, int(rs.randint(1, 7)))
        elif density == "noise":
            fg = (rs.random_sample((h, w)) < rs.uniform(0.2, 0.8)).astype(np.uint8)
        elif density == "nearly_full":
            fg = (rs.random_sample((h, w)) < 0.995).astype(np.uint8)
        else:
            fg = np.ones((h, w), np.uint8)
        if fg.all():
            fg[rs.randint(h), rs.randint(w)] = 0
        cases.append({"i": i, "size": size, "density": density, "fg": fg, "pad": int(rs.randint(1, 40)) if i % 2 else 0,
                      "sobel_blur": SOBEL_BLURS[(i // 3) % 4], "cutoff": float(rs.choice([0.1, 0.5, 3.0]))})
    return cases


def test_the_cases_cover_the_route_classes():
    cases = fuzz_cases()
    assert len(cases) == 12
    assert {c["size"] for c in cases} == set(SIZE_CLASSES) and {c["density"] for c in cases} == set(DENSITIES)
    assert {c["sobel_blur"] for c in cases} == set(SOBEL_BLURS) and {bool(c["pad"]) for c in cases} == {False, True}
    assert {(c["size"], c["density"]) for c in cases} == {(s, d) for s in SIZE_CLASSES for d in DENSITIES}
    assert all(not c["fg"].all() for c in cases)


@pytest.mark.parametrize("case", fuzz_cases(), ids=lambda c: "%d_%s_%s" % (c["i"], c["size"], c["density"]))
def test_fuzz_fibre_markers(gpu, case):
    from ark_analysis_amd import som_device
    fg, pad, sobel_blur, cutoff = case["fg"], case["pad"], case["sobel_blur"], case["cutoff"]
    h, w = fg.shape
    ridges = fmr.ridge_plane(fg, cutoff)
    assert np.array_equal(ridges > cutoff, fg != 0)

    def view_in(plane, fill):
        return padded_in(plane, gpu, pad, fill) if pad else torch.from_numpy(plane).to(gpu)

    # the cut
    buf, out = sentinel_out(h, w, torch.uint8, gpu, 3 + pad, 7)
    got_fg = som_device.plane_greater(view_in(ridges, 99.0), cutoff, out=out)
    assert np.array_equal(got_fg.cpu().numpy(), fg) and guard_intact(buf, h, w, 7)
    # the distance transform, from the strided cut
    want_edt = ndi.distance_transform_edt(fg)
    buf, out = sentinel_out(h, w, torch.float64, gpu, 3 + pad, -7.0)
    buf_sq, out_sq = sentinel_out(h, w, torch.int32, gpu, 4 + pad, -7)
    assert np.array_equal(som_device.distance_transform_edt(got_fg, out=out).cpu().numpy(), want_edt)
    assert np.array_equal(som_device.distance_transform_edt(got_fg, out=out_sq, squared=True).cpu().numpy(),
                          np.rint(want_edt * want_edt).astype(np.int32))
    assert guard_intact(buf, h, w, -7.0) and guard_intact(buf_sq, h, w, -7)
    if h * w <= 6000:
        assert np.array_equal(out_sq.cpu().numpy(), fmr.squared_distances(fg))
    # minimum, maximum, histogram of the strided distance map
    want = fmr.stages(ridges, cutoff, sobel_blur, thresholds=lambda c, e: (e[40], e[170]))
    dist = view_in(want["dist"], 1e300)
    assert som_device.plane_minmax(dist) == (want["dist"].min(), want["dist"].max())
    counts, edges = som_device.plane_histogram(dist)
    assert np.array_equal(counts.cpu().numpy(), want["counts"]) and np.array_equal(edges, want["edges"])
    # markers on thresholds that are edges of the histogram, hence near values of the plane
    buf, out = sentinel_out(h, w, torch.int32, gpu, 3 + pad, -7)
    assert np.array_equal(som_device.class_markers(dist, want["t0"], want["t1"], out=out).cpu().numpy(), want["markers"])
    assert guard_intact(buf, h, w, -7)
    # the Sobel magnitude of the strided smoothed map, scaled so that its int32 form is not all 0 and 1
    smooth = fmr.blur(want["dist"], sobel_blur) * 37.0
    mag = fmr.sobel_magnitude(smooth)
    buf, out = sentinel_out(h, w, torch.float64, gpu, 3 + pad, -7.0)
    buf_i, out_i = sentinel_out(h, w, torch.int32, gpu, 5 + pad, -7)
    assert np.array_equal(som_device.sobel_magnitude(view_in(smooth, 1e300), out=out).cpu().numpy(), mag)
    assert np.array_equal(som_device.sobel_magnitude(view_in(smooth, 1e300), out=out_i, as_int32=True).cpu().numpy(), mag.astype(np.int32))
    assert guard_intact(buf, h, w, -7.0) and guard_intact(buf_i, h, w, -7)
    # the chain on the resident plane, with caller-owned markers and elevation
    buf_m, out_m = sentinel_out(h, w, torch.int32, gpu, 3 + pad, -7)
    buf_e, out_e = sentinel_out(h, w, torch.int32, gpu, 6 + pad, -7)
    got_dist, t01, markers, elevation = som_device.watershed_inputs(torch.from_numpy(ridges).to(gpu), cutoff, sobel_blur,
                                                                    thresholds=lambda c, e: (e[40], e[170]), markers=out_m,
                                                                    elevation=out_e)
    assert np.array_equal(got_dist.cpu().numpy(), want["dist"]) and t01 == (want["t0"], want["t1"])
    assert np.array_equal(markers.cpu().numpy(), want["markers"]) and np.array_equal(elevation.cpu().numpy(), want["elevation"])
    assert guard_intact(buf_m, h, w, -7) and guard_intact(buf_e, h, w, -7)
