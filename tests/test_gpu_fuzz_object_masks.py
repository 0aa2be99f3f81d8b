"""Randomised sweep of K16 (som_device.label_components and som_device.object_mask) against the scipy statement of
tests/object_mask_reference.py; the comparison is exact.  Case i takes class i % R of the table CLASSES -- a size class, a
density, the connectivity, plain or inverted, a threshold kind and a hole kind, every value of every factor visited -- and
draws the rest (seeded).  A default run is max(12, R) cases and skips none.  ``PXSOM_FUZZ_SEED`` as in
test_gpu_fuzz_parity.py; ``PXSOM_FUZZ_CASES`` widens the run.  The generator is device-free."""
import os

import numpy as np
import pytest

from tests import object_mask_reference as omr

SEED = int(os.environ.get("PXSOM_FUZZ_SEED", "20261017"))
SIZES = ["small", "tile", "tiles"]
DENSITIES = [0.1, 0.5, 0.9]
THRESHOLDS = ["none", "percentile", "local"]
HOLES = ["none", "int"]
CLASSES = [(SIZES[i % 3], DENSITIES[(i // 3 + i) % 3], 1 + i % 2, bool((i // 2) % 2), THRESHOLDS[(i // 4) % 3],
            HOLES[(i + i // 6) % 2]) for i in range(12)]
R = len(CLASSES)
CASES = max(int(os.environ.get("PXSOM_FUZZ_CASES", "0")), 12, R)


def gen_case(i, seed=SEED):
    rs = np.random.RandomState((seed + 104729 * i) % (2 ** 32))
    size, density, connectivity, invert, thresh_kind, hole_kind = CLASSES[i % R]
    lo, hi = {"small": (1, 20), "tile": (40, 70), "tiles": (65, 200)}[size]
    h, w = int(rs.randint(lo, hi + 1)), int(rs.randint(lo, hi + 1))
    mask = (rs.rand(h, w) < density).astype(np.uint8)
    # an image for the whole chain: sparse spikes, blurred by the chain itself
    img = (rs.rand(h, w) < 0.01 + 0.03 * density) * rs.gamma(2.0, 20.0, size=(h, w))
    img = img.astype(np.float32 if rs.randint(2) else np.float64)
    sigma = [None, 0.7, 1.0, 2.5][rs.randint(4)]
    thresh = {"none": None, "percentile": int(rs.randint(1, 100)), "local": "auto"}[thresh_kind]
    block = int(2 * rs.randint(1, 15) + 1) if thresh_kind == "local" else None
    hole = int(rs.randint(1, 40)) if hole_kind == "int" else None
    min_area = int(rs.randint(0, 12))
    max_area = int(rs.choice([min_area + rs.randint(0, 300), h * w, h * w]))
    return dict(mask=mask, connectivity=connectivity, invert=invert, img=img, sigma=sigma, thresh=thresh, block=block,
                hole=hole, min_area=min_area, max_area=max_area, cls=CLASSES[i % R])


def test_classes_cover_every_value():
    for pos, values in enumerate((SIZES, DENSITIES, (1, 2), (False, True), THRESHOLDS, HOLES)):
        assert {c[pos] for c in CLASSES} == set(values)
    assert CASES >= max(12, R)
    from ark_analysis_amd import _capi
    assert "pxsom_label_components" in _capi.SYMBOLS and "pxsom_components_select" in _capi.SYMBOLS


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(CASES))
def test_fuzz_object_masks(gpu, i):
    import torch
    from ark_analysis_amd import som_device
    c = gen_case(i)
    what = repr((i, c["cls"], c["mask"].shape, c["sigma"], c["thresh"], c["block"], c["hole"], c["min_area"], c["max_area"]))
    labels, n, areas = som_device.label_components(torch.from_numpy(c["mask"]).to(gpu), c["connectivity"], invert=c["invert"])
    want_labels, want_n, want_areas = omr.label_components(c["mask"], c["connectivity"], c["invert"])
    n = int(n.item())
    assert n == want_n, what
    assert np.array_equal(labels.cpu().numpy(), want_labels), what
    areas = areas.cpu().numpy()
    assert np.array_equal(areas[:n + 1], want_areas) and not areas[n + 1:].any(), what
    got = som_device.object_mask(torch.from_numpy(c["img"]).to(gpu), c["sigma"], c["thresh"], c["hole"], c["min_area"],
                                 c["max_area"], c["block"])
    want = omr.object_mask(c["img"], c["sigma"], c["thresh"], c["hole"], c["min_area"], c["max_area"], c["block"])
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), what
