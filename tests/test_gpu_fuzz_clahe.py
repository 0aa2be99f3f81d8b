"""Seeded fuzz of som_device.equalize_adapthist against tests/clahe_reference.py, twelve cases dealt over the classes at
which the kernels' paths differ: size class (a few pixels a side, where every tile is a border tile; one short side and
several 64-column workgroups on the other, either way round; several workgroups both ways), tile side (1 or 2; odd; even;
the whole shorter side, so that one axis has a single tile), pattern (noisy bars, a smooth wave, noise, a single pixel,
fibres, a constant), row stride of input and output (contiguous or padded) and clip limit (the default, 0.003, a generous
0.05, none).  Every output -- the float64 plane, the tile maps and the uint16 plane -- is a view inside a guard-filled
buffer and is compared with the statement.  Every case ends in comparisons: none is skipped."""
import numpy as np
import pytest
import torch

from tests import clahe_reference as cr
from tests.test_gpu_clahe import GUARD_VALUE, maps_guard_intact, u16_maps_out, u16_plane_out
from tests.test_gpu_fiber_markers import guard_intact, padded_in, sentinel_out

pytestmark = pytest.mark.gpu

CASES, SEED = 12, 2027
SIZE_CLASSES = ("tiny", "short_side", "several")
PATTERNS = ("bars", "smooth", "noise", "single_pixel", "fibres", "constant")
K_CLASSES = ("small", "odd", "even", "whole_side")
CLIP_LIMITS = (0.01, 0.003, 0.05, 0.0)


def fuzz_cases(seed=SEED, count=CASES):
    rs = np.random.RandomState(seed)
    cases = []
    for i in range(count):
        size, pattern, k_class = SIZE_CLASSES[i % 3], PATTERNS[(i // 3 + i) % 6], K_CLASSES[(i // 3) % 4]
        if size == "tiny":
            h, w = int(rs.randint(2, 8)), int(rs.randint(2, 8))
        elif size == "short_side":
            h, w = int(rs.randint(2, 9)), int(rs.randint(65, 300))
            if i % 2:
                h, w = w, h
        else:
            h, w = int(rs.randint(20, 100)), int(rs.randint(65, 200))
        short = min(h, w)
        if k_class == "small":
            k = int(rs.randint(1, 3))
        elif k_class == "odd":
            k = min(short if short % 2 else short - 1, int(rs.choice([3, 5, 7, 9, 11])))
        elif k_class == "even":
            k = max(2, min(short - short % 2, int(rs.choice([4, 6, 8, 16, 32]))))
        else:
            k = short
        plane = cr.patterns(h, w, seed=int(rs.randint(1 << 30)))[pattern] * rs.uniform(0.5, 40.0) - rs.uniform(0.0, 3.0)
        cases.append({"i": i, "size": size, "pattern": pattern, "k_class": k_class, "k": k, "plane": plane,
                      "pad": int(rs.randint(1, 40)) if i % 2 else 0, "clip_limit": CLIP_LIMITS[(i + i // 4) % 4]})
    return cases


def test_the_cases_cover_the_classes():
    cases = fuzz_cases()
    assert len(cases) == 12
    assert {c["size"] for c in cases} == set(SIZE_CLASSES) and {c["pattern"] for c in cases} == set(PATTERNS)
    assert {c["k_class"] for c in cases} == set(K_CLASSES) and {c["clip_limit"] for c in cases} == set(CLIP_LIMITS)
    assert {(c["size"], c["k_class"]) for c in cases} == {(s, k) for s in SIZE_CLASSES for k in K_CLASSES}
    assert {bool(c["pad"]) for c in cases} == {False, True}
    assert all(1 <= c["k"] <= min(c["plane"].shape) and min(c["plane"].shape) >= 2 for c in cases)
    assert any(c["k"] % 2 == 1 and c["k"] > 1 for c in cases) and any(c["k"] == 1 for c in cases)
    assert any(c["plane"].shape[0] > 64 and c["plane"].shape[1] < 9 for c in cases)
    assert any(c["plane"].shape[0] % c["k"] and c["plane"].shape[1] % c["k"] for c in cases)


@pytest.mark.parametrize("case", fuzz_cases(), ids=lambda c: "%d_%s_%s_k%d" % (c["i"], c["size"], c["pattern"], c["k"]))
def test_fuzz_equalize_adapthist(gpu, case):
    from ark_analysis_amd import som_device
    plane, pad, k, clip_limit = case["plane"], case["pad"], case["k"], case["clip_limit"]
    h, w = plane.shape
    nty, ntx = -(-h // k), -(-w // k)
    want, _, want_maps, want_raw = cr.equalize_adapthist(plane, k, clip_limit)
    t = padded_in(plane, gpu, pad, 1e300) if pad else torch.from_numpy(plane).to(gpu)
    obuf, out = sentinel_out(h, w, torch.float64, gpu, 3 + pad, -7.0)
    rbuf, raw = u16_plane_out(h, w, gpu, 4 + pad)
    mbuf, maps = u16_maps_out(nty, ntx, gpu)
    got = som_device.equalize_adapthist(t, k, clip_limit, out=out, maps_out=maps, raw_out=raw)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(maps.cpu().numpy(), want_maps)
    assert np.array_equal(raw.cpu().numpy(), want_raw)
    assert np.array_equal(got.cpu().numpy(), want)
    assert guard_intact(obuf, h, w, -7.0) and guard_intact(rbuf, h, w, GUARD_VALUE) and maps_guard_intact(mbuf)
    assert np.array_equal(t.cpu().numpy(), plane)
    # the same call into new outputs, with the range handed in
    again = som_device.equalize_adapthist(t, k, clip_limit, lo_hi=(float(plane.min()), float(plane.max())))
    assert np.array_equal(again.cpu().numpy(), want)
