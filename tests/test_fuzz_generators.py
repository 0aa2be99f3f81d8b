"""The case generators of the randomised sweeps (test_gpu_fuzz_parity.py: metric assign / online training;
test_gpu_fuzz_images.py: K10 - K12) on CPU: the first 12 cases of each -- the default PXSOM_FUZZ_CASES -- land in every
route class they are meant to visit, each case's class is the one the library's own rule gives for its parameters, and
one seed gives the same cases twice."""
import numpy as np

from tests import test_gpu_fuzz_images as fi
from tests import test_gpu_fuzz_parity as fp

N = 12


def _same_cases(a, b):
    assert len(a) == len(b)
    for ca, cb in zip(a, b):
        assert ca.keys() == cb.keys()
        for key in ca:
            va, vb = ca[key], cb[key]
            if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
                assert isinstance(va, np.ndarray) and isinstance(vb, np.ndarray), key
                assert va.dtype == vb.dtype and va.shape == vb.shape, key
                assert np.array_equal(va.view(np.uint8) if va.size else va, vb.view(np.uint8) if vb.size else vb), key
            elif isinstance(va, list):
                _same_cases(va, vb)
            else:
                assert va == vb or (va != va and vb != vb), key


def _twice(gen, seed):
    a, b = list(gen(seed, N)), list(gen(seed, N))
    _same_cases(a, b)
    assert len(a) == N
    return a


def test_metric_assign_generator():
    cases = _twice(fp.metric_assign_cases, fp.SEED + 20)
    seen = set()
    for c in cases:
        assert c["route"] == fp.metric_assign_route(c["c"]) == ("register" if c["c"] <= 32 else "staged")
        assert 1 <= c["k"] <= 1024 and 1 <= c["c"] <= 1024 and c["n"] >= 1
        assert c["x"].shape == (c["n"], c["c"]) and c["w"].shape == (c["k"], c["c"])
        seen.add((c["route"], c["metric"]))
    assert seen == {(r, m) for r in fp.METRIC_ASSIGN_ROUTES for m in (1, 3, 4)}
    assert any(c["reuse"] for c in cases), "no case repeats the workspace shape of an earlier one"


def test_metric_online_generator():
    cases = _twice(fp.metric_online_cases, fp.SEED + 21)
    assert {c["route"] for c in cases} == set(fp.ONLINE_METRIC_ROUTES)
    assert {c["metric"] for c in cases} == {1, 3, 4}
    for c in cases:
        assert fp.online_metric_route(c["xdim"] * c["ydim"], c["c"]) == c["route"]
        assert c["order"].shape == (c["n"] * c["rlen"],) and c["w0"].shape == (c["xdim"] * c["ydim"], c["c"])
    assert fp.online_metric_route(100, 8) == "register"
    assert fp.online_metric_route(100, 150) == "lds"          # the named test's "codebook in LDS" shape
    assert fp.online_metric_route(264, 128) == "in_place"     # ... and its "trained where it lies" shape
    assert fp.online_metric_route(600, 20) == "lds"


def test_segmask_generator():
    cases = _twice(fi.segmask_cases, fi.SEED + 30)
    assert {c["route"] for c in cases} == set(fi.SEGMASK_ROUTES)
    for c in cases:
        keys = c["keys"]
        if c["route"] == "no_table":
            assert keys is None
            continue
        if c["route"] == "empty_table":
            assert keys.size == 0 and not c["lut"]
            continue
        assert np.all(keys[1:] > keys[:-1]) and keys.dtype == np.int32
        rng = int(keys[-1]) - int(keys[0]) + 1
        assert c["lut"] == fi.lut_route(keys.size, int(keys[0]), int(keys[-1]))
        assert c["lut"] == (c["route"] in ("lut", "lut_edge"))
        if c["route"] == "lut_edge":
            assert rng == 16 * keys.size + 65536
        if c["route"] == "search_edge":
            assert rng == 16 * keys.size + 65537
        assert 1 <= c["h"] <= 600 and 1 <= c["w"] <= 600 and c["seg"].shape == (c["h"], c["w"])
    assert fi.lut_route(1, 5, 5) and not fi.lut_route(0, 0, 0)
    assert fi.lut_route(2, 0, 16 * 2 + 65535) and not fi.lut_route(2, 0, 16 * 2 + 65536)


def test_blur_generators():
    cases = _twice(fi.blur_cases, fi.SEED + 31)
    assert {c["route"] for c in cases} == set(fi.BLUR_ROUTES)
    for c in cases:
        h, w = c["plane"].shape
        if c["route"] == "copy":
            assert c["sigma"] <= 1e-15
        else:
            assert 1e-15 < c["sigma"] < fi.BLUR_SIGMA_LIMIT
        if c["route"] == "short_plane":
            assert h <= fi._radius(c["sigma"]) and w <= fi._radius(c["sigma"])
        assert c["in_place"] == (c["route"] == "in_place") or c["route"] == "copy"
    zero = _twice(fi.zero_cases, fi.SEED + 32)
    assert {np.dtype(c["dtype"]) for c in zero} == {np.dtype(d) for d in fi.PLANE_NP}
    rem = {r["img"].size % 16 for c in zero for r in c["runs"]}
    assert rem == set(range(16))
    assert all({np.dtype(r["seg"].dtype) for r in c["runs"]} == {np.dtype(d) for d in fi.SEG_NP} for c in zero)


def test_cellquant_generator():
    cases = _twice(fi.cellquant_cases, fi.SEED + 33)
    assert {c["route"] for c in cases} == set(fi.CELLQUANT_ROUTES)
    for c in cases:
        sizes = c["sizes"][1:] if (c["seg"] == 0).any() else c["sizes"]
        if c["route"] == "pairwise":
            assert c["pairwise"]
            assert sizes.max() >= 8191
        if c["route"] == "fold_wide":
            assert not c["pairwise"] and c["c"] >= 63
        if c["route"] == "nuc_overflow":
            assert c["overflow"], (c["max_nuclei"], c["cap"])
        if c["route"] == "nuc_other_route":
            assert c["nuc"] is not None and not c["force_search"]
            assert c["cell_lut"] != c["nuc_lut"], (c["cell_lut"], c["nuc_lut"])
        if c["keys"] is not None:
            present = np.unique(c["seg"][c["seg"] != 0]).astype(np.int64)
            assert np.all(np.isin(c["keys"], present)) and c["keys"].size < present.size
    assert any(c["walks"] >= 3 for c in cases) or any(c["c"] > 128 for c in cases)
    assert sum(c["sizes"].size for c in cases) <= N * 3000
