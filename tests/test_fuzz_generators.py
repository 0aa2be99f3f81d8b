"""The case generators of the randomised sweeps (test_gpu_fuzz_parity.py: metric assign / online training;
test_gpu_fuzz_images.py: K10 - K12; test_gpu_fuzz_preprocessing.py: K2 - K5 and the label kernels) on CPU: the first
default run of cases of each -- 12, or the family's class count when that is larger -- lands in every route class it is
meant to visit, each case's class is the one the library's own rule gives for its parameters, and one seed gives the
same cases twice.  Where a sweep's reference is a numpy / scipy / pandas statement rather than the oracle, the oracle
is held to that statement here, on the cases both define."""
import numpy as np

from tests import test_gpu_fuzz_images as fi
from tests import test_gpu_fuzz_parity as fp
from tests import test_gpu_fuzz_preprocessing as fq

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


def _twice(gen, seed, n=N):
    a, b = list(gen(seed, n)), list(gen(seed, n))
    _same_cases(a, b)
    assert len(a) == n
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


# ---- test_gpu_fuzz_preprocessing.py -------------------------------------------------------------------------------
def _family(name):
    """The first default run of a family: every class visited, the same cases twice."""
    gen, salt, classes = fq.FAMILIES[name]
    n = fq.default_cases(classes)
    assert n == max(12, len(classes))
    cases = _twice(gen, fq.SEED + salt, n)
    assert {c["cls"] for c in cases} == set(classes), name
    assert [c["cls"] for c in cases] == [classes[i % len(classes)] for i in range(n)]
    return cases


def _both_settings(name, flag):
    """Two visits of every class of a family: each class meets both values of `flag` (the semantics or the dtype),
    except a class that fixes it by its suffix, whose partner class has the other one; so does the first visit of the
    classes listed per dtype."""
    gen, salt, classes = fq.FAMILIES[name]
    r = len(classes)
    seen = {}
    for c in gen(fq.SEED + salt, 2 * r):
        seen.setdefault(c["cls"], []).append(bool(flag(c)))
    for cls in classes:
        base, forced = fq._forced(cls)
        if forced is None:
            assert sorted(seen[cls]) == [False, True], (name, cls, seen[cls])
        else:
            assert seen[cls] == [forced, forced] and seen[base + ("_f64" if forced else "_f32")] == [not forced] * 2


def test_alternate_flag():
    """Odd and even class counts alike: neighbours differ within a visit, and a class flips between visits."""
    assert [fq._alternate(i, 5) for i in range(10)] == [False, True, False, True, False, True, False, True, False, True]
    assert [fq._alternate(i, 4) for i in range(8)] == [False, True, False, True, True, False, True, False]


def test_blur_hwc_generator(oracle):
    from scipy import ndimage
    cases = _family("blur_hwc")
    want_route = {"fast": "fast", "fast_h17": "fast", "fast_h16": "generic", "fast_w9": "fast", "fast_w8": "generic",
                  "strip_edge": "fast", "tile_edge": "fast", "colblock_edge": "fast", "wide_c256": "fast",
                  "wide_c257": "generic", "other_radius": "generic", "short_image": "generic", "radius_64": "generic",
                  "radius_65": "refused"}
    _both_settings("blur_hwc", lambda c: c["f32"])
    hostile = {c["f32"]: c["img"] for c in cases if c["cls"].startswith("hostile_values")}
    assert set(hostile) == {False, True}                        # both in the first default run
    with np.errstate(over="ignore"):                            # the float32 semantics reach inf by rounding
        assert np.isinf(hostile[True][np.abs(hostile[True]) == 1e300].astype(np.float32)).all()
    assert any(c["route"] == "fast" and c["img"].shape[0] % 8 and c["img"].shape[1] % 8 for c in cases)
    for c in cases:
        h, w, ch = c["img"].shape
        if c["cls"] == "fast":
            assert h % 8 and w % 8                             # a grid that is no multiple of 8
        assert c["route"] == fq.blur_route(h, w, ch, c["radius"]) and c["radius"] == fq.blur_radius(c["sigma"])
        if c["cls"] in want_route:
            assert c["route"] == want_route[c["cls"]], c["cls"]
        assert c["img"].size <= 2_000_000
        if c["cls"] == "strip_edge":
            assert h in (63, 64, 65, 128, 129)
        if c["cls"] == "tile_edge":
            assert w * ch in (1023, 1024, 1025, 2047, 2048, 2049)
        if c["cls"] == "colblock_edge":
            assert w * ch in (255, 256, 257)
        if c["cls"] == "short_image":
            assert min(h, w) * 2 <= c["radius"]                # the reflection folds more than once
        if c["cls"] == "other_radius":
            assert c["radius"] in (0, 2, 4, 12)
        if c["cls"] == "radius_64":
            assert c["radius"] == fq.kMaxRadius
        if c["cls"].startswith("hostile_values"):
            assert c["f32"] == fq._forced(c["cls"])[1]
            assert np.isnan(c["img"]).any() and np.isinf(c["img"]).any() and (np.abs(c["img"]) == 1e300).any()
            continue
        if c["f32"]:
            assert np.array_equal(c["img"], c["img"].astype(np.float32).astype(np.float64))
        if c["route"] == "refused":
            continue
        # the oracle against scipy itself, with test_fuzz_preprocessing's bars
        want = oracle.gaussian_blur_hwc(c["img"], c["sigma"], f32=c["f32"])
        for j in range(ch):
            if c["f32"]:
                ref = ndimage.gaussian_filter(c["img"][:, :, j].astype(np.float32), c["sigma"])
                assert np.array_equal(want[:, :, j].astype(np.float32), ref), (c["i"], c["cls"], j)
            else:
                np.testing.assert_allclose(want[:, :, j], ndimage.gaussian_filter(c["img"][:, :, j], c["sigma"]),
                                           rtol=1e-13, atol=1e-300, err_msg="case %d %s" % (c["i"], c["cls"]))
    assert fq.blur_route(17, 9, 256, 8) == "fast" and fq.blur_route(16, 9, 1, 8) == "generic"
    assert fq.blur_route(17, 8, 1, 8) == "generic" and fq.blur_route(17, 9, 257, 8) == "generic"
    assert fq.blur_route(50, 50, 1, 7) == "generic" and fq.blur_route(5, 5, 1, 65) == "refused"


def _pandas_rowfilter(x, thresh, f32):
    """The reference's own statement, step by step (create_fov_pixel_data, normalize_rows): the frame with its
    metadata column, sum(axis=1) of the channel columns, the two masks, the division by the new sums."""
    import pandas as pd
    channels = ["ch%03d" % j for j in range(x.shape[1])]
    pixel_mat = pd.DataFrame(x.astype(np.float32) if f32 else x, columns=channels)
    pixel_mat["pixel"] = np.arange(x.shape[0])
    with np.errstate(all="ignore"):
        rowsums = pixel_mat[channels].sum(axis=1)
        pixel_mat = pixel_mat.loc[rowsums > thresh, :].reset_index(drop=True)
        pixel_mat = pixel_mat.loc[(pixel_mat[channels] != 0).any(axis=1), :].reset_index(drop=True)
        sub = pixel_mat[channels]
        sub = sub.div(sub.sum(axis=1), axis=0)
    return sub.values.astype(np.float64).reshape(-1, x.shape[1]), pixel_mat["pixel"].values.astype(np.int64)


def test_rowfilter_generator(oracle):
    cases = _family("rowfilter")
    _both_settings("rowfilter", lambda c: c["f32"])
    assert {c["route"] for c in cases} == {"staged", "staged_raised", "direct"}
    want_route = {"c1": "staged", "c30": "staged_raised", "c31": "staged_raised", "c72": "staged_raised",
                  "c73": "direct", "c128": "direct"}
    for c in cases:
        x = c["x"]
        n, ch = x.shape
        assert c["route"] == fq.rowfilter_route(ch) and c["sweeps"] == fq.rowfilter_scan_sweeps(n)
        if c["cls"] in want_route:
            assert ch == int(c["cls"][1:]) and c["route"] == want_route[c["cls"]]
        if c["cls"][0] == "n" and c["cls"][1:].isdigit():
            assert n == int(c["cls"][1:])
        if c["f32"]:
            assert np.array_equal(x, x.astype(np.float32).astype(np.float64), equal_nan=True)
        with np.errstate(all="ignore"):
            wr, wk = oracle.rowsum_filter_normalize(x, c["thresh"], sum_mode=2 if c["f32"] else 0)
        if c["cls"] == "none_kept":
            assert wk.size == 0 and n > 0
        if c["cls"] == "all_kept":
            assert wk.size == n
        if c["cls"] == "one_per_block":
            assert wk.size == (n + 255) // 256 and np.array_equal(np.unique(wk // 256), np.arange(wk.size))
        if c["cls"] == "last_only":
            assert np.array_equal(wk, [n - 1])
        if c["cls"] == "thresh_equal":
            r = c["equal_row"]
            assert fq.seq_row_sum(x[r], c["f32"]) == c["thresh"] and r not in wk
            assert 0 < wk.size < n
        if c["cls"] == "neg_thresh":
            assert c["thresh"] < 0
        if c["cls"] == "nan_rows":
            assert np.isnan(x).any(axis=1).sum() > np.isnan(x).all(axis=1).sum() > 0
            assert np.isnan(x[wk]).any(), "no kept row holds a NaN"
        if c["cls"] == "inf_rows":
            assert np.isinf(x[wk]).any()
        if c["cls"] == "cancel":
            assert ((x != 0).any(axis=1) & (x.sum(axis=1) == 0)).any()
        if c["cls"] == "negzero_rows":
            zero_rows = ~(x != 0).any(axis=1)
            assert (zero_rows & np.signbit(x).all(axis=1)).any() and not np.isin(np.flatnonzero(zero_rows), wk).any()
        # the oracle against pandas: every case, NaN and infinite rows included
        pr, pk = _pandas_rowfilter(x, c["thresh"], c["f32"])
        assert np.array_equal(wk, pk), (c["i"], c["cls"], wk.size, pk.size)
        assert fq._same_bits(wr, pr), (c["i"], c["cls"])
    assert fq.rowfilter_route(29) == "staged" and fq.rowfilter_route(30) == "staged_raised"
    assert fq.rowfilter_scan_sweeps(262144) == 1 and fq.rowfilter_scan_sweeps(262145) == 2
    assert fq.rowfilter_scan_sweeps(0) == 0


def test_quantile_generator(oracle):
    import pandas as pd
    cases = _family("quantile")
    _both_settings("quantile", lambda c: c["x"].dtype == np.float32)
    f32_negative = [c["cls"] for c in cases if c["x"].dtype == np.float32 and c["keep_mode"] != 1 and (c["x"] < 0).any()]
    assert {"all_negative_f32", "mixed_sign_f32", "dup_straddle_f32", "low_byte_f32"} <= set(f32_negative)
    assert {c["keep_mode"] for c in cases} == {0, 1, 2}
    chunks = {"c1": (1, 1), "c47": (1, 47), "c48": (1, 48), "c49": (2, 1), "c96": (2, 48), "c97": (3, 1)}
    for c in cases:
        x, q, mode, (cls, forced) = c["x"], c["q"], c["keep_mode"], fq._forced(c["cls"])
        n, ch = x.shape
        assert forced is None or (x.dtype == np.float32) == forced, c["cls"]
        assert c["chunks"] == fq.quantile_chunks(ch) and c["passes"] == fq.quantile_passes(x.dtype.itemsize)
        assert 0.0 <= q <= 1.0 and 1 <= ch <= 65535
        kept0 = fq.quantile_kept(x[:, 0], mode)
        if cls in chunks:
            assert c["chunks"] == chunks[cls]
        if cls == "ldx_view":
            assert c["off"] > 0 and c["pad"] > 0
        if cls[0] == "n" and cls[1:].isdigit():
            assert n == int(cls[1:])
        if cls == "n_large":
            assert n > 20 * fq.kQRows
        if cls in ("m0", "m1", "m2"):
            assert kept0.size == int(cls[1])
        if cls in fq._Q_VALUES:
            assert q == fq._Q_VALUES[cls]
        if cls == "q_integral":
            assert kept0.size == n and (q * (n - 1)) % 1 == 0 and 0 < q * (n - 1) < n - 1
            assert np.float32(n - 1) * np.float32(q) == q * (n - 1)
        if cls in ("mode0", "mode1", "mode2"):
            assert mode == int(cls[4])
        if cls == "all_negative":
            assert kept0.size and (kept0 < 0).all()
        if cls == "mixed_sign":
            assert (kept0 < 0).any() and (kept0 > 0).any()
        if cls == "pm_zero":
            assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
        if cls == "subnormals":
            assert ((x != 0) & (np.abs(x) < np.finfo(x.dtype).tiny)).any()
        if cls == "inf_among_finite":
            assert np.isinf(x).any() and np.isfinite(x).any()
        if cls == "nans":
            assert np.isnan(x).mean() > 0.1
        if cls == "two_values":
            assert np.unique(x).size == 2
        if cls == "all_equal":
            assert np.unique(x).size == 1
        if cls == "dup_straddle":
            srt = np.sort(kept0)
            lo = int(np.floor(q * (srt.size - 1)))
            assert srt[lo] == srt[min(lo + 1, srt.size - 1)] and np.unique(srt).size > 1
            assert srt.size >= 3 and (q * (srt.size - 1)) % 1 != 0       # ranks lo and hi = lo + 1 both count
        bits = x.view(fq._bits_dtype(x.dtype))
        mant = 52 if x.dtype == np.float64 else 23
        if cls == "low_byte":
            assert np.unique(bits >> 8 << 8 << 1).size == 1 and np.unique(bits & 0xFF).size > 1
        if cls == "exponent_only":
            assert np.unique(bits & ((1 << mant) - 1)).size == 1 and np.unique(bits >> mant).size > 2
        # the oracle and pandas against the numpy statement, binary64, where every kept value is finite
        if x.dtype != np.float64 or np.isinf(x).any():
            continue
        want = fq.quantile_reference(x, q, mode)
        got = np.array([oracle.quantile_nonzero(np.ascontiguousarray(x[:, j]), q, mode) for j in range(ch)])
        assert fq._same_numbers(got, want), (c["i"], cls)
        if mode == 0 and n > 0:
            with np.errstate(all="ignore"):
                pq = pd.DataFrame(x).replace(0, np.nan).quantile(q).values
            assert fq._same_numbers(pq, fq.quantile_reference(x, (q * 100.0) / 100.0, 0)), (c["i"], cls)
    assert np.isnan(fq.quantile_reference(np.zeros((0, 2)), 0.5, 2)).all()
    with np.errstate(all="ignore"):                  # numpy's own NaN where its interpolation meets inf - inf
        got = [np.quantile(np.array([1, np.inf, np.inf, 2, -np.inf]), q) for q in (0, 0.3, 0.5, 0.9, 1)]
    assert np.isnan(got[0]) and got[1] == 1.2 and np.isnan(got[2:]).all()


def test_scaled_rowsum_generator():
    cases = _family("scaled_rowsum")
    _both_settings("scaled_rowsum", lambda c: c["img"].dtype == np.float32)
    for c in cases:
        ch, cls = c["img"].shape[1], c["cls"]
        assert c["route"] == fq.scaled_rowsum_route(ch) and c["norm"].dtype == c["img"].dtype
        if cls[0] == "c" and cls[1:].split("_")[0].isdigit():
            assert ch == int(cls[1:].split("_")[0])
        assert (c["route"] == "refused") == (cls == "c129_refused")
        if cls == "ldx_view":
            assert c["off"] > 0 and c["pad"] > 0
        if cls == "zero_divisor":
            assert (c["norm"] == 0).sum() == 1
        if cls == "inf_divisor":
            assert np.isinf(c["norm"]).sum() == 1
    assert fq.scaled_rowsum_route(7) == "sequential" and fq.scaled_rowsum_route(8) == "unrolled_tail0"
    assert fq.scaled_rowsum_route(127) == "unrolled_tail7" and fq.scaled_rowsum_route(129) == "refused"


def test_normalize_columns_generator(oracle):
    cases = _family("normalize_columns")
    for c in cases:
        cls, (n, ch) = c["cls"], c["x"].shape
        ldx, ldo = c["in_off"] + ch + c["in_pad"], c["out_off"] + ch + c["out_pad"]
        if cls == "ldx_ne_ldo":
            assert ldx != ldo
        if cls == "in_place":
            assert c["in_place"] and ldx == ldo
        if cls == "out_padded":
            assert ldo > ch and c["out_off"] > 0 and c["out_pad"] > 0
        if cls == "n0":
            assert n == 0
        if cls.endswith("_divisor"):
            bad = {"zero": c["norm"] == 0, "nan": np.isnan(c["norm"]), "inf": np.isinf(c["norm"])}[cls.split("_")[0]]
            assert bad.sum() == 1
        if n and np.isfinite(c["x"]).all() and np.isfinite(c["norm"]).all() and (c["norm"] != 0).all():
            assert fq._same_bits(oracle.normalize_columns(c["x"], c["norm"]), c["x"] / c["norm"][None, :])


def test_label_kernel_generator(oracle):
    cases = _family("label_kernel")
    routes = set()
    for c in cases:
        cls = c["cls"]
        if c["kind"] == "relabel":
            size = c["lut"].size
            assert size == {"relabel_lut1": 1, "relabel_lut16384": fq.RELABEL_MAX_LUT,
                            "relabel_lut16385": fq.RELABEL_MAX_LUT + 1}.get(cls, size)
            for r in c["runs"]:
                assert r["route"] == fq.relabel_route(size, r["in_off"], r["in_off"] if c["in_place"] else r["out_off"])
                assert (r["route"] == "refused") == (cls == "relabel_lut16385")
                assert ((r["labels"] < 0) | (r["labels"] >= size)).any() or size > 16000
                routes.add(r["route"])
            if cls == "relabel_offsets":
                assert {(r["in_off"], r["out_off"]) for r in c["runs"]} == {(a, b) for a in range(4) for b in range(4)}
                for a in range(4):
                    assert {r["n"] % 4 for r in c["runs"] if r["in_off"] == a} == {0, 1, 2, 3}
                assert {r["n"] % 4 for r in c["runs"] if r["route"] == "vector"} == {0, 1, 2, 3}
            want = fq.relabel_reference(c["runs"][0]["labels"], c["lut"], c["fill"])
            assert want.dtype == np.int32 and want.shape == c["runs"][0]["labels"].shape
        elif c["kind"] == "hist":
            a, b, na, nb = c["a"], c["b"], c["na"], c["nb"]
            want = fq.pair_histogram_reference(a, b, na, nb, c["start"])
            assert np.array_equal(want - c["start"], oracle.pair_histogram(a, b, na, nb)), cls
            inside = (a >= 0) & (a < na) & (b >= 0) & (b < nb)
            if cls == "hist_one_bin":
                assert np.count_nonzero(want - c["start"]) == 1 and inside.all()
            if cls == "hist_out_of_range":
                assert not inside.all() and inside.any()
            if cls == "hist_accumulate":
                assert c["start"].any()
            if cls == "hist_n0":
                assert a.size == 0
        else:
            pos = c["row_index"] * c["w"] + c["column_index"]
            assert (pos >= 0).all(), "numpy wraps a negative flat position where the kernel reports PXSOM_MASK_BAD_PIXEL"
            assert c["status"] == fq.cluster_mask_status(c["row_index"], c["column_index"], c["labels"], c["lut"],
                                                         c["h"], c["w"])
            assert c["status"] == {"mask_bad_label": fq.PXSOM_MASK_BAD_LABEL,
                                   "mask_bad_pixel": fq.PXSOM_MASK_BAD_PIXEL}.get(cls, 0), cls
            if cls == "mask_one_pixel":
                assert np.unique(pos).size == 1 and pos.size >= 1
            if cls == "mask_n0":
                assert pos.size == 0
            if cls == "mask_wide_ids":
                ids = c["lut"][c["labels"]]
                assert (np.abs(ids) > 32767).any()
                want = fq.cluster_mask_reference(c["row_index"], c["column_index"], c["labels"], c["lut"], c["h"], c["w"])
                assert want.dtype == np.int16
    assert routes == {"vector", "scalar", "refused"}
    assert fq.relabel_route(16384, 0, 4) == "vector" and fq.relabel_route(5, 0, 1) == "scalar"
    assert fq.relabel_route(0, 0, 0) == "refused"


def test_absmax_generator():
    cases = _family("absmax")
    for c in cases:
        cls, x = c["cls"], c["x"]
        for dt in fq.ABSMAX_NP:                      # every storage type holds the values
            assert np.array_equal(x.astype(dt).astype(np.float64), x, equal_nan=True)
        want = fq.absmax_reference(x)
        if cls == "ldx_view":
            assert c["off"] > 0 and c["pad"] > 0
        if cls == "negative_largest":
            assert want == 1000.5 and x.max() < 1000.5
        if cls == "nonfinite_among_finite":
            assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any() and 0 < want <= 1000
        if cls == "no_finite":
            assert x.size and want == 0.0
        if cls == "n0":
            assert x.shape[0] == 0 and want == 0.0


def test_cluster_sums_generator(oracle):
    cases = _family("cluster_sums")
    assert {r for c in cases for r in c["routes"].values()} == {"atomic", "atomic_vector", "private", "pairs"}
    want_route = {"c13": "private", "c63": "private", "n32768": "pairs", "odd_ldx": "private", "even_ldx": "pairs",
                  "base_plus_one": "private"}
    for c in cases:
        cls, x, k = c["cls"], c["x"], c["k"]
        n, ch = x.shape
        ldx = c["off"] + ch + c["pad"]
        ldx = ch if c["flat"] else ldx
        assert c["ldx"] == ldx and c["flat"] == cls.startswith("flat_")
        assert c["routes"] == {s: fq.cluster_sums_route(n, ch, ldx, c["off"], k, s) for s in (2, 4, 8)}
        assert fq.sums_private_waves(40, k) > 0
        assert len({r.split("_")[0] for r in c["routes"].values()}) == 1          # only the vector loads look at the dtype
        if cls in want_route:
            assert set(c["routes"].values()) == {want_route[cls]}, cls
        if cls in ("c14", "c64"):
            assert set(c["routes"].values()) == {"pairs" if ldx % 2 == 0 and c["off"] % 2 == 0 else "private"}
        if cls in ("c12", "c65", "n32767"):
            assert c["routes"][8] == "atomic" and c["routes"][4] in ("atomic", "atomic_vector")
        if cls == "flat_aligned":      # contiguous rows on an aligned base: 16-byte loads for f32 and f16, never for f64
            assert c["routes"] == {2: "atomic_vector", 4: "atomic_vector", 8: "atomic"}
        if cls == "flat_moved":        # the same matrix moved by 1 .. 3 elements: the alignment test fails
            assert ldx == ch and 1 <= c["off"] <= 3 and set(c["routes"].values()) == {"atomic"}
        if cls == "odd_ldx":
            assert ldx % 2 == 1
        if cls == "base_plus_one":
            assert c["off"] == 1 and ldx % 2 == 0 and ch % 2 == 0
        assert np.array_equal(np.rint(x * 256), x * 256) and np.abs(x).max() <= 8
        for dt in fq.CLUSTER_SUMS_NP:
            assert np.array_equal(x.astype(dt).astype(np.float64), x)
        valid = (c["labels"] >= 1) & (c["labels"] <= k)
        if cls == "labels_mixed":
            lab = c["labels"]
            assert (lab == 0).any() and (lab == k + 1).any() and (lab < 0).any() and valid.any()
        if cls == "one_cluster":
            assert np.unique(c["labels"]).size == 1 and valid.all()
        if cls == "prefilled":
            assert c["sums0"].any() and c["counts0"].any()
        # exact sums: the oracle's left-to-right sums equal numpy's unordered ones
        ws, wc = oracle.cluster_sums(x, c["labels"], k)
        sums = np.zeros((k, ch))
        np.add.at(sums, c["labels"][valid].astype(np.int64) - 1, x[valid])
        assert np.array_equal(ws, sums) and np.array_equal(wc, np.bincount(c["labels"][valid] - 1, minlength=k))
        assert np.abs(ws + c["sums0"]).max() < 2 ** 29                # ... and stay exact on the prefilled tables
