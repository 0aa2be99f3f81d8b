"""The case generators of the randomised sweeps (test_gpu_fuzz_parity.py: metric assign / online training;
test_gpu_fuzz_images.py: K10 - K12; test_gpu_fuzz_preprocessing.py: K2 - K5 and the label kernels;
test_gpu_fuzz_neighborhood_sums.py: K24; test_gpu_fuzz_overlays.py: K29; test_gpu_fuzz_embed.py: K30) on CPU: the first
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


# ---- K24, K29 (test_gpu_fuzz_neighborhood_sums.py, test_gpu_fuzz_overlays.py) ----------------------------------------
def _same_value(va, vb, key=""):
    if isinstance(va, np.ndarray):
        assert isinstance(vb, np.ndarray) and va.dtype == vb.dtype and va.shape == vb.shape, key
        assert va.tobytes() == vb.tobytes(), key
    elif isinstance(va, dict):
        assert va.keys() == vb.keys(), key
        for k in va:
            _same_value(va[k], vb[k], "%s.%s" % (key, k))
    elif isinstance(va, (list, tuple)):
        assert len(va) == len(vb), key
        for k, (a, b) in enumerate(zip(va, vb)):
            _same_value(a, b, "%s[%d]" % (key, k))
    else:
        assert va == vb or (va != va and vb != vb), key


def _twice_deep(gen, seed, n):
    a, b = list(gen(seed, n)), list(gen(seed, n))
    assert len(a) == len(b) == n
    _same_value(a, b)
    return a


def test_neighborhood_sums_fold_starts_from_plus_zero():
    """The statement's fold is a plain float fold from +0.0 in row order (include/pxsom.h): members that are all -0.0 give
    +0.0, where numpy's own cumulative sum from the first member gives -0.0."""
    from tests import splda_reference as sr
    xy = np.zeros((3, 2))
    feats = np.array([[-0.0, 1e8, -0.0], [-0.0, 1.0, 0.0], [-0.0, -1e8, -0.0]])
    sums, counts = sr.neighborhood_sums(xy, feats, np.array([0, 3]), 1.0)
    assert counts.tolist() == [3, 3, 3]
    for row in sums:
        for t in range(3):
            acc = 0.0
            for v in feats[:, t]:
                acc = acc + float(v)
            assert row[t] == acc and np.signbit(row[t]) == np.signbit(acc)
        assert not np.signbit(row[0]) and not np.signbit(row[2]) and row[1] == 1.0
    assert np.signbit(feats.cumsum(axis=0)[-1, 0])           # what the fold from the first member gave


def test_neighborhood_sums_generator():
    from tests import splda_reference as sr
    from tests import test_gpu_fuzz_neighborhood_sums as fn
    assert fn.NS_CASES == len(fn.NS_CLASSES) == 40 or fq._ENV_CASES is not None
    cases = _twice_deep(fn.neighborhood_sums_cases, fq.SEED + 60, len(fn.NS_CLASSES))
    assert {c["cls"] for c in cases} == set(fn.NS_CLASSES)
    assert {(c["cls"][2], c["cls"][3]) for c in cases} == {(r, f) for r in fn.RADIUS_CLASSES for f in fn.FEAT_CLASSES}
    assert {c["cls"][0] for c in cases} == {"uniform", "lattice", "clumps", "rational", "tiny_fovs", "one_big"}
    assert sum(c["cls"][0] == "lattice" and c["cls"][2] == "exact" for c in cases) >= 2
    sizes = {m for c in cases for m in c["sizes"]}
    assert {0, 1, 255, 256, 257} <= sizes
    assert any(m % fn.kBlock % fn.kGroup for m in sizes if m > fn.kBlock), "no last tile that is no multiple of 32"
    assert {c["n_feat"] for c in cases} >= {0, 1, 7, 8, 9, 16, 17} and max(c["n_feat"] for c in cases) >= 65
    assert {c["feat_off"] % 2 for c in cases if c["n_feat"]} == {0, 1}            # 8 bytes, and 16
    order_matters = 0
    for c in cases:
        xy, seg, radius = c["xy"], c["seg"], c["radius"]
        assert seg[0] == 0 and seg[-1] == len(xy) and np.all(np.diff(seg) >= 0) and np.isfinite(xy).all()
        assert (c["feats"] is None) == (c["n_feat"] == 0)
        if c["feats"] is not None and c["feats"].size >= 400:      # (a table of a few cells need not hold every kind)
            f = c["feats"]
            assert np.isnan(f).any() and np.isposinf(f).any() and (np.signbit(f) & (f == 0)).any()
            mag = np.abs(f[np.isfinite(f) & (f != 0)])
            assert mag.min() < 1e-6 and mag.max() > 1e6 and (f < 0).any() and (f > 0).any()
        layout, _, rcls, _ = c["cls"]
        if layout == "lattice":                  # exact: the coordinates are integers times the scale
            k = xy / c["scale"]
            assert np.array_equal(k, np.rint(k)) and np.array_equal(k * c["scale"], xy)
        _, lt = sr.neighborhood_sums(xy, None, seg, radius, False)
        _, le = sr.neighborhood_sums(xy, None, seg, radius, True)
        a, b = c["big"]
        if rcls == "zero":
            assert radius == 0 and not lt.any() and (le >= 1).all()
        elif rcls == "below_all":                # only the cells on the same centroid
            same = np.array([np.sum(np.all(xy[int(s):int(e)] == xy[i], axis=1)) for s, e in zip(seg[:-1], seg[1:])
                             for i in range(int(s), int(e))], dtype=np.int64)
            assert np.array_equal(lt, same) and np.array_equal(le, same)
        elif rcls == "ten":                      # about ten in a FOV large enough to hold them: between 5 and 20 on average
            if b - a >= 40:
                assert 5 <= lt[a:b].mean() <= 20, (c["cls"], lt[a:b].mean())
            assert lt.max() <= 60
        elif rcls == "all":
            assert np.array_equal(lt, np.repeat(np.diff(seg), np.diff(seg))) and np.array_equal(lt, le)
        else:                                    # pairs lie exactly at the radius: in under "le", out under "lt"
            pts = xy[a:b]
            dx, dy = pts[:, None, 0] - pts[None, :, 0], pts[:, None, 1] - pts[None, :, 1]
            at = np.sqrt(dx * dx + dy * dy) == radius
            assert at.sum() >= 2 and np.array_equal(at, at.T), c["cls"]
            assert np.array_equal((le - lt)[a:b], at.sum(axis=1)), c["cls"]
            if layout == "lattice":              # the radius is a lattice distance: hypotenuse x step x scale, exactly
                assert radius / (c["step"] * c["scale"]) in {h[2] for h in fn.LATTICE_HYPOTENUSES}
                assert at.sum() >= 8
        if c["feats"] is not None and rcls in ("all", "exact") and b - a >= 40:
            # only the ascending-row order gives the statement's bits: the members of a row folded in descending order differ
            sums, _ = sr.neighborhood_sums(xy[a:b], c["feats"][a:b], np.array([0, b - a]), radius, True)
            members = c["feats"][a:b][sr._mask(xy[a:b], 0, np.float64(radius), True)]
            with np.errstate(invalid="ignore"):
                fwd = np.concatenate([np.zeros((1, members.shape[1])), members]).cumsum(axis=0)[-1]
                rev = np.concatenate([np.zeros((1, members.shape[1])), members[::-1]]).cumsum(axis=0)[-1]
            assert fq._same_bits(fwd, sums[0])
            both = np.isfinite(fwd) & np.isfinite(rev)
            if len(members) >= 8:
                assert (fwd[both] != rev[both]).any(), c["cls"]
                order_matters += 1
    assert order_matters >= 6


def test_overlay_generators():
    from tests import overlay_reference as ovr
    from tests import test_gpu_fuzz_overlays as fo
    cases = _twice_deep(fo.overlay_cases, fq.SEED + 70, fq.default_cases(fo.OVERLAY_CLASSES))
    assert len(cases) == 30
    assert {(c["cls"]["rgb_off"], c["w"] % 4) for c in cases} == {(a, b) for a in range(4) for b in range(4)}
    assert {c["cls"]["borders_off"] for c in cases} == {0, 1, 2, 3} == {c["cls"]["in_off"] for c in cases}
    assert {(c["cls"]["plane"], c["cls"]["seg"]) for c in cases} == {(p, s) for p in fo.PLANE_NP for s in fo.SEG_NP}
    assert {(c["cls"]["plane"], c["cls"]["range_cls"]) for c in cases} == {(p, r) for p in fo.PLANE_NP for r in fo.RANGE_CLASSES}
    assert {(b, c["modes"][b]) for c in cases for b in range(3)} == {(b, m) for b in range(3) for m in range(3)}
    assert {c["alt"] is None for c in cases} == {True, False}
    assert any(abs(c["h"] - 4) <= 1 for c in cases) and any(abs(c["h"] - 16) <= 1 for c in cases)
    assert any(abs(c["w"] - 256) <= 3 for c in cases) and any(abs(c["w"] - 512) <= 3 for c in cases)
    for c in cases:
        cls = c["cls"]
        assert c["w"] % 4 == cls["wmod"] and c["seg"].dtype == cls["seg"] and c["seg"].shape == (c["h"], c["w"])
        if c["alt"] is not None:
            assert c["alt"].dtype.itemsize != c["seg"].dtype.itemsize
        b = cls["byte"]
        lo, hi = c["ranges"][b]
        mode, plane = c["modes"][b], c["planes"][b]
        assert plane.dtype == cls["plane"] and not (plane.dtype.kind == "f" and np.isnan(plane).any())
        assert (mode == ovr.OVERLAY_RESCALE and lo < hi) or (mode == ovr.OVERLAY_CLIP and lo == hi)
        if cls["range_cls"] == "negative_lo":
            assert lo < 0 < hi
        elif cls["range_cls"] == "one_ulp":
            assert np.float32(lo) == lo and np.float32(hi) == hi and np.nextafter(np.float32(lo), np.float32(np.inf)) == hi
            if plane.dtype == np.float32:
                assert (plane == np.float32(lo)).any() and (plane == np.float32(hi)).any()
        elif cls["range_cls"] == "span_2_31":
            assert hi - lo > 2.0 ** 31 - 8
            if plane.dtype == np.int32:
                assert plane.min() < -2 ** 30 and plane.max() > 2 ** 30
        elif cls["range_cls"] == "clip_below_0":
            assert lo == hi < 0 and (ovr.compose(c["planes"], c["modes"], c["ranges"], np.zeros_like(c["seg"]))[..., b] == 0).all()
        elif cls["range_cls"] == "clip_above_255":
            assert lo == hi > 255 and (ovr.compose(c["planes"], c["modes"], c["ranges"], np.zeros_like(c["seg"]))[..., b] == 255).all()
        # compose is what overlay is made of: the percentile ranges of a plane give overlay's bytes
        if cls["range_cls"] == "percentile":
            alone = ovr.compose([None, None, plane], [0, 0, mode], [(0, 0), (0, 0), (lo, hi)], c["seg"], c["alt"])
            assert np.array_equal(alone, ovr.overlay(plane, c["seg"], c["alt"]))

    cases = _twice_deep(fo.colorize_cases, fq.SEED + 71, fq.default_cases(fo.COLORIZE_CLASSES))
    assert {(c["cls"]["mask_off"], c["cls"]["out_off"]) for c in cases} >= {(a, b) for a in range(4) for b in range(4)}
    assert {c["route"] for c in cases} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(c["cls"]["out_off"], c["mask"].size % 4) for c in cases if not c["cls"]["bad"]} == {(a, b) for a in range(4) for b in range(4)}
    assert {c["mask"].dtype.type for c in cases} == set(fo.COLORIZE_MASK_NP) and {c["table"].shape[1] for c in cases} == {3, 4}
    assert {len(c["table"]) for c in cases} >= {1, 2, 255, 256, 70000}
    assert {c["mask"].dtype.type for c in cases if len(c["table"]) == 70000} >= {np.uint16, np.int32}
    for c in cases:
        assert c["route"] == fo.colorize_route(c["cls"]["mask_off"], c["cls"]["out_off"]) == (
            c["cls"]["mask_off"] == 0, c["cls"]["out_off"] == 0)
        idx = c["mask"].astype(np.int64)
        outside = (idx < 0) | (idx >= len(c["table"]))
        assert outside.any() == c["cls"]["bad"] and (not c["cls"]["bad"] or all(outside[y, x] for y, x in c["bad_at"]))
        assert (~outside).any()
    assert sum(c["cls"]["bad"] for c in cases) == 4

    cases = _twice_deep(fo.listq_cases, fq.SEED + 72, fq.default_cases(fo.LISTQ_CLASSES))
    assert [c["cls"] for c in cases] == list(fo.LISTQ_CLASSES)
    assert {c["x"].shape[1] for c in cases} >= {1, 47, 48, 49, 97} and {len(c["q"]) for c in cases} == {1, 2, 3, 4}
    assert {c["keep_mode"] for c in cases} == {0, 1, 2} and any(c["off"] and c["pad"] for c in cases)
    for c in cases:
        x, q, mode = c["x"], c["q"], c["keep_mode"]
        assert x.dtype == np.float32 and all(0 <= v <= 100 for v in q)
        kept = [fq.quantile_kept(np.ascontiguousarray(x[:, j]), mode) for j in range(x.shape[1])]
        if c["cls"] in ("m0", "m1", "m2"):
            assert kept[0].size == int(c["cls"][1])
        elif c["cls"] == "q_integral":
            assert (q[0] / 100 * (kept[0].size - 1)) % 1 == 0 and 0 < q[0] < 100
        elif c["cls"] == "two_values":
            assert all(np.unique(k).size == 2 for k in kept)
        elif c["cls"] == "all_equal":
            assert all(k.size and np.unique(k).size == 1 for k in kept)
        elif c["cls"] == "dup_straddle":
            lo = int(np.floor(q[0] / 100 * (x.shape[0] - 1)))
            assert all(np.sort(k)[lo] == np.sort(k)[lo + 1] for k in kept)
        elif c["cls"] == "low_byte":
            assert np.unique(np.abs(x).view(np.uint32) >> 8).size == 1 and np.unique(x.view(np.uint32) & 0xFF).size > 8
        elif c["cls"] == "mixed_sign":
            assert (x < 0).any() and (x > 0).any()
        elif c["cls"] == "subnormals":
            assert (np.abs(x[x != 0]) < np.finfo(np.float32).tiny).any()
        # the statement of tests/overlay_reference.py is numpy's own result for a list of q
        want = fo.listq_reference(x, q, mode)
        for j, k in enumerate(kept):
            if k.size:
                assert np.array_equal(ovr.percentile_listq_f32(k, q), want[:, j]), (c["cls"], j)
            else:
                assert np.isnan(want[:, j]).all()


# ---- K30 (test_gpu_fuzz_embed.py) --------------------------------------------------------------------------------------
def test_embed_generators():
    from tests import test_gpu_fuzz_embed as fe
    from tests import tsne_reference as ts
    cases = _twice_deep(fe.sqdist_cases, fq.SEED + 80, fq.default_cases(fe.SQDIST_CLASSES))
    assert [c["cls"] for c in cases] == list(fe.SQDIST_CLASSES)
    assert {(c["cls"][0], c["cls"][1]) for c in cases} == {(n, k) for n in fe.SQDIST_N for k in fe.SQDIST_C}
    assert {(c["cls"][2], c["x"].dtype.type) for c in cases} == {(v, d) for v in fe.SQDIST_VALUES for d in (np.float32, np.float64)}
    assert {1, 15, 16, 17, 33} <= {c["x"].shape[0] for c in cases} and any(c["x"].shape[0] > 33 for c in cases)
    for c in cases:
        x, vcls = c["x"], c["cls"][2]
        assert x.shape[1] == c["cls"][1] and np.isfinite(x).all()
        if vcls == "offset":                      # the columns' offsets dwarf the differences
            assert np.all(np.abs(x).min(axis=0) > x.max(axis=0) - x.min(axis=0)) and np.abs(x).min() > 900
        elif vcls == "duplicates" and x.shape[0] > 1:
            d = ts.pair_sqdist_f32(x)
            assert (d == 0).sum() > x.shape[0]
        elif vcls == "scale_1e-6":
            assert np.abs(x).max() < 1e-4
        elif vcls == "scale_1e6":
            assert np.abs(x).max() > 1e5 or x.size < 4
        elif vcls == "integers":
            assert np.array_equal(x, np.rint(x))
    cases = _twice_deep(fe.moment_cases, fq.SEED + 81, fq.default_cases(fe.MOMENT_CLASSES))
    rows = [c["x"].shape[0] for c in cases]
    assert {65535, 65536, 65537} <= set(rows) and rows.count(1 << 20) == 1 and any(65537 < n <= 70000 for n in rows)
    assert {(c["x"].shape[1], c["x"].dtype.type) for c in cases} == {(k, d) for k in (2, 3) for d in (np.float32, np.float64)}
    for c in cases:
        n = c["x"].shape[0]
        assert c["trips"] == fe.moment_trips(n) and (c["trips"] >= 2) == (n > 65536)
    assert fe.moment_trips(1 << 20) == 16 and ((1 << 20) // fe.kMomentRows) * 8 == 32 * 1024

    cases = _twice_deep(fe.affinity_cases, fq.SEED + 82, fq.default_cases(fe.AFFINITY_CLASSES))
    assert [c["cls"] for c in cases] == list(fe.AFFINITY_CLASSES)
    assert {(c["cls"][0], c["cls"][1]) for c in cases} == {(d, r) for d in fe.AFFINITY_DATA for r in fe.AFFINITY_ROWS}
    assert {(c["cls"][0], c["cls"][2]) for c in cases} == {(d, p) for d in fe.AFFINITY_DATA for p in fe.AFFINITY_PERPLEXITY}
    assert {(c["cls"][1], c["cls"][2]) for c in cases if c["cls"][1] != 2} == {
        (r, p) for r in fe.AFFINITY_ROWS if r != 2 for p in fe.AFFINITY_PERPLEXITY}
    rows = {c["d32"].shape[0] for c in cases}
    assert {2, 3} <= rows and rows & {31, 32, 33} and rows & {63, 64, 65} and rows & {511, 512, 513} and max(rows) <= 600
    smallest = np.inf
    for c in cases:
        n, data, perp = c["d32"].shape[0], c["cls"][0], c["perplexity"]
        assert c["d32"].dtype == np.float32 and np.array_equal(c["d32"], ts.pair_sqdist_f32(c["x"])) and c["ws_off"] % 2 == 0
        assert 1.01 <= perp <= max(1.01, 0.98 * (n - 1)) and (n > 2 or perp == 1.01)
        assert perp == {"low": 1.01, "high": max(1.01, 0.98 * (n - 1))}.get(c["cls"][2], perp)
        off = c["d32"][~np.eye(n, dtype=bool)]
        if data == "lattice":
            assert np.array_equal(c["x"], np.rint(c["x"])) and (n <= 3 or (off == 0).any())
        elif data == "outliers":
            assert off.max() > 1e6 * max(np.median(off), 1e-30) or n < 4
        elif data == "scale_1e-6_f32":
            assert c["x"].dtype == np.float32 and off.max() < 1e-8
        elif data == "scale_1e6":
            assert off.max() > 1e12
        # no row of the default seed's cases sits within the rounding bound of a branch of its search
        margins = ts.conditional_p(c["d32"], perp, margin=True)[3]
        assert margins.min() > 1, (c["cls"], margins.min())
        smallest = min(smallest, margins.min())
    assert smallest > 100

    cases = _twice_deep(fe.step_cases, fq.SEED + 83, fq.default_cases(fe.STEP_CLASSES))
    assert {(c["cls"]["even"], c["cls"]["aligned"], c["cls"]["scale"], c["cls"]["p"]) for c in cases} == {
        (a, b, s, p) for a in (False, True) for b in (False, True) for s in fe.STEP_SCALES for p in fe.STEP_P}
    assert {(c["route"], c["cls"]["want_error"], c["cls"]["grad"]) for c in cases} == {
        (a, b, g) for a in (False, True) for b in (False, True) for g in (False, True)}
    assert {c["cls"]["e"] for c in cases} == {1.0, 12.0}
    for c in cases:
        n, cls, P = len(c["Y"]), c["cls"], c["P"]
        # VEC exactly when n is even and P is 16-byte aligned: an odd number of doubles into an aligned buffer is 8 mod 16
        assert (n % 2 == 0) == cls["even"] and (c["p_off"] % 2 == 0) == cls["aligned"]
        assert c["route"] == fe.step_route(n, c["p_off"]) == (cls["even"] and cls["aligned"])
        assert np.array_equal(P, P.T) and np.all(np.diag(P) == ts.EPS) and P.min() >= ts.EPS and c["ws_off"] % 2 == 0
        if cls["p"] == "uniform":
            assert np.unique(P[~np.eye(n, dtype=bool)]).size == 1
        elif cls["p"] == "eps_rows":
            assert (P == ts.EPS).all(axis=1).any()
        if cls["scale"] == 200.0:
            assert np.abs(c["Y"]).max() > 1e6
        else:
            assert np.abs(c["Y"]).max() < 10 * cls["scale"]
