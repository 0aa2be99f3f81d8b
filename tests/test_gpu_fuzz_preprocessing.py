"""Randomised parity sweep of the pre-processing and label kernels (csrc/pxsom_pre.hip: K2 blur [h, w, c], K3 row-sum
filter, K4 column normalisation, K5 quantile select, the scaled row sums, cluster mask and relabel; pxsom_pair_histogram,
pxsom_absmax and pxsom_cluster_sums with arbitrary labels), each against its plain reference -- the oracle, or live
numpy in the array's dtype -- by route class: case i of a generator takes class i % R of a fixed tuple, then draws the
rest within the entry's domain, so a default run visits every class (a family with more than 12 classes raises its
default count to R; tests/test_fuzz_generators.py checks the visits and each class against the library's rule on CPU).
Every buffer a kernel writes -- outputs, scratch, workspaces, padded outputs -- is a slice at a drawn element offset of
a larger buffer filled with a sentinel, and everything outside the slice must still hold the sentinel afterwards; entries
whose wrapper allocates its own outputs are called the way the wrapper calls them, through _capi.  No case is skipped; a
class that is a refusal asserts the documented status and untouched outputs.  NaNs are compared by position only.
``PXSOM_FUZZ_CASES`` / ``PXSOM_FUZZ_SEED`` as in test_gpu_fuzz_parity.py.  The generators are device-free."""
import os

import numpy as np
import pytest

from tests.test_gpu_fuzz_images import _bytes_equal, _guard_intact, _sentinel, _view1d, _view2d

pytestmark = pytest.mark.gpu

_ENV_CASES = os.environ.get("PXSOM_FUZZ_CASES")
SEED = int(os.environ.get("PXSOM_FUZZ_SEED", "20261017"))

PXSOM_OK, PXSOM_ERR_INVALID_ARG, PXSOM_ERR_UNSUPPORTED = 0, -1, -2     # include/pxsom.h


def default_cases(classes):
    """The default case count of a family: 12, or its class count when that is larger."""
    return max(12, len(classes))


def case_count(classes):
    return int(_ENV_CASES) if _ENV_CASES is not None else default_cases(classes)


def _same_bits(got, want):
    """Equal bit for bit wherever `want` is a number, NaN exactly where `want` is NaN (host and device may form
    different quiet NaNs)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    return _bytes_equal(got[~wn], want[~wn])


def _same_numbers(got, want):
    """Equal as numbers, or both NaN (the sign of a zero is not compared)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def _f32(flag):
    return "f32" if flag else "f64"


def _alternate(i, r):
    """A flag that differs between neighbouring classes and between successive visits of one class, whatever the
    parity of the class count r: the parity of (visit number + class number)."""
    return bool(((i // r) + (i % r)) % 2)


def _forced(cls):
    """(class, flag) of a class name that fixes the semantics / dtype by a suffix: ("x", True) for "x_f32", ("x",
    False) for "x_f64", else (cls, None).  A family lists a class whose values matter per dtype once with each
    suffix, so that the first default run meets both."""
    if cls.endswith("_f32") or cls.endswith("_f64"):
        return cls[:-4], cls.endswith("_f32")
    return cls, None


# ---- K2 pxsom_gaussian_blur_hwc -----------------------------------------------------------------------------------
kMaxRadius = 64                       # pxsom_pre.hip
BLUR_FAST_RADIUS, BLUR_FAST_MIN_H, BLUR_FAST_MIN_W, BLUR_FAST_MAX_C = 8, 17, 9, 256
BLUR_TY, BLUR_TX, BLUR_COLBLOCK = 64, 1024, 256
PXSOM_BLUR_GENERIC_FORM = 2
BLUR_HWC_CLASSES = ("fast", "fast_h17", "fast_h16", "fast_w9", "fast_w8", "strip_edge", "tile_edge", "colblock_edge",
                    "wide_c256", "wide_c257", "other_radius", "short_image", "radius_64", "radius_65",
                    "hostile_values_f32", "hostile_values_f64")
_TILE_WC = {1023: (1, 3, 11), 1024: (1, 2, 4, 8), 1025: (1, 5), 2047: (1, 23), 2048: (1, 2, 4, 8), 2049: (1, 3)}
_COLBLOCK_WC = {255: (1, 3, 5, 15, 17), 256: (1, 2, 4, 8, 16), 257: (1,)}


def blur_radius(sigma, truncate=4.0):
    return int(truncate * float(sigma) + 0.5)


def blur_route(h, w, c, radius):
    """pxsom_gaussian_blur_hwc: refused beyond kMaxRadius; the register-window / LDS-tile form at radius 8 on images of
    at least 17 rows, 9 columns and at most 256 channels; else the thread-per-output form."""
    if radius < 0 or radius > kMaxRadius:
        return "refused"
    if radius == BLUR_FAST_RADIUS and h >= BLUR_FAST_MIN_H and w >= BLUR_FAST_MIN_W and c <= BLUR_FAST_MAX_C:
        return "fast"
    return "generic"


def _blur_values(rs, h, w, c, f32, hostile):
    x = rs.gamma(0.5, 2.0, size=(h, w, c))
    x[rs.rand(h, w, c) < 0.4] = 0.0
    if hostile or rs.rand() < 0.3:
        x[rs.rand(h, w, c) < 0.3] *= -1.0
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    if hostile:          # +-1e300 and 1e-310 are no float32 values: under f32 semantics the first pass rounds them (to inf, 0)
        pool = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 1e-310, -7.5])
        for v in pool:
            for _ in range(int(rs.randint(1, 4))):
                x[rs.randint(0, h), rs.randint(0, w), rs.randint(0, c)] = v
    return x


def blur_hwc_cases(seed, count):
    """Cases of test_fuzz_blur_hwc: class i % 16 of BLUR_HWC_CLASSES (16 classes: the default run is 16 cases) -- the
    fast form inside, on a grid whose h and w are no multiples of 8; h = 17 (fast) and 16 (generic); w = 9 and 8; h on
    the strip edges of TY = 64; w * c on the tile edges of TX = 1024 and on the 256-element column blocks of the row
    pass; c = 256 (fast) and 257 (generic); sigma 0.1 / 0.5 / 1 / 3; an axis so short that the reflection folds more
    than once; radius 64 and the refused 65; hostile values under either semantics (float32: +-1e300 must round to
    inf) -- then shape, values, the semantics (alternating between the visits of a class) and the element offsets of
    image and scratch."""
    rs = np.random.RandomState(seed)
    r_cls = len(BLUR_HWC_CLASSES)
    for i in range(count):
        cls, forced = _forced(BLUR_HWC_CLASSES[i % r_cls])
        sigma = 2.0
        h, w, c = int(rs.randint(17, 160)), int(rs.randint(9, 160)), int(rs.randint(1, 9))
        if cls == "fast":
            h, w = h + (h % 8 == 0), w + (w % 8 == 0)
        elif cls == "fast_h17" or cls == "fast_h16":
            h = 17 if cls == "fast_h17" else 16
        elif cls == "fast_w9" or cls == "fast_w8":
            w = 9 if cls == "fast_w9" else 8
        elif cls == "strip_edge":
            h, w, c = int(rs.choice([63, 64, 65, 128, 129])), int(rs.randint(9, 60)), int(rs.randint(1, 7))
        elif cls in ("tile_edge", "colblock_edge"):
            table = _TILE_WC if cls == "tile_edge" else _COLBLOCK_WC
            wc = int(rs.choice(sorted(table)))
            c = int(rs.choice(table[wc]))
            w, h = wc // c, int(rs.randint(17, 60))
        elif cls in ("wide_c256", "wide_c257"):
            h, w, c = int(rs.randint(17, 25)), int(rs.randint(9, 15)), 256 if cls == "wide_c256" else 257
        elif cls == "other_radius":
            sigma = float(rs.choice([0.1, 0.5, 1.0, 3.0]))
            h, w = int(rs.randint(1, 90)), int(rs.randint(1, 90))
        elif cls == "short_image":
            sigma = float(rs.choice([2.0, 3.0, 5.0]))
            short = int(rs.randint(1, max(2, blur_radius(sigma) // 3 + 1)))
            h, w = (short, int(rs.randint(1, 60))) if rs.rand() < 0.5 else (int(rs.randint(1, 60)), short)
        elif cls in ("radius_64", "radius_65"):
            sigma = 16.0 if cls == "radius_64" else 16.125
            h, w, c = int(rs.randint(3, 80)), int(rs.randint(3, 80)), int(rs.randint(1, 4))
        elif cls == "hostile_values" and (i // r_cls) % 2:
            sigma = 1.0
        f32 = _alternate(i, r_cls) if forced is None else forced
        radius = blur_radius(sigma)
        yield dict(i=i, cls=BLUR_HWC_CLASSES[i % r_cls], sigma=sigma, radius=radius, f32=f32, route=blur_route(h, w, c, radius),
                   img=_blur_values(rs, h, w, c, f32, cls == "hostile_values"),
                   off=int(rs.randint(0, 4)), tail=int(rs.randint(0, 9)), tmp_off=int(rs.randint(0, 4)),
                   tmp_tail=int(rs.randint(0, 9)))


def test_fuzz_blur_hwc(gpu, oracle):
    """pxsom_gaussian_blur_hwc: the whole image against oracle.gaussian_blur_hwc bit for bit; a fast-form case again in
    the generic form, bit for bit; image and scratch inside sentinel buffers; radius 65 returns PXSOM_ERR_UNSUPPORTED
    and leaves both untouched."""
    import torch
    from ark_analysis_amd import _capi, som_device
    lib = _capi.lib()
    fill = _sentinel(np.float64)
    for case in blur_hwc_cases(SEED + 40, case_count(BLUR_HWC_CLASSES)):
        img = case["img"]
        h, w, c = img.shape
        tag = "case %d: class=%s route=%s %dx%dx%d sigma=%g %s off=%d tmp_off=%d (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], case["cls"], case["route"], h, w, c, case["sigma"], _f32(case["f32"]), case["off"],
            case["tmp_off"], SEED)
        weights, radius = som_device.gaussian_kernel1d(case["sigma"])
        assert radius == case["radius"], tag
        forms = [0, PXSOM_BLUR_GENERIC_FORM] if case["route"] == "fast" else [0]
        want = None if case["route"] == "refused" else oracle.gaussian_blur_hwc(img, case["sigma"], f32=case["f32"])
        for form in forms:
            ibuf, it = _view1d(gpu, img, case["off"], case["tail"], fill)
            tbuf, tt = _view1d(gpu, np.full(img.shape, fill), case["tmp_off"], case["tmp_tail"], fill)
            before = ibuf.cpu().numpy()
            rc = lib.pxsom_gaussian_blur_hwc(it.data_ptr(), tt.data_ptr(), h, w, c, weights.ctypes.data, radius,
                                             int(case["f32"]) | form, _capi.stream_ptr())
            torch.cuda.synchronize()
            t = tag + (" generic form" if form else "")
            if case["route"] == "refused":
                assert rc == PXSOM_ERR_UNSUPPORTED, t
                assert _bytes_equal(ibuf.cpu().numpy(), before), t + ": a refused call changed the image"
                assert _guard_intact(tbuf.cpu().numpy(), slice(0, 0), fill), t + ": a refused call wrote the scratch"
                continue
            assert rc == PXSOM_OK, t
            got = it.cpu().numpy()
            assert _same_bits(got, want), t + ": %d of %d elements differ" % (
                int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()), got.size)
            n = img.size
            assert _guard_intact(ibuf.cpu().numpy(), slice(case["off"], case["off"] + n), fill), t + ": image guard"
            assert _guard_intact(tbuf.cpu().numpy(), slice(case["tmp_off"], case["tmp_off"] + n), fill), t + ": scratch guard"


# ---- K3 pxsom_rowsum_filter_normalize -----------------------------------------------------------------------------
kRowBlock = 256                        # pxsom_pre.hip
ROWFILTER_STAGED_MAX_C = 72
ROWFILTER_DEFAULT_LDS = 64 * 1024
BLOCK_SCAN_WIDTH = 1024
ROWFILTER_CLASSES = ("interior", "c1", "c30", "c31", "c72", "c73", "c128", "n0", "n1", "n255", "n256", "n257",
                     "n262144", "n262145", "none_kept", "all_kept", "one_per_block", "last_only", "thresh_equal",
                     "neg_thresh", "nan_rows", "inf_rows", "cancel", "negzero_rows")


def rowfilter_route(c):
    """pxsom_rowsum_filter_normalize: rows staged in LDS up to c = 72 (256 rows of c | 1 doubles, the row sums and the
    kept list; past 64 KB -- from c = 30 on, where c | 1 = 31 -- with a raised dynamic-LDS limit), else thread per row."""
    if c > ROWFILTER_STAGED_MAX_C:
        return "direct"
    write_bytes = kRowBlock * (c | 1) * 8 + kRowBlock * 8 + kRowBlock * 2
    return "staged_raised" if write_bytes > ROWFILTER_DEFAULT_LDS else "staged"


def rowfilter_scan_sweeps(n):
    """1024-wide sweeps of block_scan_kernel over the (n + 255) / 256 workgroup counts."""
    nblocks = (n + kRowBlock - 1) // kRowBlock
    return (nblocks + BLOCK_SCAN_WIDTH - 1) // BLOCK_SCAN_WIDTH


def seq_row_sum(row, f32):
    """The row sum as pandas forms it: left to right in the frame's dtype, NaN skipped."""
    acc = np.float32(0) if f32 else np.float64(0)
    with np.errstate(all="ignore"):
        for v in row:
            v = np.float32(v) if f32 else np.float64(v)
            if v == v:
                acc = acc + v
    return float(acc)


def rowfilter_cases(seed, count):
    """Cases of test_fuzz_rowfilter: class i % 24 of ROWFILTER_CLASSES (24 classes: the default run is 24 cases) -- c on
    the edges of the three forms; n around a workgroup's 256 rows and around the second sweep of block_scan_kernel; the
    keep patterns; a threshold equal to a row's sum, a negative one, NaN rows, +inf rows, cancelling signs, rows of
    -0.0 -- then the rest, both semantics."""
    rs = np.random.RandomState(seed)
    r_cls = len(ROWFILTER_CLASSES)
    for i in range(count):
        cls = ROWFILTER_CLASSES[i % r_cls]
        f32 = _alternate(i, r_cls)
        c = int(rs.choice([1, 2, 3, 5, 8, 12, 22]))
        n = int(rs.randint(2, 3000))
        if cls[0] == "c" and cls[1:].isdigit():
            c = int(cls[1:])
        if cls[0] == "n" and cls[1:].isdigit():
            n = int(cls[1:])
            if n > 100000:
                c = int(rs.randint(1, 5))
        if cls in ("one_per_block", "last_only"):
            n = int(rs.choice([257, 1000, 5000]))
        if cls == "thresh_equal":
            n = max(n, 50)
        x = rs.gamma(0.5, 2.0, size=(n, c))
        x[rs.rand(n, c) < 0.4] = 0.0
        x[rs.rand(n) < 0.1] = 0.0
        thresh = float(rs.choice([0.0, 0.5, float(np.median(x.sum(1))) if n else 0.0]))
        if cls == "none_kept":
            thresh = 1e30
        elif cls == "all_kept":
            x = x + 0.25
            thresh = float(rs.choice([0.0, -1.0]))
        elif cls == "one_per_block":
            keep = np.array([b + int(rs.randint(0, min(kRowBlock, n - b))) for b in range(0, n, kRowBlock)])
            mask = np.zeros(n, bool)
            mask[keep] = True
            x[~mask] = 0.0
            x[mask] += 1.0
            thresh = 0.0
        elif cls == "last_only":
            x[:n - 1] = 0.0
            x[n - 1] += 1.0
            thresh = 0.0
        elif cls == "neg_thresh":
            x[rs.rand(n, c) < 0.2] *= -3.0
            thresh = float(rs.choice([-1.0, -0.5, -1e30]))
        elif cls == "nan_rows":
            rows = rs.rand(n) < 0.15
            x[rows[:, None] & (rs.rand(n, c) < 0.5)] = np.nan
            x[rs.rand(n) < 0.03] = np.nan
            x[0, 0] = np.nan
            thresh = float(rs.choice([0.0, -1.0, thresh]))
        elif cls == "inf_rows":
            x[(rs.rand(n) < 0.1)[:, None] & (rs.rand(n, c) < 0.5)] = np.inf
            x[0, 0] = np.inf
        elif cls == "cancel":
            x[rs.rand(n) < 0.5, 1:] = 0.0
            if c >= 2:
                rows = rs.rand(n) < 0.3
                x[rows, 1] = -x[rows, 0]
                x[rows, 2:] = 0.0
            else:
                x[rs.rand(n) < 0.3] *= -1.0
            thresh = float(rs.choice([-1.0, -1e-300]))
        elif cls == "negzero_rows":
            x[rs.rand(n) < 0.3] = -0.0
            x[0] = -0.0
            thresh = float(rs.choice([-1.0, 0.0]))
        if f32:
            x = x.astype(np.float32).astype(np.float64)
        equal_row = -1
        if cls == "thresh_equal":            # the test is strict: the row whose sum equals thresh is dropped
            sums = x.astype(np.float32).sum(1) if f32 else x.sum(1)
            equal_row = int(rs.choice(np.flatnonzero(sums > 0)))
            thresh = seq_row_sum(x[equal_row], f32)
        yield dict(i=i, cls=cls, x=np.ascontiguousarray(x), thresh=thresh, f32=f32, equal_row=equal_row,
                   route=rowfilter_route(c), sweeps=rowfilter_scan_sweeps(n),
                   rows_off=int(rs.randint(0, 4)), idx_off=int(rs.randint(0, 4)), cnt_off=int(rs.randint(0, 4)),
                   ws_off=int(rs.randint(0, 8)))


def _run_rowfilter(gpu, x, thresh, f32, m_want, rows_off=1, idx_off=1, cnt_off=1, ws_off=1, tag=""):
    """pxsom_rowsum_filter_normalize the way som_device.rowsum_filter_normalize calls it, every output and the
    workspace inside sentinel buffers; returns (rows [m, c], kept [m]) after checking the count against `m_want`, the
    reference's number of kept rows, and the guards: only the first m_want rows and indices may be written."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    n, c = x.shape
    fr, fi, fw = _sentinel(np.float64), _sentinel(np.int64), _sentinel(np.uint32)
    xt = torch.from_numpy(x).to(gpu)
    rbuf, rows = _view1d(gpu, np.full(n * c, fr), rows_off, 5, fr)
    ibuf, idx = _view1d(gpu, np.full(n, fi), idx_off, 5, fi)
    cbuf, cnt = _view1d(gpu, np.full(1, fi), cnt_off, 3, fi)
    wsb = lib.pxsom_rownorm_workspace_bytes(n)
    assert wsb % 4 == 0 and wsb > 0, tag
    wbuf, ws = _view1d(gpu, np.full(wsb // 4, fw), ws_off, 7, fw)
    rc = lib.pxsom_rowsum_filter_normalize(xt.data_ptr(), n, c, float(thresh), rows.data_ptr(), idx.data_ptr(),
                                           cnt.data_ptr(), ws.data_ptr(), wsb, int(bool(f32)), _capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == PXSOM_OK, tag
    m = int(cnt.item())
    assert m == m_want, tag + ": kept %d rows, the reference %d" % (m, m_want)
    assert _guard_intact(rbuf.cpu().numpy(), slice(rows_off, rows_off + m * c), fr), tag + ": stores past the kept rows"
    assert _guard_intact(ibuf.cpu().numpy(), slice(idx_off, idx_off + m), fi), tag + ": stores past the kept indices"
    assert _guard_intact(cbuf.cpu().numpy(), slice(cnt_off, cnt_off + 1), fi), tag + ": count guard"
    assert _guard_intact(wbuf.cpu().numpy(), slice(ws_off, ws_off + wsb // 4), fw), tag + ": workspace guard"
    assert _bytes_equal(xt.cpu().numpy(), x), tag + ": the input changed"
    return rows.cpu().numpy()[:m * c].reshape(m, c), idx.cpu().numpy()[:m]


def test_fuzz_rowfilter(gpu, oracle):
    """pxsom_rowsum_filter_normalize against oracle.rowsum_filter_normalize: kept indices equal, rows bit for bit with
    NaNs matching in position; rows, indices, count and workspace inside sentinel buffers."""
    for case in rowfilter_cases(SEED + 41, case_count(ROWFILTER_CLASSES)):
        x = case["x"]
        n, c = x.shape
        tag = "case %d: class=%s route=%s n=%d c=%d thresh=%r %s sweeps=%d (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], case["cls"], case["route"], n, c, case["thresh"], _f32(case["f32"]), case["sweeps"], SEED)
        with np.errstate(all="ignore"):
            wr, wk = oracle.rowsum_filter_normalize(x, case["thresh"], sum_mode=2 if case["f32"] else 0)
        rows, kept = _run_rowfilter(gpu, x, case["thresh"], case["f32"], wk.size, case["rows_off"], case["idx_off"],
                                    case["cnt_off"], case["ws_off"], tag)
        assert np.array_equal(kept, wk), tag + ": kept %d rows, the oracle %d" % (kept.size, wk.size)
        assert _same_bits(rows, wr), tag + ": normalised rows"
        if case["equal_row"] >= 0:
            assert case["equal_row"] not in kept, tag + ": the row whose sum equals thresh was kept"


def test_rowfilter_nan_rows_follow_pandas(gpu, oracle):
    """Found by the nan_rows class: DataFrame.sum(axis=1) skips NaN, so a row with a NaN is judged by the sum of its
    other values and kept with its NaN in place; kernel and oracle used to let the NaN poison the sum and drop the
    row.  The expected values are pandas' (tests/test_fuzz_generators.py holds the oracle to them)."""
    nan = np.nan
    x = np.array([[nan, 2.0, 3.0], [nan, nan, nan], [0.5, 0.25, 0.25], [nan, 0.0, 0.0], [1.0, nan, -1.0]])
    for f32 in (False, True):
        rows, kept = _run_rowfilter(gpu, x, 0.0, f32, 2, tag="thresh 0 %s" % _f32(f32))
        assert np.array_equal(kept, [0, 2])
        assert _same_bits(rows, np.array([[nan, 0.4, 0.6], [0.5, 0.25, 0.25]], np.float32 if f32 else np.float64)
                          .astype(np.float64))
        rows, kept = _run_rowfilter(gpu, x, -1.0, f32, 5, tag="thresh -1 %s" % _f32(f32))
        assert np.array_equal(kept, [0, 1, 2, 3, 4])
        with np.errstate(all="ignore"):
            wr, wk = oracle.rowsum_filter_normalize(x, -1.0, sum_mode=2 if f32 else 0)
        assert np.array_equal(wk, kept) and _same_bits(rows, wr)
        assert np.isnan(rows[1]).all() and np.isnan(rows[3]).all()       # x / 0 with x NaN or 0
        assert np.isnan(rows[4, 1]) and rows[4, 0] == np.inf and rows[4, 2] == -np.inf


# ---- K5 pxsom_quantile_nonzero / pxsom_quantile_f32 ---------------------------------------------------------------
kQCols, kQRows = 48, 1024               # pxsom_pre.hip
QUANTILE_CLASSES = ("interior", "c1", "c47", "c48", "c49", "c96", "c97", "ldx_view", "n0", "n1", "n2", "n1023",
                    "n1024", "n1025", "n_large", "m0", "m1", "m2", "q_0", "q_1", "q_1e-9", "q_0.5", "q_0.999",
                    "q_pandas", "q_integral", "mode0", "mode1", "mode2") + tuple(
                        v + sfx for v in ("all_negative", "mixed_sign", "pm_zero", "subnormals", "inf_among_finite", "nans",
                                          "two_values", "all_equal", "dup_straddle", "low_byte", "exponent_only")
                        for sfx in ("_f32", "_f64"))
_Q_VALUES = {"q_0": 0.0, "q_1": 1.0, "q_1e-9": 1e-9, "q_0.5": 0.5, "q_0.999": 0.999, "q_pandas": (0.999 * 100) / 100}


def quantile_chunks(c):
    """(sweeps per pass, columns of the last sweep): one q_hist_kernel sweep serves up to kQCols columns."""
    return (c + kQCols - 1) // kQCols, c - (c - 1) // kQCols * kQCols


def quantile_passes(itemsize):
    """Radix passes run: 8 for binary64 rows, 5 for binary32 rows (fill_low completes key bits 0 .. 23)."""
    return 8 if itemsize == 8 else 5


def quantile_kept(col, keep_mode):
    with np.errstate(invalid="ignore"):
        if keep_mode == 0:
            return col[(col != 0) & ~np.isnan(col)]
        if keep_mode == 1:
            return col[col > 0]
    return col[~np.isnan(col)]


def quantile_reference(x, q, keep_mode):
    """np.quantile of the kept values of every column in the array's dtype, NaN for a column without one -> [c] f64."""
    out = np.full(x.shape[1], np.nan)
    with np.errstate(all="ignore"):
        for j in range(x.shape[1]):
            kept = quantile_kept(np.ascontiguousarray(x[:, j]), keep_mode)
            if kept.size:
                out[j] = np.quantile(kept, q)
    return out


def _bits_dtype(dt):
    return np.uint64 if np.dtype(dt).itemsize == 8 else np.uint32


def quantile_cases(seed, count):
    """Cases of test_fuzz_quantile, for pxsom_quantile_nonzero (binary64) and pxsom_quantile_f32 alike: class i % 50
    of QUANTILE_CLASSES (50 classes: the default run is 50 cases) -- c on the 48-column sweeps; a strided view at a
    column offset; n around the 1024-row blocks; 0 / 1 / 2 kept values; the q values, one with q (m - 1) integral; the
    keep modes; every value class once per dtype (the float32 entry skips three radix passes and completes the key
    by the value's sign, the binary64 entry runs the pass over the lowest key byte) -- then the dtype of the other
    classes (alternating between the visits of a class), the rest of shape, q, keep mode and view at random."""
    rs = np.random.RandomState(seed)
    r_cls = len(QUANTILE_CLASSES)
    for i in range(count):
        cls, forced = _forced(QUANTILE_CLASSES[i % r_cls])
        dt = np.float32 if (_alternate(i, r_cls) if forced is None else forced) else np.float64
        c, n = int(rs.randint(1, 7)), int(rs.randint(3, 400))
        q = float(rs.choice([0.05, 0.5, 0.99, 0.123456, 0.75]))
        mode = int(rs.randint(0, 3))
        off, pad = int(rs.choice([0, 0, 1, 3])), int(rs.choice([0, 0, 2, 5]))
        if cls[0] == "c" and cls[1:].isdigit():
            c = int(cls[1:])
        elif cls == "ldx_view":
            off, pad = int(rs.randint(1, 6)), int(rs.randint(1, 8))
        elif cls[0] == "n" and cls[1:].isdigit():
            n = int(cls[1:])
        elif cls == "n_large":
            n, c = int(rs.randint(30000, 120000)), int(rs.randint(1, 4))
        elif cls in _Q_VALUES:
            q = _Q_VALUES[cls]
        elif cls == "q_integral":
            n, mode = int(rs.choice([65, 129, 1025])), 2
            q = float(rs.choice([0.25, 0.5, 0.75, 0.015625]))
        elif cls in ("mode0", "mode1", "mode2"):
            mode = int(cls[4])
        x = rs.standard_normal(size=(n, c)) * 10.0 ** float(rs.uniform(-3, 3))
        x[rs.rand(n, c) < 0.3] = 0.0
        if cls != "q_integral":
            x[rs.rand(n, c) < 0.02] = np.nan
        x = x.astype(dt)
        tiny = np.finfo(dt).smallest_subnormal
        if cls in ("m0", "m1", "m2"):                    # column 0: exactly m kept values among values the mode drops
            n = max(n, 5)
            x = np.resize(x, (n, c)).copy()
            drop = {0: [0.0, -0.0, np.nan], 1: [0.0, -0.0, np.nan, -1.5, -np.inf], 2: [np.nan]}[mode]
            x[:, 0] = rs.choice(drop, size=n)
            m = int(cls[1])
            x[rs.choice(n, m, replace=False), 0] = (rs.uniform(0.5, 9.0, size=m) * (1 if mode == 1 else
                                                                                    rs.choice([-1, 1], size=m)))
        elif cls == "all_negative":
            x = -np.abs(x) - dt(1e-3)
            mode = int(rs.choice([0, 2]))
        elif cls == "mixed_sign":
            x = (rs.standard_normal(size=(n, c)) * 3).astype(dt)
            mode = int(rs.choice([0, 2]))
        elif cls == "pm_zero":
            x = rs.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, tiny, -tiny], dt), size=(n, c))
            mode = 2 if rs.rand() < 0.7 else mode
        elif cls == "subnormals":
            x = (rs.randint(-50, 51, size=(n, c)) * tiny).astype(dt)
            x[rs.rand(n, c) < 0.2] = dt(rs.choice([1.0, -1.0])) * np.finfo(dt).tiny
        elif cls == "inf_among_finite":
            x[rs.rand(n, c) < 0.1] = np.inf
            x[rs.rand(n, c) < 0.1] = -np.inf
            x[0, 0] = np.inf
            mode = int(rs.choice([0, 1, 2]))
        elif cls == "nans":
            x[rs.rand(n, c) < 0.3] = np.nan
        elif cls == "two_values":
            a, b = (rs.standard_normal(2) * 5).astype(dt)
            x = rs.choice(np.array([a, b], dt), size=(n, c))
        elif cls == "all_equal":
            x = np.full((n, c), dt(rs.standard_normal() * 7 + 0.1))
        elif cls == "dup_straddle":                    # ranks lo, lo + 1 (and one more) of every column hold one value
            mode, q = 2, float(rs.choice([0.5, 0.123456, 0.9]))
            if (q * (n - 1)) % 1 == 0:                 # a fractional index: ranks lo and hi = lo + 1 both count
                q = 0.123456
            x = (rs.standard_normal(size=(n, c)) * 4).astype(dt)
            lo = int(np.floor(q * (n - 1)))
            for j in range(c):
                order = np.argsort(x[:, j], kind="stable")
                x[order[lo:min(n, lo + 3)], j] = x[order[lo], j]
        elif cls in ("low_byte", "exponent_only"):
            ub = _bits_dtype(dt)
            base = np.array([rs.uniform(1.0, 2.0)], dt).view(ub)[0]
            if cls == "low_byte":
                bits = (base & ~ub(0xFF)) | rs.randint(0, 256, size=(n, c)).astype(ub)
            else:
                mant_bits, ebias, emax = (52, 1023, 1000) if dt == np.float64 else (23, 127, 120)
                mant = base & ub((1 << mant_bits) - 1)
                bits = mant | (rs.randint(ebias - emax, ebias + emax, size=(n, c)).astype(ub) << ub(mant_bits))
            x = bits.astype(ub).view(dt).reshape(n, c).copy()
            x[rs.rand(n, c) < 0.4] *= -1
            mode = int(rs.choice([0, 2]))
        yield dict(i=i, cls=QUANTILE_CLASSES[i % r_cls], x=np.ascontiguousarray(x), q=q, keep_mode=mode, off=off, pad=pad,
                   chunks=quantile_chunks(c), passes=quantile_passes(np.dtype(dt).itemsize),
                   out_off=int(rs.randint(0, 4)), ws_off=int(rs.randint(0, 4)))


def _run_quantile(gpu, x_t, n, c, ldx, q, keep_mode, out_off=1, ws_off=1, tag=""):
    """pxsom_quantile_nonzero / pxsom_quantile_f32 by the dtype of x_t, called as the som_device wrappers call them,
    with the [c] output and the workspace inside sentinel buffers -> [c] f64 after the guard checks."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fo, fw = _sentinel(np.float64), _sentinel(np.int64)
    obuf, out = _view1d(gpu, np.full(c, fo), out_off, 3, fo)
    wsb = lib.pxsom_quantile_workspace_bytes(n, c)
    assert wsb > 0 and wsb % 8 == 0, tag
    wbuf, ws = _view1d(gpu, np.full(wsb // 8, fw), ws_off, 3, fw)
    fn = lib.pxsom_quantile_f32 if x_t.dtype == torch.float32 else lib.pxsom_quantile_nonzero
    rc = fn(x_t.data_ptr(), n, c, ldx, float(q), int(keep_mode), out.data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == PXSOM_OK, tag
    assert _guard_intact(obuf.cpu().numpy(), slice(out_off, out_off + c), fo), tag + ": output guard"
    assert _guard_intact(wbuf.cpu().numpy(), slice(ws_off, ws_off + wsb // 8), fw), tag + ": workspace guard"
    return out.cpu().numpy()


def test_fuzz_quantile(gpu):
    """Both quantile entries against np.quantile of the kept values in the array's dtype: equal as numbers or both NaN
    (numpy's own NaN where its interpolation meets inf - inf included); the matrix a strided view at a column offset,
    output and workspace inside sentinel buffers."""
    for case in quantile_cases(SEED + 42, case_count(QUANTILE_CLASSES)):
        x = case["x"]
        n, c = x.shape
        tag = "case %d: class=%s %s n=%d c=%d q=%r keep_mode=%d off=%d pad=%d chunks=%s (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], case["cls"], x.dtype, n, c, case["q"], case["keep_mode"], case["off"], case["pad"],
            case["chunks"], SEED)
        buf, xt = _view2d(gpu, x, case["off"], case["pad"], fill=_sentinel(x.dtype))
        ldx = case["off"] + c + case["pad"]
        got = _run_quantile(gpu, xt, n, c, ldx, case["q"], case["keep_mode"], case["out_off"], case["ws_off"], tag)
        want = quantile_reference(x, case["q"], case["keep_mode"])
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        assert bad.size == 0, tag + ": columns %s: got %r, numpy %r" % (bad[:5], got[bad[:5]], want[bad[:5]])


def test_quantile_f32_index_past_2_24(gpu):
    """One float32 column of m = 2^24 + 5 kept values of both signs, q = 0.999: the virtual index (float)(m - 1) *
    (float)q and its fraction are formed in binary32 above 2^24, where consecutive integers are no longer
    representable; the result must equal np.quantile's on the float32 array."""
    import torch
    m = 2 ** 24 + 5
    x = np.random.RandomState(SEED + 43).standard_normal(size=(m, 1)).astype(np.float32)
    got = _run_quantile(gpu, torch.from_numpy(x).to(gpu), m, 1, 1, 0.999, 2, tag="m=2^24+5")
    want = quantile_reference(x, 0.999, 2)
    assert _same_numbers(got, want), "got %r, numpy %r" % (got, want)


# ---- pxsom_scaled_rowsum_f32 / _f64 -------------------------------------------------------------------------------
SCALED_ROWSUM_MAX_C = 128
SCALED_ROWSUM_CLASSES = ("interior", "c1", "c7", "c8", "c9", "c15", "c16", "c17", "c127", "c128", "ldx_view",
                         "zero_divisor", "inf_divisor", "c129_refused")


def scaled_rowsum_route(c):
    """scaled_rowsum_kernel: left to right below 8 terms, else numpy's eight running sums with a tail of c % 8 terms;
    refused past 128 channels."""
    if c > SCALED_ROWSUM_MAX_C:
        return "refused"
    return "sequential" if c < 8 else "unrolled_tail%d" % (c % 8)


def scaled_rowsum_cases(seed, count):
    """Cases of test_fuzz_scaled_rowsum: class i % 14 of SCALED_ROWSUM_CLASSES (14 classes: the default run is 14
    cases) -- c around the blocks of 8 and at the limit of 128, a strided view, a zero and an infinite divisor, the
    refused c = 129 -- then dtype, n, values and the output offset."""
    rs = np.random.RandomState(seed)
    r_cls = len(SCALED_ROWSUM_CLASSES)
    for i in range(count):
        cls = SCALED_ROWSUM_CLASSES[i % r_cls]
        dt = np.float32 if _alternate(i, r_cls) else np.float64
        c, n = int(rs.randint(1, 40)), int(rs.choice([1, 255, 256, 257, int(rs.randint(1, 4000))]))
        off, pad = int(rs.choice([0, 0, 1, 3])), int(rs.choice([0, 0, 1, 4]))
        if cls[0] == "c" and cls[1:].split("_")[0].isdigit():
            c = int(cls[1:].split("_")[0])
        elif cls == "ldx_view":
            off, pad = int(rs.randint(1, 5)), int(rs.randint(1, 9))
        img = (rs.gamma(0.5, 2.0, size=(n, c)) * (rs.rand(n, c) < 0.7) * rs.choice([1.0, -1.0], size=(n, c))).astype(dt)
        norm = rs.uniform(0.5, 3.0, size=c).astype(dt)
        if cls == "zero_divisor":
            norm[rs.randint(0, c)] = 0.0
        elif cls == "inf_divisor":
            norm[rs.randint(0, c)] = np.inf
        yield dict(i=i, cls=cls, img=img, norm=norm, off=off, pad=pad, route=scaled_rowsum_route(c),
                   out_off=int(rs.randint(0, 4)))


def scaled_rowsum_reference(img, norm):
    with np.errstate(all="ignore"):
        return np.sum(np.ascontiguousarray(img) / norm, axis=-1)


def test_fuzz_scaled_rowsum(gpu):
    """pxsom_scaled_rowsum_f32 / _f64 against np.sum(img / norm, axis=-1) on a contiguous array of the dtype, bit for
    bit with NaNs by position; the [n] output inside a sentinel buffer; c = 129 returns PXSOM_ERR_INVALID_ARG."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    for case in scaled_rowsum_cases(SEED + 44, case_count(SCALED_ROWSUM_CLASSES)):
        img, norm = case["img"], case["norm"]
        n, c = img.shape
        tag = "case %d: class=%s route=%s %s n=%d c=%d off=%d pad=%d out_off=%d (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], case["cls"], case["route"], img.dtype, n, c, case["off"], case["pad"], case["out_off"], SEED)
        fill = _sentinel(img.dtype)
        _, xt = _view2d(gpu, img, case["off"], case["pad"], fill=fill)
        obuf, out = _view1d(gpu, np.full(n, fill, img.dtype), case["out_off"], 5, fill)
        fn = lib.pxsom_scaled_rowsum_f32 if img.dtype == np.float32 else lib.pxsom_scaled_rowsum_f64
        norm_t = torch.from_numpy(norm).to(gpu)
        rc = fn(xt.data_ptr(), n, c, case["off"] + c + case["pad"], norm_t.data_ptr(), out.data_ptr(), _capi.stream_ptr())
        torch.cuda.synchronize()
        if case["route"] == "refused":
            assert rc == PXSOM_ERR_INVALID_ARG, tag
            assert _guard_intact(obuf.cpu().numpy(), slice(0, 0), fill), tag + ": a refused call wrote the output"
            continue
        assert rc == PXSOM_OK, tag
        assert _same_bits(out.cpu().numpy(), scaled_rowsum_reference(img, norm)), tag
        assert _guard_intact(obuf.cpu().numpy(), slice(case["out_off"], case["out_off"] + n), fill), tag + ": guard"


# ---- K4 pxsom_normalize_columns -----------------------------------------------------------------------------------
NORMALIZE_CLASSES = ("interior", "ldx_ne_ldo", "in_place", "out_padded", "zero_divisor", "nan_divisor",
                     "inf_divisor", "n0")


def normalize_columns_cases(seed, count):
    """Cases of test_fuzz_normalize_columns: class i % 8 of NORMALIZE_CLASSES -- input and output row strides that
    differ, in place, an output with padding columns, divisors 0 / NaN / inf, no rows -- then shape and values."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        cls = NORMALIZE_CLASSES[i % len(NORMALIZE_CLASSES)]
        n, c = int(rs.randint(1, 3000)), int(rs.randint(1, 100))
        if cls == "n0":
            n = 0
        x = rs.standard_normal(size=(n, c)) * 10.0 ** rs.uniform(-3, 3, size=(1, c))
        x[rs.rand(n, c) < 0.3] = 0.0
        if rs.rand() < 0.3 and n:
            x[rs.randint(0, n), rs.randint(0, c)] = np.nan
        norm = rs.uniform(0.1, 5.0, size=c)
        if cls.endswith("_divisor"):
            norm[rs.randint(0, c)] = {"zero": 0.0, "nan": np.nan, "inf": np.inf}[cls.split("_")[0]]
        in_off, in_pad = int(rs.choice([0, 1, 2])), int(rs.choice([0, 1, 3]))
        out_off, out_pad = int(rs.choice([0, 1, 3])), int(rs.choice([0, 2, 5]))
        if cls == "ldx_ne_ldo":
            in_off, in_pad, out_off, out_pad = 1, 2, int(rs.choice([0, 2])), int(rs.choice([0, 5]))
        elif cls == "out_padded":
            out_off, out_pad = int(rs.randint(1, 4)), int(rs.randint(1, 6))
        elif cls == "in_place":
            out_off, out_pad = in_off, in_pad
        yield dict(i=i, cls=cls, x=x, norm=norm, in_place=cls == "in_place", in_off=in_off, in_pad=in_pad,
                   out_off=out_off, out_pad=out_pad, rows=int(rs.randint(0, 3)))


def test_fuzz_normalize_columns(gpu):
    """pxsom_normalize_columns against numpy's x / norm, bit for bit with NaNs by position; strided input and output
    views (ldx != ldo), in place; the padding columns and guard rows of the output buffer keep the sentinel."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fill = _sentinel(np.float64)
    for case in normalize_columns_cases(SEED + 45, case_count(NORMALIZE_CLASSES)):
        x, norm = case["x"], case["norm"]
        n, c = x.shape
        top = case["rows"]
        tag = "case %d: class=%s n=%d c=%d in(off=%d pad=%d) out(off=%d pad=%d rows=%d) (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], case["cls"], n, c, case["in_off"], case["in_pad"], case["out_off"], case["out_pad"], top, SEED)
        xbuf, xt = _view2d(gpu, x, case["in_off"], case["in_pad"], top, top, fill)
        if case["in_place"]:
            obuf, out = xbuf, xt
        else:
            obuf, out = _view2d(gpu, np.full((n, c), fill), case["out_off"], case["out_pad"], top, top, fill)
        ldx, ldo = case["in_off"] + c + case["in_pad"], case["out_off"] + c + case["out_pad"]
        norm_t = torch.from_numpy(norm).to(gpu)
        rc = lib.pxsom_normalize_columns(xt.data_ptr(), n, c, ldx, norm_t.data_ptr(), out.data_ptr(), ldo,
                                         _capi.stream_ptr())
        torch.cuda.synchronize()
        assert rc == PXSOM_OK, tag
        with np.errstate(all="ignore"):
            want = x / norm[None, :]
        assert _same_bits(out.cpu().numpy(), want), tag
        region = (slice(top, top + n), slice(case["out_off"], case["out_off"] + c))
        assert _guard_intact(obuf.cpu().numpy(), region, fill), tag + ": stores outside the output view"
        if not case["in_place"]:
            assert _bytes_equal(xbuf.cpu().numpy()[top:top + n, case["in_off"]:case["in_off"] + c], x), tag + ": input changed"


# ---- pxsom_relabel, pxsom_pair_histogram, pxsom_cluster_mask ------------------------------------------------------
RELABEL_MAX_LUT = 16384                 # pxsom_relabel: the table in LDS, 64 KB
PXSOM_MASK_BAD_LABEL, PXSOM_MASK_BAD_PIXEL = 1, 2
PXSOM_LUT_UNMAPPED = -2 ** 31
LABEL_CLASSES = ("relabel_interior", "relabel_lut1", "relabel_lut16384", "relabel_lut16385", "relabel_offsets",
                 "relabel_in_place", "hist_interior", "hist_one_bin", "hist_out_of_range", "hist_accumulate",
                 "hist_n0", "mask_interior", "mask_one_pixel", "mask_n0", "mask_wide_ids", "mask_bad_label",
                 "mask_bad_pixel")


def relabel_route(lut_size, in_off, out_off):
    """pxsom_relabel: refused outside 1 .. 16384 table entries; 16-byte vectors of 4 labels when both pointers are
    16-byte aligned (here: both element offsets multiples of 4 in a 256-byte aligned buffer), else label by label."""
    if lut_size < 1 or lut_size > RELABEL_MAX_LUT:
        return "refused"
    return "vector" if in_off % 4 == 0 and out_off % 4 == 0 else "scalar"


def cluster_mask_status(row_index, column_index, labels, lut, h, w):
    """The status word of pxsom_cluster_mask: PXSOM_MASK_BAD_PIXEL for a flat position outside [0, h w),
    PXSOM_MASK_BAD_LABEL for a label (of a row inside the image) outside the table or mapped to PXSOM_LUT_UNMAPPED."""
    pos = row_index * w + column_index
    inside = (pos >= 0) & (pos < h * w)
    status = 0 if inside.all() else PXSOM_MASK_BAD_PIXEL
    lb = labels[inside]
    ok = (lb >= 0) & (lb < lut.size)
    if not ok.all() or (lut[lb[ok]] == PXSOM_LUT_UNMAPPED).any():
        status |= PXSOM_MASK_BAD_LABEL
    return status


def label_kernel_cases(seed, count):
    """Cases of test_fuzz_label_kernels: class i % 17 of LABEL_CLASSES (17 classes: the default run is 17 cases).
    relabel: tables of 1 and 16384 entries, the refused 16385, every pair of input / output element offsets 0 .. 3 with
    every n % 4, in place.  pair_histogram: all pairs in one bin, pairs outside the table, a table that already holds
    counts, n = 0.  cluster_mask: every row on one pixel, n = 0, ids beyond int16, labels unmapped or outside the
    table, positions past the image (never negative: numpy would wrap those where the kernel reports
    PXSOM_MASK_BAD_PIXEL)."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        cls = LABEL_CLASSES[i % len(LABEL_CLASSES)]
        case = dict(i=i, cls=cls, kind=cls.split("_")[0])
        if case["kind"] == "relabel":
            lut_size = {"relabel_lut1": 1, "relabel_lut16384": 16384, "relabel_lut16385": 16385}.get(
                cls, int(rs.randint(2, 2000)))
            lut = rs.randint(-50, 50, size=lut_size).astype(np.int32)
            if cls == "relabel_offsets":       # every offset pair; every n % 4 for each input offset and for the aligned pair
                runs = [dict(in_off=a, out_off=b, n=4 * int(rs.randint(1, 1500)) + (a + b) % 4)
                        for a in range(4) for b in range(4)]
                runs += [dict(in_off=0, out_off=0, n=4 * int(rs.randint(1, 1500)) + r) for r in (1, 2, 3)]
            else:
                runs = [dict(in_off=int(rs.randint(0, 4)), out_off=int(rs.randint(0, 4)), n=int(rs.randint(1, 20000)))]
            for r in runs:
                r["labels"] = rs.randint(-3, lut_size + 3, size=r["n"]).astype(np.int32)
                r["labels"][rs.randint(0, r["n"])] = lut_size - 1
                r["route"] = relabel_route(lut_size, r["in_off"], r["in_off"] if cls == "relabel_in_place" else r["out_off"])
            case.update(lut=lut, fill=int(rs.choice([-1, -7, 2 ** 31 - 1])), in_place=cls == "relabel_in_place",
                        runs=runs)
        elif case["kind"] == "hist":
            na, nb = int(rs.randint(1, 300)), int(rs.randint(1, 40))
            n = 0 if cls == "hist_n0" else int(rs.randint(1, 30000))
            a = rs.randint(0, na, size=n).astype(np.int32)
            b = rs.randint(0, nb, size=n).astype(np.int32)
            if cls == "hist_one_bin":
                a[:], b[:] = int(rs.randint(0, na)), int(rs.randint(0, nb))
            elif cls == "hist_out_of_range":
                a = rs.randint(-3, na + 3, size=n).astype(np.int32)
                b = rs.randint(-3, nb + 3, size=n).astype(np.int32)
                a[0], b[0] = na, nb - 1
                a[-1], b[-1] = 0, -1
            start = np.zeros((na, nb), np.int64)
            if cls == "hist_accumulate" or rs.rand() < 0.3:
                start = rs.randint(0, 2 ** 40, size=(na, nb)).astype(np.int64)
            case.update(a=a, b=b, na=na, nb=nb, start=start, off=int(rs.randint(0, 4)))
        else:
            h, w = int(rs.randint(1, 120)), int(rs.randint(1, 120))
            lut_size = int(rs.randint(1, 60))
            n = 0 if cls == "mask_n0" else int(rs.randint(1, 2 * h * w + 2))
            lut = rs.randint(-30000, 30000, size=lut_size).astype(np.int32)
            if cls == "mask_wide_ids":
                lut = rs.randint(-70000, 70001, size=lut_size).astype(np.int32)
                lut[0] = 40000
            pos = rs.randint(0, h * w, size=n).astype(np.int64)
            if cls == "mask_one_pixel":
                pos[:] = int(rs.randint(0, h * w))
            labels = rs.randint(0, lut_size, size=n).astype(np.int64)
            if cls == "mask_wide_ids":
                labels[0] = 0
            row_index, column_index = pos // w, pos % w
            if cls == "mask_bad_label":
                which = int(rs.randint(0, 3))
                if which == 0:
                    lut[labels[0]] = PXSOM_LUT_UNMAPPED
                else:
                    labels[int(rs.randint(0, n))] = lut_size + int(rs.randint(0, 3)) if which == 1 else -1
            elif cls == "mask_bad_pixel":                       # flat positions past the image, never negative
                j = int(rs.randint(0, n))
                row_index[j], column_index[j] = (h, 0) if rs.rand() < 0.5 else (h - 1, w + int(rs.randint(0, 5)))
            case.update(row_index=row_index, column_index=column_index, labels=labels, lut=lut, h=h, w=w,
                        status=cluster_mask_status(row_index, column_index, labels, lut, h, w),
                        off=int(rs.randint(0, 4)), st_off=int(rs.randint(0, 4)), ws_off=int(rs.randint(0, 4)))
        yield case


def relabel_reference(labels, lut, fill):
    inside = (labels >= 0) & (labels < lut.size)
    return np.where(inside, lut[np.clip(labels, 0, lut.size - 1)], np.int32(fill)).astype(np.int32)


def pair_histogram_reference(a, b, na, nb, start):
    want = start.copy()
    ok = (a >= 0) & (a < na) & (b >= 0) & (b < nb)
    np.add.at(want, (a[ok].astype(np.int64), b[ok].astype(np.int64)), 1)
    return want


def cluster_mask_reference(row_index, column_index, labels, lut, h, w):
    """generate_pixel_cluster_mask's numpy statement; for a status of 0 only."""
    want = np.zeros(h * w, np.int16)
    want[row_index * w + column_index] = lut[labels].astype(np.int16)
    return want.reshape(h, w)


def test_fuzz_label_kernels(gpu):
    """pxsom_relabel, pxsom_pair_histogram and pxsom_cluster_mask against their numpy statements, array_equal; labels
    and outputs at element offsets inside sentinel buffers, the mask's status word and workspace too."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    f32i, f64i, f16i = _sentinel(np.int32), _sentinel(np.int64), _sentinel(np.int16)
    for case in label_kernel_cases(SEED + 46, case_count(LABEL_CLASSES)):
        tag = "case %d: class=%s (PXSOM_FUZZ_SEED=%d)" % (case["i"], case["cls"], SEED)
        if case["kind"] == "relabel":
            lut = case["lut"]
            lut_t = torch.from_numpy(lut).to(gpu)
            for r in case["runs"]:
                n, labels = r["n"], r["labels"]
                t = tag + " lut=%d n=%d (n %% 4 = %d) in_off=%d out_off=%d route=%s fill=%d" % (
                    lut.size, n, n % 4, r["in_off"], r["out_off"], r["route"], case["fill"])
                lbuf, lt = _view1d(gpu, labels, r["in_off"], 5, f32i)
                if case["in_place"]:
                    obuf, out, out_off = lbuf, lt, r["in_off"]
                else:
                    obuf, out = _view1d(gpu, np.full(n, f32i), r["out_off"], 5, f32i)
                    out_off = r["out_off"]
                rc = lib.pxsom_relabel(lt.data_ptr(), n, lut_t.data_ptr(), lut.size, case["fill"], out.data_ptr(),
                                       _capi.stream_ptr())
                torch.cuda.synchronize()
                if r["route"] == "refused":
                    assert rc == PXSOM_ERR_INVALID_ARG, t
                    assert _guard_intact(obuf.cpu().numpy(), slice(0, 0), f32i), t + ": a refused call wrote the output"
                    continue
                assert rc == PXSOM_OK, t
                assert np.array_equal(out.cpu().numpy(), relabel_reference(labels, lut, case["fill"])), t
                assert _guard_intact(obuf.cpu().numpy(), slice(out_off, out_off + n), f32i), t + ": output guard"
                if not case["in_place"]:
                    assert _bytes_equal(lt.cpu().numpy(), labels), t + ": the labels changed"
        elif case["kind"] == "hist":
            a, b, na, nb = case["a"], case["b"], case["na"], case["nb"]
            t = tag + " n=%d na=%d nb=%d off=%d" % (a.size, na, nb, case["off"])
            hbuf, hist = _view1d(gpu, case["start"], case["off"], 5, f64i)
            at, bt = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
            rc = lib.pxsom_pair_histogram(at.data_ptr(), bt.data_ptr(), a.size, na, nb, hist.data_ptr(), _capi.stream_ptr())
            torch.cuda.synchronize()
            assert rc == PXSOM_OK, t
            assert np.array_equal(hist.cpu().numpy(), pair_histogram_reference(a, b, na, nb, case["start"])), t
            assert _guard_intact(hbuf.cpu().numpy(), slice(case["off"], case["off"] + na * nb), f64i), t + ": guard"
        else:
            h, w, lut = case["h"], case["w"], case["lut"]
            n = case["labels"].size
            t = tag + " n=%d %dx%d lut=%d status=%d off=%d" % (n, h, w, lut.size, case["status"], case["off"])
            mbuf, mask = _view1d(gpu, np.full((h, w), f16i), case["off"], 7, f16i)
            sbuf, status = _view1d(gpu, np.full(1, f32i), case["st_off"], 3, f32i)
            wsb = lib.pxsom_cluster_mask_workspace_bytes(h, w)
            assert wsb == h * w * 8, t
            wbuf, ws = _view1d(gpu, np.full(h * w, f64i), case["ws_off"], 3, f64i)
            dev = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu)
                   for v in (case["row_index"], case["column_index"], case["labels"])]
            lut_t = torch.from_numpy(lut).to(gpu)
            rc = lib.pxsom_cluster_mask(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n,
                                        lut_t.data_ptr(), lut.size, h, w, mask.data_ptr(),
                                        status.data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr())
            torch.cuda.synchronize()
            assert rc == PXSOM_OK, t
            assert int(status.item()) == case["status"], t + ": status %d" % int(status.item())
            if case["status"] == 0:
                want = cluster_mask_reference(case["row_index"], case["column_index"], case["labels"], lut, h, w)
                assert np.array_equal(mask.cpu().numpy(), want), t
            assert _guard_intact(mbuf.cpu().numpy(), slice(case["off"], case["off"] + h * w), f16i), t + ": mask guard"
            assert _guard_intact(sbuf.cpu().numpy(), slice(case["st_off"], case["st_off"] + 1), f32i), t + ": status guard"
            assert _guard_intact(wbuf.cpu().numpy(), slice(case["ws_off"], case["ws_off"] + h * w), f64i), t + ": workspace guard"


# ---- pxsom_absmax -------------------------------------------------------------------------------------------------
ABSMAX_CLASSES = ("interior", "ldx_view", "negative_largest", "nonfinite_among_finite", "no_finite", "n0")
ABSMAX_NP = (np.float32, np.float64, np.float16)


def absmax_reference(x):
    """max |x| over the finite entries, 0 when there is none, as a binary64 number."""
    f = x[np.isfinite(x)]
    return float(np.abs(f).max()) if f.size else 0.0


def absmax_cases(seed, count):
    """Cases of test_fuzz_absmax: class i % 6 of ABSMAX_CLASSES -- a strided view, a negative value the largest, NaN
    and +-inf among finite values, no finite entry at all, no rows.  The values are multiples of 1/2 within +-1000.5
    (every storage type holds them); each case runs in f32, f64 and f16."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        cls = ABSMAX_CLASSES[i % len(ABSMAX_CLASSES)]
        n, c = int(rs.randint(1, 3000)), int(rs.randint(1, 70))
        if cls == "n0":
            n = 0
        x = rs.randint(-2000, 2001, size=(n, c)) / 2.0
        x[rs.rand(n, c) < 0.3] = 0.0
        off, pad = int(rs.choice([0, 0, 1, 3])), int(rs.choice([0, 0, 1, 5]))
        if cls == "ldx_view":
            off, pad = int(rs.randint(1, 5)), int(rs.randint(1, 9))
        elif cls == "negative_largest":
            x[rs.randint(0, n), rs.randint(0, c)] = -1000.5
        elif cls == "nonfinite_among_finite":
            for v in (np.nan, np.inf, -np.inf):
                x[rs.rand(n, c) < 0.05] = v
                x[rs.randint(0, n), rs.randint(0, c)] = v
        elif cls == "no_finite":
            x = rs.choice([np.nan, np.inf, -np.inf], size=(n, c))
        yield dict(i=i, cls=cls, x=x, off=off, pad=pad, out_off=int(rs.randint(0, 4)))


def test_fuzz_absmax(gpu):
    """pxsom_absmax in all three storage types against numpy over the finite entries (0 when there is none), equal; the
    matrix a strided view inside a buffer of large sentinels, the one-element output inside a sentinel buffer."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fo = _sentinel(np.float64)
    codes = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.float16): torch.float16}
    for case in absmax_cases(SEED + 47, case_count(ABSMAX_CLASSES)):
        for npdt in ABSMAX_NP:
            x = case["x"].astype(npdt)
            n, c = x.shape
            tag = "case %d: class=%s %s n=%d c=%d off=%d pad=%d (PXSOM_FUZZ_SEED=%d)" % (
                case["i"], case["cls"], x.dtype, n, c, case["off"], case["pad"], SEED)
            # the columns beside the view hold a finite value larger than any entry: reading one of them shows
            _, xt = _view2d(gpu, x, case["off"], case["pad"], fill=npdt(30000.0))
            obuf, out = _view1d(gpu, np.full(1, fo), case["out_off"], 3, fo)
            rc = lib.pxsom_absmax(xt.data_ptr(), n, c, case["off"] + c + case["pad"],
                                  _capi.dtype_code(torch.empty(0, dtype=codes[np.dtype(npdt)])), out.data_ptr(),
                                  _capi.stream_ptr())
            torch.cuda.synchronize()
            assert rc == PXSOM_OK, tag
            got, want = float(out.item()), absmax_reference(x)
            assert got == want, tag + ": got %r, numpy %r" % (got, want)
            assert _guard_intact(obuf.cpu().numpy(), slice(case["out_off"], case["out_off"] + 1), fo), tag + ": guard"


# ---- pxsom_cluster_sums with arbitrary labels ---------------------------------------------------------------------
SUMS_PRIVATE_MIN_C, SUMS_PRIVATE_MAX_C, SUMS_PRIVATE_MIN_N = 13, 64, 32768     # pxsom_sums.hip cluster_sums_typed
SUMS_PAIRS_MIN_C = 14                                                          # launch_sums_pairs
SUMS_LDS_LIMIT, kSumsSpare = 150 * 1024, 16                                    # cluster_sums_typed, cluster_sums_kernel
CLUSTER_SUMS_CLASSES = ("interior", "c12", "c13", "c14", "c63", "c64", "c65", "n32767", "n32768", "odd_ldx",
                        "even_ldx", "base_plus_one", "flat_aligned", "flat_moved", "labels_mixed", "one_cluster",
                        "prefilled")
CLUSTER_SUMS_NP = (np.float32, np.float64, np.float16)


def sums_private_waves(c, k):
    """pxsom_sums.hip sums_private_waves: waves per workgroup whose private [k + 1, c] tables fit the LDS, 0 for none."""
    if not SUMS_PRIVATE_MIN_C <= c <= SUMS_PRIVATE_MAX_C:
        return 0
    tbytes, budget = ((k + 1) * c + 64) * 8, 160 * 1024 - 1024
    if 8 * tbytes + k * 8 <= budget or 4 * tbytes + k * 4 <= budget:
        return 4
    return 2 if 2 * tbytes + k * 4 <= budget else 0


def cluster_sums_route(n, c, ldx, elem_off, k, itemsize):
    """cluster_sums_typed: wave-private tables for 13 <= c <= 64 and n >= 32768 when they fit -- two channels per lane
    when c and ldx are even, c >= 14 and the base is aligned to a pair of elements (an even element offset in an
    aligned buffer) -- else cluster_sums_kernel, the workgroup table with LDS atomics: binary32 / binary16 rows that
    are contiguous (ldx == c) on a 16-byte aligned base, with the table in LDS, are read as one flat range of 16-byte
    vectors ("atomic_vector"), every other matrix element by element ("atomic")."""
    if n >= SUMS_PRIVATE_MIN_N and sums_private_waves(c, k):
        if c % 2 == 0 and ldx % 2 == 0 and c >= SUMS_PAIRS_MIN_C and elem_off % 2 == 0:
            return "pairs"
        return "private"
    lds_odd = (k * (c | 1) + kSumsSpare) * 8 + k * 4
    use_lds = min(lds_odd, (k * c + kSumsSpare) * 8 + k * 4) <= SUMS_LDS_LIMIT
    if itemsize <= 4 and use_lds and ldx == c and (elem_off * itemsize) % 16 == 0:
        return "atomic_vector"
    return "atomic"


def cluster_sums_cases(seed, count):
    """Cases of test_fuzz_cluster_sums: class i % 17 of CLUSTER_SUMS_CLASSES (17 classes: the default run is 17 cases)
    -- c and n on the edges of the wave-private and pair-load routes, odd and even row strides, the base moved by one
    element, a contiguous matrix on a 16-byte aligned base (the 16-byte vector loads of cluster_sums_kernel) and the
    same moved by 1 .. 3 elements (its alignment test fails: element by element), labels 0 / k + 1 / negative mixed
    in, every row in one cluster, tables that already hold values.  Rows are whole multiples of 1/256 within +-8,
    exact in all three storage types, so every partial sum is exact; each case runs in f32, f64 and f16, and `routes`
    gives the route per item size.  A `flat` case is a contiguous matrix at element `off` of a flat buffer."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        cls = CLUSTER_SUMS_CLASSES[i % len(CLUSTER_SUMS_CLASSES)]
        c = int(rs.choice([1, 4, 12, 13, 14, 16, 22, 40, 63, 64, 65]))
        n = int(rs.choice([32767, 32768, 40000, int(rs.randint(1, 5000))]))
        k = int(rs.randint(1, 65))
        off, pad = int(rs.choice([0, 0, 1, 2])), int(rs.choice([0, 0, 1, 2]))
        if cls[0] == "c" and cls[1:].isdigit():
            c, n = int(cls[1:]), int(rs.choice([32768, 40000]))
        elif cls[0] == "n" and cls[1:].isdigit():
            n, c = int(cls[1:]), int(rs.choice([14, 16, 22, 40]))
            off = pad = 0
        elif cls in ("odd_ldx", "even_ldx", "base_plus_one"):
            c, n = int(rs.choice([14, 16, 22, 40, 64])), int(rs.choice([32768, 40000]))
            off, pad = (1, 0) if cls == "base_plus_one" else (0, 1 if cls == "odd_ldx" else int(rs.choice([0, 2])))
            if cls == "base_plus_one":
                pad = 1                                    # an even stride: only the base keeps the pair loads away
        flat = cls in ("flat_aligned", "flat_moved")
        if flat:                # rows of whole vectors in f32 and f16 (16, 24), in f32 alone (12, 68), in neither (5, 13)
            c = int(rs.choice([12, 68, 16, 24, 5, 13]))
            n = int(rs.choice([32767, int(rs.randint(1, 5000))]))
            off, pad = 0 if cls == "flat_aligned" else int(rs.randint(1, 4)), 0
        x = rs.randint(-2048, 2049, size=(n, c)) / 256.0
        labels = rs.randint(1, k + 1, size=n).astype(np.int32)
        if cls == "labels_mixed" or rs.rand() < 0.3:
            bad = rs.rand(n) < 0.2
            labels[bad] = rs.choice([0, k + 1, -1, -(2 ** 31) + 1, 2 ** 31 - 1], size=int(bad.sum())).astype(np.int32)
        if cls == "one_cluster":
            labels[:] = int(rs.randint(1, k + 1))
        prefilled = cls == "prefilled" or rs.rand() < 0.3
        sums0 = rs.randint(-2 ** 20, 2 ** 20, size=(k, c)) / 256.0 if prefilled else np.zeros((k, c))
        counts0 = rs.randint(0, 2 ** 40, size=k).astype(np.int64) if prefilled else np.zeros(k, np.int64)
        ldx = c if flat else off + c + pad
        yield dict(i=i, cls=cls, x=x, labels=labels, k=k, sums0=sums0, counts0=counts0, off=off, pad=pad, flat=flat,
                   ldx=ldx, routes={s: cluster_sums_route(n, c, ldx, off, k, s) for s in (2, 4, 8)}, sums_off=int(rs.randint(0, 4)),
                   counts_off=int(rs.randint(0, 4)))


def test_fuzz_cluster_sums(gpu, oracle):
    """pxsom_cluster_sums with labels that no assign produced, in all three storage types, against
    oracle.cluster_sums added onto the same starting tables: sums and counts bit for bit (every partial sum is exact);
    sums and counts inside sentinel buffers, the rows a strided view."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fs, fc = _sentinel(np.float64), _sentinel(np.int64)
    codes = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.float16): torch.float16}
    for case in cluster_sums_cases(SEED + 48, case_count(CLUSTER_SUMS_CLASSES)):
        x64, labels, k = case["x"], case["labels"], case["k"]
        n, c = x64.shape
        ws, wc = oracle.cluster_sums(x64, labels, k)
        ws, wc = ws + case["sums0"], wc + case["counts0"]
        lt = torch.from_numpy(labels).to(gpu)
        for npdt in CLUSTER_SUMS_NP:
            x = x64.astype(npdt)
            assert np.array_equal(x.astype(np.float64), x64)
            tag = "case %d: class=%s route=%s %s n=%d c=%d k=%d off=%d ldx=%d (PXSOM_FUZZ_SEED=%d)" % (
                case["i"], case["cls"], case["routes"][x.dtype.itemsize], x.dtype, n, c, k, case["off"], case["ldx"], SEED)
            if case["flat"]:
                _, xt = _view1d(gpu, x, case["off"], 3, npdt(7.75))
            else:
                _, xt = _view2d(gpu, x, case["off"], case["pad"], fill=npdt(7.75))
            sbuf, sums = _view1d(gpu, case["sums0"], case["sums_off"], 5, fs)
            cbuf, counts = _view1d(gpu, case["counts0"], case["counts_off"], 5, fc)
            rc = lib.pxsom_cluster_sums(xt.data_ptr(), n, c, case["ldx"],
                                        _capi.dtype_code(torch.empty(0, dtype=codes[np.dtype(npdt)])), lt.data_ptr(), k,
                                        sums.data_ptr(), counts.data_ptr(), _capi.stream_ptr())
            torch.cuda.synchronize()
            assert rc == PXSOM_OK, tag
            assert np.array_equal(counts.cpu().numpy(), wc), tag + ": counts"
            assert _bytes_equal(sums.cpu().numpy() + 0.0, ws + 0.0), tag + ": sums"
            assert _guard_intact(sbuf.cpu().numpy(), slice(case["sums_off"], case["sums_off"] + k * c), fs), tag + ": sums guard"
            assert _guard_intact(cbuf.cpu().numpy(), slice(case["counts_off"], case["counts_off"] + k), fc), tag + ": counts guard"


FAMILIES = {"blur_hwc": (blur_hwc_cases, 40, BLUR_HWC_CLASSES), "rowfilter": (rowfilter_cases, 41, ROWFILTER_CLASSES),
            "quantile": (quantile_cases, 42, QUANTILE_CLASSES),
            "scaled_rowsum": (scaled_rowsum_cases, 44, SCALED_ROWSUM_CLASSES),
            "normalize_columns": (normalize_columns_cases, 45, NORMALIZE_CLASSES),
            "label_kernel": (label_kernel_cases, 46, LABEL_CLASSES), "absmax": (absmax_cases, 47, ABSMAX_CLASSES),
            "cluster_sums": (cluster_sums_cases, 48, CLUSTER_SUMS_CLASSES)}
