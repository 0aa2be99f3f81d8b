"""Randomised parity sweep of the image kernels: K10 pxsom_segmask (segmentation_mask), K11 pxsom_gaussian_blur_plane and
pxsom_zero_by_seg, K12 pxsom_cellquant (cell_quantify), each against its plain reference -- tests/cell_mask_reference.py,
live scipy.ndimage.gaussian_filter / numpy indexing, tests/cell_table_reference.py -- on shapes, strides, dtypes, tables
and cell sizes drawn at random (seeded) around the routes each kernel picks.  Case i of a generator first takes route
class i % R from a fixed list, then draws the rest within that class, so the default 12 cases visit every class.  Every
caller-provided output is a slice of a larger buffer filled with a sentinel: a store outside the slice fails as a wrong
value.  ``PXSOM_FUZZ_CASES`` / ``PXSOM_FUZZ_SEED`` as in test_gpu_fuzz_parity.py.  The generators are device-free
(tests/test_fuzz_generators.py checks them on CPU)."""
import os

import numpy as np
import pytest

from tests import cell_mask_reference as cr
from tests import cell_table_reference as ctr

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("PXSOM_FUZZ_CASES", "12"))
SEED = int(os.environ.get("PXSOM_FUZZ_SEED", "20260928"))

SEG_NP = (np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64)
PLANE_NP = (np.uint8, np.int16, np.uint16, np.int32, np.float32)
DENSE_MAX_ENTRIES = 1 << 24


def lut_route(n_keys, kmin, kmax):
    """The K10 rule (pxsom_segmask_workspace_bytes, the key tables of pxsom_cellquant): a dense LUT over
    [kmin, kmax] when range <= 2^24 and range <= 16 n_keys + 65536, else a binary search."""
    if n_keys <= 0 or kmax < kmin:
        return False
    rng = int(kmax) - int(kmin) + 1
    return rng <= DENSE_MAX_ENTRIES and rng <= 16 * int(n_keys) + 65536


def _torch_dt(npdt):
    import torch
    return {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.uint16): torch.uint16,
            np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.uint32, np.dtype(np.int64): torch.int64,
            np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(npdt)]


def _sentinel(npdt):
    """A fill no kernel output is likely to equal: 0x5A in every byte."""
    return np.frombuffer(b"\x5a" * np.dtype(npdt).itemsize, dtype=npdt)[0]


def _bytes_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                 np.ascontiguousarray(b).view(np.uint8))


def _view2d(gpu, arr, off, pad, top=0, bottom=0, fill=None):
    """(buffer, view): `arr` [h, w] written into columns off .. off + w of an [top + h + bottom, off + w + pad] buffer
    (row stride off + w + pad) at row `top`; the rest holds `fill` (zero by default)."""
    import torch
    h, w = arr.shape
    npbuf = np.full((top + h + bottom, off + w + pad), fill if fill is not None else 0, dtype=arr.dtype)
    npbuf[top:top + h, off:off + w] = arr
    buf = torch.from_numpy(npbuf).to(gpu)
    return buf, buf[top:top + h, off:off + w]


def _view1d(gpu, arr, off, tail, fill):
    """(buffer, view): the flat `arr` at element `off` of a buffer of off + size + tail elements filled with `fill`."""
    import torch
    flat = np.ascontiguousarray(arr).reshape(-1)
    npbuf = np.full(off + flat.size + tail, fill, dtype=arr.dtype)
    npbuf[off:off + flat.size] = flat
    buf = torch.from_numpy(npbuf).to(gpu)
    return buf, buf[off:off + flat.size].view(arr.shape)


def _guard_intact(buf_host, region, fill):
    """Every element of buf_host outside the index `region` still holds `fill`, bit for bit."""
    mask = np.ones(buf_host.shape, dtype=bool)
    mask[region] = False
    return _bytes_equal(buf_host[mask], np.full(int(mask.sum()), fill, dtype=buf_host.dtype))


# ---- K10 pxsom_segmask --------------------------------------------------------------------------------------------
SEGMASK_ROUTES = ("no_table", "lut", "search", "lut_edge", "search_edge", "empty_table")


def _wrap_to(rs, key, npdt):
    """A label of dtype npdt whose int32 cast is `key`, or None when the dtype has none."""
    info = np.iinfo(npdt)
    if np.dtype(npdt) == np.int64:
        return int(key) + (1 << 32) * int(rs.choice([0, 0, 0, 1, -1, 3]))
    if np.dtype(npdt) == np.uint32:
        return int(key) % (1 << 32)
    return int(key) if info.min <= key <= info.max else None


def _draw_dim(rs, anchors):
    u = rs.rand()
    if u < 0.45:
        return int(max(1, min(600, int(rs.choice(anchors)) + int(rs.randint(-3, 4)))))
    return int(rs.randint(1, 601))


def segmask_cases(seed, count):
    """Cases of test_fuzz_segmask: route class i % 6 of SEGMASK_ROUTES (no lookup, LUT, binary search, the range just
    at and just past 16 n_keys + 65536, the empty table), then label dtype, shape, input and output views, erosion,
    connectivity, background, output dtype and table values at random."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        route = SEGMASK_ROUTES[i % len(SEGMASK_ROUTES)]
        npdt = SEG_NP[int(rs.randint(0, len(SEG_NP)))]
        if route in ("search", "search_edge") and np.iinfo(npdt).max < 2 ** 31:
            npdt = (np.int32, np.uint32, np.int64)[int(rs.randint(0, 3))]     # 8 / 16-bit labels: the key range
        h = _draw_dim(rs, [4, 8, 64, 128, 256, 300, 512])
        w = _draw_dim(rs, [64, 256, 512])
        # the table first (key space int32), then labels that wrap onto its keys and a few that miss it
        keys = np.zeros(0, np.int64)
        if route in ("lut", "search", "lut_edge", "search_edge"):
            n_keys = int(rs.randint(1 if route == "lut" else 2, 60))
            if route == "lut":
                span = 1 if n_keys == 1 else int(rs.randint(n_keys, 65537))   # LUT whatever unique() leaves
            elif route == "search":
                span = int(rs.choice([16 * n_keys + 65537 + int(rs.randint(0, 10 ** 6)), 2 ** 31 - 5,
                                      DENSE_MAX_ENTRIES + 1]))
                span = max(span, 16 * n_keys + 65537)
            else:
                span = 16 * n_keys + 65536 + (route == "search_edge")
            info = np.iinfo(npdt)
            lo_min = -(2 ** 31) if info.min < 0 or np.dtype(npdt).itemsize >= 4 else 0
            if np.dtype(npdt).itemsize < 4 and rs.rand() < 0.8:           # keys the 8 / 16-bit labels can hold
                kmin = int(rs.randint(max(lo_min, int(info.min) - span // 2), int(info.max) + 1))
            elif rs.rand() < 0.7:
                kmin = int(rs.randint(lo_min, 2 ** 31 - span + 1))
            else:
                kmin = max(lo_min, -(span // 2))
            kmax = kmin + span - 1
            inner = rs.randint(kmin, kmax + 1, size=max(0, n_keys - 2)) if n_keys > 2 else np.zeros(0, np.int64)
            keys = np.unique(np.concatenate([[kmin, kmax], inner]).astype(np.int64))
            if route in ("lut_edge", "search_edge"):     # unique() may have merged keys: keep the range on the edge
                while keys.size < n_keys:
                    keys = np.unique(np.concatenate([keys, rs.randint(kmin, kmax + 1, size=n_keys - keys.size)]))
        pool = [_wrap_to(rs, int(v), npdt) for v in keys]
        info = np.iinfo(npdt)
        extra = rs.randint(max(info.min, -(2 ** 40)), min(info.max, 2 ** 40) + 1, size=int(rs.randint(1, 12)),
                           dtype=np.int64)
        pool = np.array([v for v in pool if v is not None] + list(extra) + [0, 1, info.max, info.min], dtype=np.int64)
        ny, nx = int(rs.randint(1, min(h, 24) + 1)), int(rs.randint(1, min(w, 24) + 1))
        ids = rs.choice(pool, size=(ny, nx))
        ry = np.sort(rs.randint(0, ny, size=h))
        rx = np.sort(rs.randint(0, nx, size=w))
        seg = ids[ry[:, None], rx[None, :]]
        spots = rs.rand(h, w) < float(rs.choice([0.0, 0.02, 0.2]))
        seg[spots] = rs.choice(pool, size=int(spots.sum()))            # single-pixel cells
        seg = seg.astype(npdt)
        out_kind = str(rs.choice(["i16", "i32", "f64", "same"]))
        out_np = {"i16": np.int16, "i32": np.int32, "f64": np.float64, "same": npdt}[out_kind]
        if route == "no_table":
            keys_t = values = None
            unassigned = 0
        else:
            keys_t = keys.astype(np.int32)
            if out_np == np.float64:
                values = rs.randn(keys_t.size) * 10.0 ** int(rs.randint(0, 6))
                unassigned = float(rs.choice([np.nan, -0.5, 0.0, 1e300]))
            else:
                values = rs.randint(-70000, 70001, size=keys_t.size)       # narrows in int16 / uint8 / uint16
                unassigned = int(rs.choice([0, -3, 40000, 2 ** 31 - 1, -(2 ** 31)]))
        present = np.unique(seg)
        yield dict(i=i, route=route, seg=seg, h=h, w=w,
                   erode=[None, "thick", "inner"][int(rs.randint(0, 3))],
                   conn=int(rs.choice([1, 2, 3, 1, 2, 0, -1] if rs.rand() < 0.15 else [1, 2, 3])),
                   background=int(rs.choice(present)) if rs.rand() < 0.7 else 0,
                   keys=keys_t, values=values, unassigned=unassigned, out_np=out_np,
                   in_off=int(rs.randint(0, 9)), in_pad=int(rs.choice([0, 0, 1, 3, 8])),
                   out_off=int(rs.randint(0, 9)), out_pad=int(rs.choice([0, 0, 1, 2, 5])), out_rows=int(rs.randint(0, 3)),
                   lut=keys_t is not None and lut_route(keys_t.size, int(keys_t[0]) if keys_t.size else 0,
                                                        int(keys_t[-1]) if keys_t.size else 0))


def test_fuzz_segmask(gpu):
    """segmentation_mask against cell_mask_reference.segmask, array_equal with the dtype, into a row-strided output
    view at a column offset inside a sentinel-filled buffer; LUT-route cases again with force_search."""
    import torch
    from ark_analysis_amd import _capi, som_device
    lib = _capi.lib()
    for case in segmask_cases(SEED + 30, CASES):
        seg, h, w = case["seg"], case["h"], case["w"]
        keys, values = case["keys"], case["values"]
        tag = "case %d: route=%s %s %dx%d erode=%s conn=%d bg=%d out=%s n_keys=%s range=%s unassigned=%r " \
              "in(off=%d pad=%d) out(off=%d pad=%d rows=%d) (PXSOM_FUZZ_SEED=%d)" % (
                  case["i"], case["route"], seg.dtype, h, w, case["erode"], case["conn"], case["background"],
                  np.dtype(case["out_np"]), None if keys is None else keys.size,
                  None if keys is None or not keys.size else (int(keys[0]), int(keys[-1])), case["unassigned"],
                  case["in_off"], case["in_pad"], case["out_off"], case["out_pad"], case["out_rows"], SEED)
        if keys is not None and keys.size:
            assert (lib.pxsom_segmask_workspace_bytes(keys.size, int(keys[0]), int(keys[-1])) > 0) == case["lut"], tag
        _, seg_t = _view2d(gpu, seg, case["in_off"], case["in_pad"])
        out_np = np.dtype(case["out_np"])
        fill = _sentinel(out_np)
        want = cr.segmask(seg, case["erode"], case["conn"], case["background"], keys, values, case["unassigned"], out_np)
        table = None if keys is None else som_device.segmask_table(keys, values, gpu,
                                                                   float_values=out_np == np.float64)
        runs = [False, True] if case["lut"] else [False]
        for force in runs:
            top = case["out_rows"]
            obuf, out = _view2d(gpu, np.full((h, w), fill, out_np), case["out_off"], case["out_pad"], top, top, fill)
            res = som_device.segmentation_mask(seg_t, erode=case["erode"], connectivity=case["conn"],
                                               background=case["background"], table=table,
                                               unassigned=case["unassigned"], out_dtype=_torch_dt(out_np),
                                               force_search=force, out=out)
            assert res.data_ptr() == out.data_ptr(), tag
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            t = tag + (" force_search" if force else "")
            assert got.dtype == want.dtype and got.shape == want.shape, t
            assert np.array_equal(got, want, equal_nan=out_np.kind == "f"), t + ": %d pixels differ" % int(
                (~((got == want) | (np.isnan(got) & np.isnan(want)) if out_np.kind == "f" else got == want)).sum())
            region = (slice(top, top + h), slice(case["out_off"], case["out_off"] + w))
            assert _guard_intact(obuf.cpu().numpy(), region, fill), t + ": stores outside the output view"


# ---- K11 pxsom_gaussian_blur_plane, pxsom_zero_by_seg -------------------------------------------------------------
BLUR_ROUTES = ("short_plane", "copy", "in_place", "out_of_place")
BLUR_SIGMA_LIMIT = 16.125


def _radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def _plane_values(rs, npdt, h, w):
    if np.dtype(npdt) == np.float32:
        x = (rs.standard_normal(size=(h, w)) * 10.0 ** float(rs.uniform(-3, 6))).astype(np.float32)
        x[rs.rand(h, w) < 0.2] = 0
        u = rs.rand()
        if u < 0.5:
            big = rs.rand(h, w) < 0.02
            x[big] = (rs.uniform(0.5, 1.0, size=int(big.sum())) * np.finfo(np.float32).max).astype(np.float32)
            for v in (np.nan, np.inf, -np.inf):
                if rs.rand() < 0.6:
                    x[rs.randint(0, h), rs.randint(0, w)] = v
        return x
    info = np.iinfo(npdt)
    lo, hi = (info.min, info.max) if np.dtype(npdt) != np.int32 else (-2_000_000_000, 2_000_000_000)
    return rs.randint(lo, hi, size=(h, w), dtype=np.int64).astype(npdt)


def blur_cases(seed, count):
    """Cases of test_fuzz_blur_plane: class i % 4 -- a plane shorter than the radius in both axes, sigma <= 1e-15 (a
    copy), in place, out of place -- then dtype, shape, sigma from (0, 16.125) and element offsets at random."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        route = BLUR_ROUTES[i % len(BLUR_ROUTES)]
        npdt = PLANE_NP[int(rs.randint(0, len(PLANE_NP)))]
        if route == "copy":
            sigma = float(rs.choice([0.0, 1e-16, 1e-15, -1.0, 5e-324]))
        elif rs.rand() < 0.5:
            sigma = float(rs.uniform(0.0, BLUR_SIGMA_LIMIT))
        else:
            sigma = float(np.exp(rs.uniform(np.log(1e-3), np.log(BLUR_SIGMA_LIMIT))))
        if route == "short_plane":
            sigma = float(rs.uniform(0.4, BLUR_SIGMA_LIMIT))
            r = _radius(sigma)
            h, w = int(rs.randint(1, r + 1)), int(rs.randint(1, r + 1))
        else:
            h = int(rs.randint(1, 401)) if rs.rand() < 0.7 else int(rs.choice([1, 2, 3, 64, 65, 127, 128, 129]))
            w = int(rs.randint(1, 401)) if rs.rand() < 0.7 else int(rs.choice([1, 2, 3, 64, 65, 127, 128, 129]))
        assert sigma < BLUR_SIGMA_LIMIT
        yield dict(i=i, route=route, plane=_plane_values(rs, npdt, h, w), sigma=sigma,
                   in_place=route == "in_place" or (route == "copy" and rs.rand() < 0.5),
                   off=int(rs.randint(0, 17)), tail=int(rs.randint(0, 17)), out_off=int(rs.randint(0, 17)),
                   out_tail=int(rs.randint(0, 17)))


def test_fuzz_blur_plane(gpu):
    """gaussian_blur_plane against live scipy.ndimage.gaussian_filter, equal with the dtype (test_channel_edits._same),
    plane and output at element offsets inside sentinel-filled buffers, in place and out of place."""
    import scipy.ndimage as ndimage
    import torch
    from ark_analysis_amd import som_device
    from tests.test_channel_edits import _same
    for case in blur_cases(SEED + 31, CASES):
        plane, sigma = case["plane"], case["sigma"]
        h, w = plane.shape
        tag = "case %d: route=%s %s %dx%d sigma=%r in_place=%s off=%d tail=%d out_off=%d out_tail=%d " \
              "(PXSOM_FUZZ_SEED=%d)" % (case["i"], case["route"], plane.dtype, h, w, sigma, case["in_place"],
                                        case["off"], case["tail"], case["out_off"], case["out_tail"], SEED)
        fill = _sentinel(plane.dtype)
        pbuf, pt = _view1d(gpu, plane, case["off"], case["tail"], fill)
        if case["in_place"]:
            out = pt
        else:
            obuf, out = _view1d(gpu, np.full(plane.shape, fill, plane.dtype), case["out_off"], case["out_tail"], fill)
        with np.errstate(all="ignore"):
            want = ndimage.gaussian_filter(plane, sigma)
        res = som_device.gaussian_blur_plane(pt, sigma, out=out)
        assert res.data_ptr() == out.data_ptr(), tag
        torch.cuda.synchronize()
        try:
            _same(out.cpu().numpy(), want)
        except AssertionError as e:
            raise AssertionError(tag + ": " + str(e)) from e
        n = h * w
        assert _guard_intact(pbuf.cpu().numpy(), slice(case["off"], case["off"] + n), fill), tag + ": plane guard"
        if not case["in_place"]:
            assert _bytes_equal(pt.cpu().numpy(), plane), tag + ": the input plane changed"
            assert _guard_intact(obuf.cpu().numpy(), slice(case["out_off"], case["out_off"] + n), fill), \
                tag + ": output guard"


def zero_cases(seed, count):
    """Cases of test_fuzz_zero_by_segmentation: image dtype i % 5; each case runs every segmentation dtype, with
    lengths whose remainders mod 16 go round all 16 over the cases, at random element offsets."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        npdt = PLANE_NP[i % len(PLANE_NP)]
        runs = []
        for j, sdt in enumerate(SEG_NP):
            n = 16 * int(rs.choice([0, 1, 2, 7, 64, 1000, int(rs.randint(0, 20000))])) + (i * len(SEG_NP) + j) % 16
            n = max(n, 1)
            info = np.iinfo(sdt)
            seg = rs.randint(-3 if info.min < 0 else 0, 4, size=n).astype(sdt)
            seg[rs.randint(0, n)] = info.max
            if info.min < 0:
                seg[rs.randint(0, n)] = info.min
            runs.append(dict(seg=seg, img=_plane_values(rs, npdt, 1, n).reshape(n), exclude=bool(rs.rand() < 0.5),
                             off=int(rs.randint(0, 33)), tail=int(rs.randint(0, 33))))
        yield dict(i=i, dtype=npdt, runs=runs)


def test_fuzz_zero_by_segmentation(gpu):
    import torch
    from ark_analysis_amd import som_device
    from tests.test_channel_edits import _same
    for case in zero_cases(SEED + 32, CASES):
        for run in case["runs"]:
            img, seg = run["img"], run["seg"]
            n = img.size
            tag = "case %d: img %s seg %s n=%d (n %% 16 = %d) exclude=%s off=%d tail=%d (PXSOM_FUZZ_SEED=%d)" % (
                case["i"], img.dtype, seg.dtype, n, n % 16, run["exclude"], run["off"], run["tail"], SEED)
            fill = _sentinel(img.dtype)
            buf, t = _view1d(gpu, img, run["off"], run["tail"], fill)
            som_device.zero_by_segmentation(t, torch.from_numpy(seg).to(gpu), run["exclude"])
            want = img.copy()
            want[seg > 0 if run["exclude"] else seg == 0] = 0
            try:
                _same(t.cpu().numpy(), want)
            except AssertionError as e:
                raise AssertionError(tag + ": " + str(e)) from e
            assert _guard_intact(buf.cpu().numpy(), slice(run["off"], run["off"] + n), fill), tag + ": guard"


# ---- K12 pxsom_cellquant ------------------------------------------------------------------------------------------
CELLQUANT_ROUTES = ("pairwise", "fold_wide", "nuc_overflow", "nuc_other_route")
CELL_SIZES = (1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 16385)
NUC_CAPACITY_DEFAULT = 128
IMG_NP = (np.uint8, np.int16, np.uint16, np.int32, np.float32, np.float64)


def _image(rs, h, w, c, npdt):
    if np.dtype(npdt).kind == "f":
        x = rs.gamma(0.6, 3.0, size=(h, w, c)) * (rs.rand(h, w, c) < 0.7)
        if rs.rand() < 0.5:
            x *= 10.0 ** rs.uniform(-6, 6, size=(1, 1, c))
        return x.astype(npdt)
    info = np.iinfo(npdt)
    hi = int(min(info.max, rs.choice([3000, info.max])))
    lo = int(max(info.min, -hi)) if rs.rand() < 0.3 else 0
    return rs.randint(lo, hi + 1, size=(h, w, c), dtype=np.int64).astype(npdt)


def _place_runs(rs, seg, sizes, first_label):
    """Overwrite disjoint regions of exactly `sizes` pixels with new labels first_label, first_label + 1, ...; each region
    a raster run (wrapping rows) or, when the size factors into the width, a rectangle below the runs before it."""
    h, w = seg.shape
    flat = seg.reshape(-1)
    pos = 0
    lab = first_label
    for s in sizes:
        gap = int(rs.randint(0, 40))
        if pos + gap + s > flat.size:
            break
        pos += gap
        r0 = (pos + w - 1) // w
        rect = [(a, s // a) for a in range(2, min(h - r0, s) + 1) if s % a == 0 and s // a <= w]
        if rect and rs.rand() < 0.4:
            a, b = rect[int(rs.randint(0, len(rect)))]
            c0 = int(rs.randint(0, w - b + 1))
            seg[r0:r0 + a, c0:c0 + b] = lab
            pos = (r0 + a) * w
        else:
            flat[pos:pos + s] = lab
            pos += s
        lab += 1
    return seg


def _sparse_labels(rs, n):
    """n distinct labels spread over 1 .. 2^31 - 1 (a key range no LUT takes), sorted; sometimes the largest int32."""
    v = np.unique(rs.randint(1, 2 ** 31 - 1, size=2 * n + 8, dtype=np.int64))
    v = np.sort(rs.choice(v, size=n, replace=False))
    if rs.rand() < 0.5:
        v[-1] = 2 ** 31 - 1
    return v


def _max_nuclei_per_cell(seg, nuc):
    s, q = seg.astype(np.int64).ravel(), nuc.astype(np.int64).ravel()
    m = (s != 0) & (q != 0)
    if not m.any():
        return 0
    pairs = np.unique(np.stack([s[m], q[m]], 1), axis=0)
    return int(np.bincount(np.unique(pairs[:, 0], return_inverse=True)[1]).max())


def cellquant_cases(seed, count):
    """Cases of test_cell_quantify: class i % 4 of CELLQUANT_ROUTES -- one float channel (numpy's pairwise sum) with
    cells on its 8 / 128 / 8192 / 16384 edges; 63 .. 257 channels (a third walk past 256); a nuclear image with more
    distinct nuclei in a cell than nuc_capacity; the cell and the nuclear key tables on different routes (LUT / search)
    -- then mode, dtypes, label strides, threshold, nuclear capacity and an explicit key subset at random."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        route = CELLQUANT_ROUTES[i % len(CELLQUANT_ROUTES)]
        mode = ctr.MODES[int(rs.randint(0, 3))]
        cap = int(rs.choice([1, 2, 3, 64, 65, 128, 0]))
        if route != "nuc_overflow" and rs.rand() < 0.4:
            cap = 0
        if route == "pairwise":
            c, mode = 1, "total_intensity"
            img_np = (np.float32, np.float64)[int(rs.randint(0, 2))]
            big = [int(v) for v in rs.choice([8191, 8192, 8193, 16385], size=int(rs.randint(1, 3)), replace=False)]
            small = [int(v) for v in rs.choice([1, 7, 8, 9, 127, 128, 129], size=int(rs.randint(3, 10)))]
            sizes = big + small
            h = int(rs.randint(96, 200))
            w = int(max(64, (sum(sizes) + 40 * len(sizes)) // h + int(rs.randint(1, 40))))
        else:
            if route == "fold_wide" or rs.rand() < 0.3:
                c = int(rs.choice([63, 64, 65, 127, 128, 129, 255, 256, 257]))
            else:
                c = int(rs.choice([1, 2, 3, 63, 64, 65])) if rs.rand() < 0.7 else int(rs.randint(1, 258))
            img_np = IMG_NP[int(rs.randint(0, len(IMG_NP)))]
            sizes = [int(v) for v in rs.choice([1, 7, 8, 9, 127, 128, 129], size=int(rs.randint(2, 8)))]
            h, w = int(rs.randint(8, 120)), int(rs.randint(8, 160))
            if c <= 3 and rs.rand() < 0.3:
                sizes.append(int(rs.choice([8191, 8192, 8193])))
                h, w = max(h, 100), max(w, 120)
            if route == "nuc_overflow":                                   # a cell that can meet capacity + 8 nuclei
                sizes.append((cap or NUC_CAPACITY_DEFAULT) + 8 + int(rs.randint(0, 100)))
                h, w = max(h, 40), max(w, 60)
        # labels: a Voronoi base, exact-size runs, sometimes fragmented labels; dtype, spread (key route) after
        n_cells = int(rs.randint(2, max(3, min(1500, h * w // 12))))
        base = ctr.voronoi_labels(h, w, n_cells, seed=int(rs.randint(0, 2 ** 31)), background=float(rs.uniform(0, 0.3)),
                                  dtype=np.int64)
        if rs.rand() < 0.3 and h > 4 and w > 4:
            present = np.unique(base[base > 0])
            if present.size:
                base = ctr.fragment(base, rs.choice(present, size=min(3, present.size), replace=False), pieces=4,
                                    seed=int(rs.randint(0, 1000)))
        seg = _place_runs(rs, base, sizes, n_cells + 1)
        present = np.unique(seg[seg > 0])
        seg_np = SEG_NP[int(rs.randint(0, len(SEG_NP)))]
        want_search = route == "nuc_other_route" and rs.rand() < 0.5          # cells on search, nuclei on the LUT
        if want_search:
            seg_np = (np.int32, np.uint32, np.int64)[int(rs.randint(0, 3))]
        if present.size > 250 and seg_np == np.uint8:
            seg_np = np.uint16
        relabel = np.zeros(int(seg.max()) + 1, np.int64)
        if want_search:
            new = _sparse_labels(rs, present.size)
        else:
            top = min(np.iinfo(seg_np).max, 2 ** 31 - 1)
            new = np.sort(rs.choice(np.arange(1, min(top, 5 * present.size + 10) + 1), size=present.size, replace=False))
        relabel[present] = rs.permutation(new)
        seg = relabel[seg].astype(seg_np)
        keys_all = np.unique(seg[seg != 0]).astype(np.int64)
        # nuclear image
        nuc = None
        if route in ("nuc_overflow", "nuc_other_route") or rs.rand() < 0.3:
            nuc_np = SEG_NP[int(rs.randint(0, len(SEG_NP)))]
            nuc_search = route == "nuc_other_route" and not want_search
            if nuc_search:
                nuc_np = (np.int32, np.uint32, np.int64)[int(rs.randint(0, 3))]
            while nuc_np == seg_np and route != "nuc_other_route":
                nuc_np = SEG_NP[int(rs.randint(0, len(SEG_NP)))]
            top = min(np.iinfo(nuc_np).max, 2 ** 31 - 1)
            n_nuc = int(min(top, rs.choice([40, 200, 400, 3000] if route != "nuc_overflow" else [200, 400, 3000])))
            if nuc_search:
                pool = _sparse_labels(rs, n_nuc)
            else:
                pool = np.arange(1, n_nuc + 1)
            step = int(rs.choice([1, 2, 3]))
            nuc = np.zeros((h, w), np.int64)
            nuc[::step, ::step] = rs.choice(pool, size=nuc[::step, ::step].shape)
            nuc[rs.rand(h, w) < 0.3] = 0
            if route == "nuc_overflow":                # the largest cell meets limit + 1 .. limit + 8 distinct nuclei
                limit = cap or NUC_CAPACITY_DEFAULT
                labs, cnts = np.unique(seg[seg != 0], return_counts=True)
                cell = np.argwhere(seg == labs[np.argmax(cnts)])
                m = min(cell.shape[0], limit + int(rs.randint(1, 9)))
                nuc[tuple(cell[rs.choice(cell.shape[0], m, replace=False)].T)] = rs.choice(pool, size=m, replace=False)
            elif route != "nuc_other_route" and rs.rand() < 0.2:
                nuc[:, :] = 0                                                # no nucleus at all
            nuc = nuc.astype(nuc_np)
        # mode details
        if mode == "positive_pixel":
            threshold = float(rs.choice([0.0, 0.1, 1.0 / 3.0, 1e-8, 1e40, 2.5, float(rs.uniform(-5, 3000))]))
        else:
            threshold = 0.0
        keys = None
        if keys_all.size >= 2 and rs.rand() < 0.2:
            keep = rs.rand(keys_all.size) < 0.6
            drop = int(rs.randint(0, keys_all.size))
            keep[drop] = False                                             # a strict subset
            keep[(drop + 1) % keys_all.size] |= not keep.any()
            keys = keys_all[keep]
        img = _image(rs, h, w, c, img_np)
        if c == 1 and rs.rand() < 0.5:
            img = img[:, :, 0]
        nuc_keys = None if nuc is None else np.unique(nuc[nuc != 0]).astype(np.int64)
        info = dict(
            i=i, route=route, mode=mode, seg=seg, img=img, c=c, nuc=nuc, cap=cap, threshold=threshold, keys=keys,
            seg_off=int(rs.randint(0, 6)), seg_pad=int(rs.choice([0, 0, 3, 64])),
            nuc_off=int(rs.randint(0, 6)), nuc_pad=int(rs.choice([0, 0, 1, 7])),
            force_search=route != "nuc_other_route" and bool(rs.rand() < 0.15))
        k_tab = keys if keys is not None else keys_all
        info["cell_lut"] = lut_route(k_tab.size, int(k_tab[0]) if k_tab.size else 0, int(k_tab[-1]) if k_tab.size else 0)
        info["nuc_lut"] = None if nuc is None else lut_route(nuc_keys.size, int(nuc_keys[0]) if nuc_keys.size else 0,
                                                              int(nuc_keys[-1]) if nuc_keys.size else 0)
        info["max_nuclei"] = 0 if nuc is None else _max_nuclei_per_cell(seg, nuc)
        info["overflow"] = nuc is not None and info["max_nuclei"] > (cap or NUC_CAPACITY_DEFAULT)
        info["pairwise"] = c == 1 and np.dtype(img_np).kind == "f" and mode == "total_intensity"
        info["walks"] = (c + 127) // 128
        info["sizes"] = np.bincount(np.unique(seg.ravel().astype(np.int64), return_inverse=True)[1])
        yield info


def _subset(want, keys):
    rows = np.searchsorted(want["keys"].astype(np.int64), keys)
    out = {k: (v[rows] if k not in ("nuc_keys",) else v) for k, v in want.items()}
    out["keys"] = keys.astype(np.int32)
    return out


def test_cell_quantify(gpu):
    """cell_quantify against cell_table_reference.quantify, held to test_gpu_cell_table._check (keys, count, sums,
    bbox, nuc exact; values exact, center_weighting within center_weighting_bound); strided label and nuclear images
    of different dtypes, both key-table routes, nuclear overflow, thresholds not exact in binary32, key subsets."""
    import torch
    from ark_analysis_amd import _capi, som_device
    from ark_analysis_amd.segmentation.marker_quantification import _threshold_for
    from tests.test_gpu_cell_table import _check
    lib = _capi.lib()
    for case in cellquant_cases(SEED + 33, CASES):
        seg, img, nuc = case["seg"], case["img"], case["nuc"]
        h, w = seg.shape
        tag = "case %d: route=%s mode=%s seg %s %dx%d img %s c=%d nuc %s cap=%d max_nuclei=%d threshold=%r " \
              "keys=%s seg(off=%d pad=%d) nuc(off=%d pad=%d) force_search=%s cell_lut=%s nuc_lut=%s " \
              "largest cell=%d (PXSOM_FUZZ_SEED=%d)" % (
                  case["i"], case["route"], case["mode"], seg.dtype, h, w, img.dtype, case["c"],
                  None if nuc is None else nuc.dtype, case["cap"], case["max_nuclei"], case["threshold"],
                  "all" if case["keys"] is None else "subset of %d" % case["keys"].size, case["seg_off"],
                  case["seg_pad"], case["nuc_off"], case["nuc_pad"], case["force_search"], case["cell_lut"],
                  case["nuc_lut"], int(case["sizes"][1:].max()) if case["sizes"].size > 1 else 0, SEED)
        _, seg_t = _view2d(gpu, seg, case["seg_off"], case["seg_pad"])
        nuc_t = None if nuc is None else _view2d(gpu, nuc, case["nuc_off"], case["nuc_pad"])[1]
        keys_t = None if case["keys"] is None else torch.from_numpy(case["keys"].astype(np.int32)).to(gpu)
        with np.errstate(over="ignore"):
            thr = _threshold_for(img.dtype, case["threshold"])
        got = som_device.cell_quantify(seg_t, torch.from_numpy(img).to(gpu), keys=keys_t, mode=case["mode"],
                                       threshold=thr, nuc=nuc_t, nuc_capacity=case["cap"],
                                       force_search=case["force_search"])
        kt = got["keys"].cpu().numpy()
        if kt.size:
            assert (lib.pxsom_segmask_workspace_bytes(kt.size, int(kt[0]), int(kt[-1])) > 0) == case["cell_lut"], tag
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        with np.errstate(over="ignore", invalid="ignore"):
            want = ctr.quantify(seg, img, case["mode"], case["threshold"], nuc=nuc)
        if case["keys"] is not None:
            want = _subset(want, case["keys"])
        try:
            _check(got, want, seg, img, case["mode"])
        except AssertionError as e:
            raise AssertionError(tag + ": " + str(e)) from e
