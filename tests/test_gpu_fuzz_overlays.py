"""Randomised parity sweep of K29 (csrc/pxsom_overlay.hip, pxsom_percentile_f32_listq of csrc/pxsom_pre.hip) against the
numpy statement of tests/overlay_reference.py and live numpy, array_equal, by route class: case i of a generator takes
class i % R of a fixed tuple and draws the rest, so a default run (max(12, R) cases) visits every class.  Every buffer a
kernel writes -- rgb, borders, out, status, the percentile output and workspace -- is a slice at a drawn offset of a sentinel
buffer whose rest must still hold the sentinel afterwards; for the byte outputs the offset is in bytes, so that the base
is 0, 1, 2 or 3 bytes off a 4-byte boundary (torch allocations are 256-byte aligned).  pxsom_overlay_rgb runs through
som_device.overlay_compose with explicit modes and ranges; pxsom_colorize through _capi, so that the status word too lies
in a guard, and again through som_device.colorize(out=), which allocates the status itself; the percentiles through _capi.  ``PXSOM_FUZZ_CASES`` /
``PXSOM_FUZZ_SEED`` as in test_gpu_fuzz_preprocessing.py.  The generators are device-free (tests/test_fuzz_generators.py
checks them on CPU)."""
import numpy as np
import pytest

from tests import overlay_reference as ovr
from tests.test_gpu_fuzz_images import PLANE_NP, SEG_NP, _guard_intact, _sentinel, _view1d, _view2d
from tests.test_gpu_fuzz_preprocessing import (PXSOM_OK, QUANTILE_CLASSES, SEED, _same_numbers, case_count, quantile_cases,
                                                quantile_chunks, quantile_kept)

pytestmark = pytest.mark.gpu

# ---- pxsom_overlay_rgb ----------------------------------------------------------------------------------------------------
RANGE_CLASSES = ("percentile", "negative_lo", "one_ulp", "span_2_31", "clip_below_0", "clip_above_255")
# class j: rgb j % 4 and borders (j // 4) % 4 bytes off a 4-byte boundary, w % 4 = (j + j // 4) % 4 (j < 16 meets every
# pair of rgb offset and w % 4); plane dtype j % 5 with range class (j // 5) % 6 (every pair); label dtype j % 6 (every
# pair with the plane dtype, since 5 and 6 are coprime); the byte j % 3 takes the range class, byte b of the other two
# mode (j + j // 3 + b) % 3; alt present unless j % 3 == 0; inputs (j // 2) % 4 elements off their allocation
OVERLAY_CLASSES = tuple(dict(j=j, rgb_off=j % 4, borders_off=(j // 4) % 4, wmod=(j + j // 4) % 4, plane=PLANE_NP[j % 5],
                             range_cls=RANGE_CLASSES[(j // 5) % 6], seg=SEG_NP[j % 6], byte=j % 3, alt=j % 3 != 0,
                             in_off=(j // 2) % 4) for j in range(30))
_H_ANCHORS, _W_ANCHORS = (1, 3, 4, 5, 15, 16, 17, 33), (1, 5, 254, 255, 256, 257, 258, 510, 511, 512, 513, 514)


def _plane(rs, h, w, npdt, wide=False):
    """A plane without NaN: ovr.signal's mix (zeros, negatives, a heavy tail), or the whole int32 range."""
    if wide:
        return rs.randint(-2 ** 31, 2 ** 31, size=(h, w), dtype=np.int64).astype(np.int32)
    out = ovr.signal(h, w, int(rs.randint(0, 2 ** 31 - 1)), npdt)
    if not (out > 0).any():
        out[rs.randint(h), rs.randint(w)] = 9
    return out


def _range_of(rs, cls, plane):
    """(mode, (lo, hi)) of a range class on a plane; Python floats as the wrapper passes them."""
    if cls == "percentile":
        lo, hi = (float(v) for v in ovr.percentiles_positive(plane))
        return (ovr.OVERLAY_CLIP if lo == hi else ovr.OVERLAY_RESCALE), (lo, hi)
    if cls == "negative_lo":
        return ovr.OVERLAY_RESCALE, (-float(rs.choice([0.5, 3.0, 1000.25])), float(rs.choice([1.0, 40.5, 3000.0])))
    if cls == "one_ulp":                   # two neighbouring binary32 numbers around a value of the plane
        v = np.float32(plane.reshape(-1)[rs.randint(plane.size)]) if plane.dtype == np.float32 else np.float32(rs.choice([0.75, 9.0, 200.0]))
        v = np.float32(1.0) if not np.isfinite(v) or v == 0 else v
        return ovr.OVERLAY_RESCALE, (float(v), float(np.nextafter(v, np.float32(np.inf))))
    if cls == "span_2_31":
        return ovr.OVERLAY_RESCALE, (float(rs.choice([-2.0 ** 31, -2.0 ** 31 + 1, -5.0])), float(rs.choice([2.0 ** 31 - 1, 2.0 ** 31 - 2])))
    v = float(rs.choice([-5.0, -0.25])) if cls == "clip_below_0" else float(rs.choice([255.5, 300.0, 70000.0]))
    return ovr.OVERLAY_CLIP, (v, v)


def overlay_cases(seed, count):
    """Cases of test_fuzz_overlay: class i % 30 of OVERLAY_CLASSES, then shape (h around 4 and 16, w around 256 and 512
    with the class's w % 4), planes, label planes, the modes and ranges of the other two bytes and the guard tails."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        cls = OVERLAY_CLASSES[i % len(OVERLAY_CLASSES)]
        h = int(rs.choice(_H_ANCHORS))
        w = int(rs.choice(_W_ANCHORS))
        w += (cls["wmod"] - w) % 4
        pdt, rcls = cls["plane"], cls["range_cls"]
        planes, modes, ranges = [None] * 3, [ovr.OVERLAY_ZERO] * 3, [(0.0, 0.0)] * 3
        for b in range(3):
            if b == cls["byte"]:
                planes[b] = _plane(rs, h, w, pdt, wide=rcls == "span_2_31" and pdt == np.int32)
                modes[b], ranges[b] = _range_of(rs, rcls, planes[b])
                if rcls == "one_ulp" and pdt == np.float32:          # pixels equal to lo and to hi, the rest outside
                    planes[b][rs.rand(h, w) < 0.3] = np.float32(ranges[b][0])
                    planes[b][rs.rand(h, w) < 0.3] = np.float32(ranges[b][1])
                continue
            mode = (cls["j"] + cls["j"] // 3 + b) % 3
            if mode == ovr.OVERLAY_ZERO:
                continue
            planes[b] = _plane(rs, h, w, pdt)
            if mode == ovr.OVERLAY_RESCALE:
                modes[b], ranges[b] = _range_of(rs, str(rs.choice(["percentile", "negative_lo"])), planes[b])
            else:
                v = float(rs.choice([-5.0, 9.0, 77.5, 300.0]))
                modes[b], ranges[b] = ovr.OVERLAY_CLIP, (v, v)
        seg = ovr.cells(h, w, int(rs.randint(0, 2 ** 31 - 1)), cls["seg"], big=np.dtype(cls["seg"]).itemsize >= 4)
        alt = None
        if cls["alt"]:                      # in a label dtype of another width
            others = [d for d in SEG_NP if np.dtype(d).itemsize != np.dtype(cls["seg"]).itemsize]
            alt = ovr.cells(h, w, int(rs.randint(0, 2 ** 31 - 1)), others[int(rs.randint(len(others)))])
        yield dict(i=i, cls=cls, h=h, w=w, planes=planes, modes=modes, ranges=ranges, seg=seg, alt=alt,
                   rgb_tail=int(rs.randint(0, 9)), borders_tail=int(rs.randint(0, 9)))


def _byte_view(gpu, shape, off, tail):
    """(buffer, view): a uint8 tensor of ``shape`` ``off`` bytes into a sentinel buffer whose base is 4-byte aligned."""
    n = int(np.prod(shape))
    buf, view = _view1d(gpu, np.full(n, _sentinel(np.uint8)), off, tail, _sentinel(np.uint8))
    assert buf.data_ptr() % 4 == 0 and view.data_ptr() % 4 == off % 4
    return buf, view.view(shape)


def test_fuzz_overlay(gpu):
    """overlay_compose with explicit modes and ranges against ovr.compose, array_equal; rgb and borders 0 ... 3 bytes into
    uint8 sentinel buffers (the 12-byte packed store of a lane must not reach past the right edge or the last row); the
    borders-only and the rgb-only launch give the same bytes."""
    import torch
    from ark_analysis_amd import som_device as sd
    fill = _sentinel(np.uint8)
    for case in overlay_cases(SEED + 70, case_count(OVERLAY_CLASSES)):
        cls, h, w = case["cls"], case["h"], case["w"]
        tag = "case %d: class=%s %dx%d modes=%s ranges=%s alt=%s (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], {k: (np.dtype(v).name if k in ("plane", "seg") else v) for k, v in cls.items()}, h, w, case["modes"],
            case["ranges"], None if case["alt"] is None else case["alt"].dtype, SEED)
        put = lambda a: None if a is None else _view1d(gpu, a, cls["in_off"], 2, _sentinel(a.dtype))[1]   # noqa: E731
        planes = [put(p) for p in case["planes"]]
        seg, alt = put(case["seg"]), put(case["alt"])
        want = ovr.compose(case["planes"], case["modes"], case["ranges"], case["seg"], case["alt"])
        want_borders = ovr.borders(case["seg"])
        for want_rgb, want_b in ((True, True), (True, False), (False, True)):
            rbuf, rgb = _byte_view(gpu, (h, w, 3), cls["rgb_off"], case["rgb_tail"])
            bbuf, borders = _byte_view(gpu, (h, w), cls["borders_off"], case["borders_tail"])
            got = sd.overlay_compose(planes, case["modes"], case["ranges"], seg, alt, want_rgb=want_rgb, want_borders=want_b,
                                     rgb=rgb if want_rgb else None, borders=borders if want_b else None)
            torch.cuda.synchronize()
            t = tag + " rgb=%s borders=%s" % (want_rgb, want_b)
            if want_rgb:
                assert got[0].data_ptr() == rgb.data_ptr(), t
                bad = np.argwhere(rgb.cpu().numpy() != want)
                assert bad.size == 0, t + ": %d bytes differ, first at %s" % (len(bad), bad[0])
            if want_b:
                assert got[1].data_ptr() == borders.data_ptr(), t
                assert np.array_equal(borders.cpu().numpy(), want_borders), t + ": borders"
            assert _guard_intact(rbuf.cpu().numpy(), slice(cls["rgb_off"], cls["rgb_off"] + (h * w * 3 if want_rgb else 0)),
                                 fill), t + ": rgb guard"
            assert _guard_intact(bbuf.cpu().numpy(), slice(cls["borders_off"], cls["borders_off"] + (h * w if want_b else 0)),
                                 fill), t + ": borders guard"


# ---- pxsom_colorize -------------------------------------------------------------------------------------------------------
COLORIZE_MASK_NP = (np.uint8, np.int16, np.uint16, np.int32)
COLORIZE_TABLE_ROWS = (1, 2, 255, 256, 70000)
# class j < 16: the mask j % 4 elements and out j // 4 bytes off their 4-element / 4-byte alignment -- the 16 offset
# pairs, hence all four vec_in x vec_out pairs; classes 16 ... 19 hold an index outside the table, the mask at every
# offset.  n_px % 4 = (j + j // 4) % 4, so every output offset meets every ragged last group; the mask dtype, the 3 or 4
# columns and the table size cycle with other periods (70 000 rows fall on uint8, uint16, int32 and int16 masks)
COLORIZE_CLASSES = tuple(dict(j=j, mask_off=j % 4, out_off=(j // 4) % 4, pxmod=(j + j // 4) % 4,
                              mask=COLORIZE_MASK_NP[(j + j // 8) % 4], ncol=3 + ((j + j // 4) // 2) % 2,
                              rows=COLORIZE_TABLE_ROWS[j % 5], bad=j >= 16) for j in range(20))


def colorize_route(mask_off, out_off):
    """(vec_in, vec_out) of colorize_typed: the mask base on 4 elements, the output base on 4 bytes."""
    return mask_off % 4 == 0, out_off % 4 == 0


def colorize_cases(seed, count):
    """Cases of test_fuzz_colorize: class i % 20 of COLORIZE_CLASSES; the last four classes hold an index outside the
    table (negative where the dtype is signed, else past the end) among valid ones."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        cls = COLORIZE_CLASSES[i % len(COLORIZE_CLASSES)]
        mdt = np.dtype(cls["mask"])
        n_rows, top = cls["rows"], int(np.iinfo(mdt).max)
        if cls["bad"] and mdt.kind == "u" and n_rows > top:          # an unsigned mask needs an index past the end
            n_rows = 255 if mdt.itemsize == 1 else 256
        live = min(n_rows, top + 1)                                  # the rows the mask's dtype can name
        h = int(rs.choice([1, 3, 7, 41]))                            # odd, so that w alone sets n_px % 4
        w = int(rs.randint(1, 300))
        w += next(k for k in range(4) if (h * (w + k)) % 4 == cls["pxmod"])
        mask = rs.randint(0, live, size=(h, w)).astype(mdt)
        mask[rs.randint(h), rs.randint(w)] = live - 1
        bad_at = None
        if cls["bad"]:
            bad_at = [(int(rs.randint(h)), int(rs.randint(w))) for _ in range(int(rs.randint(1, 4)))]
            bad_at[0] = (h - 1, w - 1) if rs.rand() < 0.5 else bad_at[0]          # in the ragged last group
            for y, x in bad_at:
                negative = mdt.kind == "i" and (n_rows > top or rs.rand() < 0.5)
                mask[y, x] = -1 - int(rs.randint(0, 100)) if negative else min(n_rows + int(rs.randint(0, 2)), top)
        table = rs.randint(0, 256, size=(n_rows, cls["ncol"])).astype(np.uint8)
        table[rs.randint(n_rows)] = 0
        yield dict(i=i, cls=cls, mask=mask, table=table, bad_at=bad_at, route=colorize_route(cls["mask_off"], cls["out_off"]),
                   out_tail=int(rs.randint(0, 9)), status_off=int(rs.randint(0, 4)))


def test_fuzz_colorize(gpu):
    """pxsom_colorize against table[mask]; mask and out each aligned or 1 ... 3 elements / bytes off, out and the status
    word inside sentinel buffers; an index outside the table sets the status and leaves a zero pixel, nothing else."""
    import torch
    from ark_analysis_amd import _capi, som_device as sd
    lib = _capi.lib()
    fill, fi = _sentinel(np.uint8), _sentinel(np.int32)
    for case in colorize_cases(SEED + 71, case_count(COLORIZE_CLASSES)):
        cls, mask, table = case["cls"], case["mask"], case["table"]
        h, w = mask.shape
        ncol = table.shape[1]
        tag = "case %d: class=%s %dx%d table %d x %d route vec_in=%s vec_out=%s (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], {k: (np.dtype(v).name if k == "mask" else v) for k, v in cls.items()}, h, w, table.shape[0], ncol,
            case["route"][0], case["route"][1], SEED)
        mbuf, mt = _view1d(gpu, mask, cls["mask_off"], 2, _sentinel(mask.dtype))
        assert mbuf.data_ptr() % 16 == 0
        assert (mt.data_ptr() % (4 * mask.dtype.itemsize) == 0) == case["route"][0], tag
        tt = torch.from_numpy(table).to(gpu)
        obuf, out = _byte_view(gpu, (h, w, ncol), cls["out_off"], case["out_tail"])
        assert (out.data_ptr() % 4 == 0) == case["route"][1], tag
        sbuf, status = _view1d(gpu, np.full(1, fi), case["status_off"], 3, fi)
        rc = lib.pxsom_colorize(mt.data_ptr(), sd.overlays.COLORIZE_MASK_DTYPES[mt.dtype], h, w, tt.data_ptr(), table.shape[0], ncol,
                                out.data_ptr(), status.data_ptr(), _capi.stream_ptr())
        torch.cuda.synchronize()
        assert rc == PXSOM_OK, tag
        idx = mask.astype(np.int64)
        ok = (idx >= 0) & (idx < table.shape[0])
        want = np.where(ok[:, :, None], table[np.where(ok, idx, 0)], 0).astype(np.uint8)
        assert bool((~ok).any()) == cls["bad"], tag
        got = out.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, tag + ": %d bytes differ, first at %s" % (len(bad), bad[0])
        assert int(status.cpu()[0]) == (sd.COLORIZE_BAD_INDEX if cls["bad"] else 0), tag
        assert _guard_intact(obuf.cpu().numpy(), slice(cls["out_off"], cls["out_off"] + h * w * ncol), fill), tag + ": out guard"
        assert _guard_intact(sbuf.cpu().numpy(), slice(case["status_off"], case["status_off"] + 1), fi), tag + ": status guard"
        # the same call as the wrapper makes it, into a second guarded output
        obuf2, out2 = _byte_view(gpu, (h, w, ncol), cls["out_off"], case["out_tail"])
        got2, status2 = sd.colorize(mt, tt, out=out2)
        assert got2.data_ptr() == out2.data_ptr() and status2 == (sd.COLORIZE_BAD_INDEX if cls["bad"] else 0), tag
        assert np.array_equal(out2.cpu().numpy(), want), tag + ": through som_device.colorize"
        assert _guard_intact(obuf2.cpu().numpy(), slice(cls["out_off"], cls["out_off"] + h * w * ncol), fill), tag + ": out guard (wrapper)"


# ---- pxsom_percentile_f32_listq ---------------------------------------------------------------------------------------------
LISTQ_VALUE_CLASSES = ("two_values", "all_equal", "dup_straddle", "low_byte", "mixed_sign", "subnormals")
LISTQ_CLASSES = ("c1", "c47", "c48", "c49", "c97", "ldx_view", "nq1", "nq2", "nq3", "nq4", "q_integral", "mode0", "mode1",
                 "mode2", "m0", "m1", "m2") + LISTQ_VALUE_CLASSES
LISTQ_Q = (0.0, 5.0, 37.5, 50.0, 95.0, 100.0)


def listq_value_pool(seed):
    """The float32 matrices of the six value classes, drawn by quantile_cases itself (one run over its classes with a
    seed of this family; the existing family's cases are not touched) -> {class: (x [n, c0], q, keep_mode)}."""
    want = {QUANTILE_CLASSES.index(v + "_f32"): v for v in LISTQ_VALUE_CLASSES}
    pool = {}
    for case in quantile_cases(seed, max(want) + 1):
        if case["i"] in want:
            assert case["x"].dtype == np.float32
            pool[want[case["i"]]] = (case["x"], case["q"], case["keep_mode"])
    return pool


def listq_reference(x, q_percent, keep_mode):
    """np.percentile(kept, [q...]) of every float32 column, NaN for a column without a kept value -> [n_q, c] float64."""
    out = np.full((len(q_percent), x.shape[1]), np.nan)
    with np.errstate(all="ignore"):
        for j in range(x.shape[1]):
            kept = quantile_kept(np.ascontiguousarray(x[:, j]), keep_mode)
            if kept.size:
                out[:, j] = np.percentile(kept, list(q_percent))
    return out


def listq_cases(seed, count):
    """Cases of test_fuzz_listq: class i % 23 of LISTQ_CLASSES -- c on the 48-column sweeps, a strided view at a column
    offset, 1 ... 4 quantiles (one list with q (m - 1) integral), the keep modes, columns with 0, 1 and 2 kept values, the
    six value classes (their columns are row permutations of the pool's, which keeps what each class is named for)."""
    rs = np.random.RandomState(seed)
    pool = listq_value_pool(seed + 1)
    r_cls = len(LISTQ_CLASSES)
    for i in range(count):
        cls = LISTQ_CLASSES[i % r_cls]
        c, n = int(rs.randint(2, 7)), int(rs.randint(3, 400))
        mode = int(rs.randint(0, 3))
        n_q = int(rs.randint(1, 5))
        off, pad = int(rs.choice([0, 0, 1, 3])), int(rs.choice([0, 0, 2, 5]))
        if cls[0] == "c" and cls[1:].isdigit():
            c = int(cls[1:])
        elif cls == "ldx_view":
            off, pad = int(rs.randint(1, 6)), int(rs.randint(1, 8))
        elif cls[:2] == "nq":
            n_q = int(cls[2])
        elif cls in ("mode0", "mode1", "mode2"):
            mode = int(cls[4])
        q = [float(v) for v in rs.choice(LISTQ_Q, size=n_q)]
        if cls in LISTQ_VALUE_CLASSES:
            base, q0, mode = pool[cls]
            n, c = base.shape[0], int(rs.choice([1, 3, 49]))
            x = np.stack([base[rs.permutation(n), j % base.shape[1]] for j in range(c)], axis=1)
            q[0] = 100.0 * q0                             # the q that class was drawn for (dup_straddle)
            if cls == "all_equal":
                mode = 2                                  # (a negative constant has no kept value under mode 1)
        else:
            x = (rs.standard_normal(size=(n, c)) * 10.0 ** float(rs.uniform(-3, 3))).astype(np.float32)
            x[rs.rand(n, c) < 0.3] = 0.0
            if cls == "q_integral":                       # 64 or 128 intervals, q a multiple of 1 / 64
                n, mode = int(rs.choice([65, 129])), 2
                x = (rs.standard_normal(size=(n, c)) * 5).astype(np.float32)
                q[0] = float(rs.choice([25.0, 50.0, 75.0, 1.5625]))
            else:
                x[rs.rand(n, c) < 0.02] = np.nan
        if cls in ("m0", "m1", "m2"):                     # column 0: exactly m kept values among values the mode drops
            n = max(n, 5)
            x = np.resize(x, (n, c)).copy()
            drop = {0: [0.0, -0.0, np.nan], 1: [0.0, -0.0, np.nan, -1.5, -np.inf], 2: [np.nan]}[mode]
            x[:, 0] = rs.choice(drop, size=n)
            m = int(cls[1])
            x[rs.choice(n, m, replace=False), 0] = (rs.uniform(0.5, 9.0, size=m) * (1 if mode == 1 else rs.choice([-1, 1], size=m)))
        yield dict(i=i, cls=cls, x=np.ascontiguousarray(x, dtype=np.float32), q=q, keep_mode=mode, off=off, pad=pad,
                   chunks=quantile_chunks(c), out_off=int(rs.randint(0, 4)), ws_off=int(rs.randint(0, 4)))


def test_fuzz_listq(gpu):
    """pxsom_percentile_f32_listq against np.percentile(kept, [q...]) on the float32 column: equal as numbers, NaN for a
    column without a kept value; the matrix a strided view at a column offset (ldx > c), out [n_q, c] and the workspace
    inside sentinel buffers."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fo, fw = _sentinel(np.float64), _sentinel(np.int64)
    for case in listq_cases(SEED + 72, case_count(LISTQ_CLASSES)):
        x, q = case["x"], case["q"]
        n, c = x.shape
        n_q = len(q)
        tag = "case %d: class=%s n=%d c=%d q=%r keep_mode=%d off=%d pad=%d chunks=%s (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], case["cls"], n, c, q, case["keep_mode"], case["off"], case["pad"], case["chunks"], SEED)
        buf, xt = _view2d(gpu, x, case["off"], case["pad"], fill=_sentinel(np.float32))
        ldx = case["off"] + c + case["pad"]
        obuf, out = _view1d(gpu, np.full((n_q, c), fo), case["out_off"], 3, fo)
        wsb = lib.pxsom_quantile_workspace_bytes(n, c)
        assert wsb > 0 and wsb % 8 == 0, tag
        wbuf, ws = _view1d(gpu, np.full(wsb // 8, fw), case["ws_off"], 3, fw)
        qs = np.ascontiguousarray([v / 100 for v in q], dtype=np.float64)          # as som_device.percentiles_positive
        rc = lib.pxsom_percentile_f32_listq(xt.data_ptr(), n, c, ldx, qs.ctypes.data, n_q, int(case["keep_mode"]),
                                            out.data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr())
        torch.cuda.synchronize()
        assert rc == PXSOM_OK, tag
        got, want = out.cpu().numpy(), listq_reference(x, q, case["keep_mode"])
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        assert _same_numbers(got, want), tag + ": [q, column] %s: got %r, numpy %r" % (
            bad[:5].tolist(), got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])
        assert _guard_intact(obuf.cpu().numpy(), slice(case["out_off"], case["out_off"] + n_q * c), fo), tag + ": output guard"
        assert _guard_intact(wbuf.cpu().numpy(), slice(case["ws_off"], case["ws_off"] + wsb // 8), fw), tag + ": workspace guard"
