"""Randomised parity sweep of K24 pxsom_neighborhood_sums against the numpy statement of tests/splda_reference.py, bit for
bit, by route class: case i takes class i % 40 of NS_CLASSES -- a layout and coordinate scale of
tests/test_gpu_fuzz_cell_distances.py (uniform with duplicates, lattice, clumps, rational, tiny_fovs, one_big; 1e-3 ... 1e6),
a radius class (0, below every distance, about ten neighbours, every cell of the FOV, exactly a distance that occurs) and a
feature-count class (0 with null feats / sums, 1, 7, 8, 9, 16, 17, 65 ... 200); 5 and 8 are coprime, so 40 cases meet
every radius class with every feature-count class, and the exact-distance radius meets the lattice twice.  FOV sizes
include 0, 1, 255 ... 257 and sizes whose last tile of 256 candidates is no multiple of the 32 of a round of pair tests.
Features are signed values over 10^-8 ... 10^8, so a sum in any order but ascending rows differs in its bits, with +-0.0, NaN
and +-inf sprinkled in.  Every radius runs under "lt" and "le".  feats and sums sit at drawn 8-byte offsets, xy stays
16-byte aligned, sums and counts lie inside sentinel buffers.  The entry is called as som_device.neighborhood_sums calls it,
through _capi, since the wrapper allocates its outputs.  ``PXSOM_FUZZ_CASES`` / ``PXSOM_FUZZ_SEED`` as in
test_gpu_fuzz_preprocessing.py.  The generator is device-free (tests/test_fuzz_generators.py checks it on CPU)."""
import numpy as np
import pytest

from tests import splda_reference as sr
from tests.test_gpu_fuzz_cell_distances import CLASSES as LAYOUT_CLASSES
from tests.test_gpu_fuzz_images import _guard_intact, _sentinel, _view1d
from tests.test_gpu_fuzz_preprocessing import PXSOM_OK, SEED, _same_bits, case_count

RADIUS_CLASSES = ("zero", "below_all", "ten", "all", "exact")
FEAT_CLASSES = (0, 1, 7, 8, 9, 16, 17, "wide")
NS_CLASSES = tuple((LAYOUT_CLASSES[j % len(LAYOUT_CLASSES)][2], LAYOUT_CLASSES[j % len(LAYOUT_CLASSES)][1],
                    RADIUS_CLASSES[j % 5], FEAT_CLASSES[j % 8]) for j in range(40))
kBlock, kGroup = 256, 32               # pxsom_neighborhood_sums.hip: candidates per staged tile, per round of pair tests
LATTICE_HYPOTENUSES = ((0, 1, 1), (3, 4, 5), (5, 12, 13), (8, 15, 17))
_FOV_SIZES = (0, 1, 2, 31, 33, 255, 256, 257, 300, 556)       # 300 and 556: a last tile of 44 candidates


def lattice_scale(scale):
    """The lattice's scale: the class's, but 2^-10 for 1e-3, which is no binary64 number -- lattice coordinates times the
    scale must be exact, so that a radius of hypotenuse x step x scale is exactly the distance of the cells it names."""
    return 2.0 ** -10 if scale < 1 else scale


def _exact_product(ints, scale):
    """ints * scale in binary64, asserted exact."""
    ints = np.asarray(ints, dtype=np.int64)
    out = ints.astype(np.float64) * scale
    if scale >= 1:
        assert float(scale) == int(scale) and np.all(np.abs(ints) * int(scale) < 2 ** 53)
        assert np.array_equal(out, (ints * int(scale)).astype(np.float64))
    else:
        assert np.array_equal(out / scale, ints.astype(np.float64)) and np.log2(scale) == int(np.log2(scale))
    return out


def _features(rs, n, p):
    f = rs.choice([-1.0, 1.0], size=(n, p)) * 10.0 ** rs.uniform(-8, 8, size=(n, p))
    f[rs.rand(n, p) < 0.05] = 0.0
    f[rs.rand(n, p) < 0.05] = -0.0
    if n:
        for v in (np.nan, np.inf, -np.inf, np.inf):
            f[rs.randint(0, n), rs.randint(0, p)] = v
    return f


def neighborhood_sums_cases(seed, count):
    """Cases of test_fuzz_neighborhood_sums -> dict(xy, feats or None, seg, radius, step, ...)."""
    for i in range(count):
        rs = np.random.RandomState((seed + 7919 * i) % (2 ** 32))
        layout, scale, rcls, fcls = cls = NS_CLASSES[i % len(NS_CLASSES)]
        if layout == "lattice":
            scale = lattice_scale(scale)
        if layout == "tiny_fovs":
            sizes = rs.randint(0, 9, size=rs.randint(100, 300)).tolist()
        elif layout == "one_big":
            sizes = [int(rs.randint(700, 1100))]
        else:
            sizes = [int(rs.choice(_FOV_SIZES + (int(rs.randint(3, 500)),))) for _ in range(rs.randint(1, 5))]
            sizes[0] = int(_FOV_SIZES[i % len(_FOV_SIZES)])         # every edge size within one run of the classes
        if rcls == "exact" and max(sizes) < 40:
            sizes.append(int(rs.choice([257, 300])))
        step = int(rs.choice([1, 3, 10]))
        xy = []
        for m in sizes:
            side = max(30.0 * np.sqrt(m), 8.0)
            if layout == "lattice":
                cols = max(int(np.ceil(np.sqrt(max(m, 1)))), 1)
                idx = rs.permutation(cols * cols)[:m]
                pts = _exact_product(np.stack([idx // cols, idx % cols], 1) * step, scale)
            elif layout == "clumps":
                centres = rs.uniform(0, side, (max(m // 8, 1), 2))
                pts = centres[rs.randint(0, len(centres), m)] * scale
            elif layout == "rational":
                pts = rs.randint(0, int(side * 40) + 1, (m, 2)) / rs.randint(20, 80, (m, 1)) * scale
            else:
                pts = rs.uniform(0, side, (m, 2))
                if m >= 2 and rs.randint(2):
                    dup = rs.randint(0, m, size=max(1, m // 20))
                    pts[dup] = pts[rs.randint(0, m, size=dup.size)]
                pts = pts * scale
            xy.append(np.asarray(pts, dtype=np.float64).reshape(m, 2))
        n = int(sum(sizes))
        xy = np.ascontiguousarray(np.concatenate(xy).reshape(n, 2))
        seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        big = int(np.argmax(sizes))
        a, b = int(seg[big]), int(seg[big + 1])
        if rcls == "zero":
            radius = 0.0
        elif rcls == "below_all":
            radius = 1e-7 * scale
        elif rcls == "ten":
            radius = 1.8 * step * scale if layout == "lattice" else 53.5 * scale
        elif rcls == "all":
            radius = 3.0 * float(np.abs(xy).max() if n else 1.0) + 1.0
        elif layout == "lattice":
            h = LATTICE_HYPOTENUSES[int(rs.randint(0, len(LATTICE_HYPOTENUSES)))]
            radius = float(_exact_product([h[2] * step], scale)[0])
        else:                              # the distance of two cells of the largest FOV, as the statement forms it
            p, q = xy[a + int(rs.randint(0, b - a))], xy[a + int(rs.randint(0, b - a))]
            dx, dy = q[0] - p[0], q[1] - p[1]
            radius = float(np.sqrt(dx * dx + dy * dy))
        n_feat = int(rs.randint(65, 201)) if fcls == "wide" else int(fcls)
        yield dict(i=i, cls=cls, xy=xy, seg=seg, radius=radius, step=step, scale=scale, sizes=sizes, big=(a, b),
                   feats=_features(rs, n, n_feat) if n_feat else None, n_feat=n_feat,
                   feat_off=int(rs.randint(0, 4)), sums_off=int(rs.randint(0, 4)), counts_off=int(rs.randint(0, 4)))


NS_CASES = case_count(NS_CLASSES)


@pytest.mark.gpu
def test_fuzz_neighborhood_sums(gpu):
    """Counts equal and sums bit-equal (NaN by position) to splda_reference.neighborhood_sums under "lt" and "le"; sums and
    counts inside sentinel buffers, of which nothing outside the [n, p] and [n] slices may change."""
    import torch
    from ark_analysis_amd import _capi, som_device
    lib = _capi.lib()
    fs, fc = _sentinel(np.float64), _sentinel(np.int32)
    for case in neighborhood_sums_cases(SEED + 60, NS_CASES):
        xy, feats, seg, p = case["xy"], case["feats"], case["seg"], case["n_feat"]
        n = len(xy)
        xy_t, seg_t = torch.from_numpy(xy).to(gpu), torch.from_numpy(seg).to(gpu)
        assert xy_t.data_ptr() % 16 == 0
        ft = _view1d(gpu, feats, case["feat_off"], 3, fs)[1] if p else None
        for closed in (False, True):
            tag = "case %d: class=%s n=%d FOVs=%s n_feat=%d radius=%r %s offsets=%d/%d/%d (PXSOM_FUZZ_SEED=%d)" % (
                case["i"], case["cls"], n, case["sizes"][:8], p, case["radius"], "le" if closed else "lt", case["feat_off"],
                case["sums_off"], case["counts_off"], SEED)
            sbuf, sums = _view1d(gpu, np.full((n, p), fs), case["sums_off"], 5, fs)
            cbuf, counts = _view1d(gpu, np.full(n, fc), case["counts_off"], 5, fc)
            rc = lib.pxsom_neighborhood_sums(xy_t.data_ptr(), ft.data_ptr() if p else None, seg_t.data_ptr(), len(seg) - 1, n,
                                             p, som_device.radius_threshold(case["radius"], closed),
                                             sums.data_ptr() if p else None, counts.data_ptr(), _capi.stream_ptr())
            torch.cuda.synchronize()
            assert rc == PXSOM_OK, tag
            want_sums, want_counts = sr.neighborhood_sums(xy, feats, seg, case["radius"], closed)
            got_counts, got_sums = counts.cpu().numpy(), sums.cpu().numpy()
            bad = np.flatnonzero(got_counts != want_counts)
            assert bad.size == 0, tag + ": counts of rows %s: %s, statement %s" % (bad[:5], got_counts[bad[:5]],
                                                                                 want_counts[bad[:5]])
            assert _same_bits(got_sums, want_sums), tag + ": %d of %d sums differ in their bits" % (
                int((~((got_sums.view(np.int64) == want_sums.view(np.int64)) | (np.isnan(got_sums) & np.isnan(want_sums)))).sum()),
                got_sums.size)
            assert _guard_intact(sbuf.cpu().numpy(), slice(case["sums_off"], case["sums_off"] + n * p), fs), tag + ": sums guard"
            assert _guard_intact(cbuf.cpu().numpy(), slice(case["counts_off"], case["counts_off"] + n), fc), tag + ": counts guard"
