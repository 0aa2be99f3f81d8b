"""pxsom_cellquant on the GPU (the per-cell table of generate_cell_table) against the numpy statement of
tests/cell_table_reference.py, and generate_cell_table on the HIP path against the g17 fixtures of the reference and
against the numpy frames."""

import numpy as np
import pytest
import torch

from tests import cell_table_reference as ctr

pytestmark = pytest.mark.gpu

IMG_DTYPES = {"u8": (np.uint8, torch.uint8), "i16": (np.int16, torch.int16), "u16": (np.uint16, torch.uint16),
              "i32": (np.int32, torch.int32), "f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}
SEG_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.uint16): torch.uint16,
              np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.uint32, np.dtype(np.int64): torch.int64}


def _image(rs, h, w, c, npdt):
    if np.dtype(npdt).kind == "f":
        x = rs.gamma(0.6, 3.0, size=(h, w, c)) * (rs.rand(h, w, c) < 0.7)
        return x.astype(npdt)
    hi = min(np.iinfo(npdt).max, 3000)
    return rs.randint(0, hi + 1, size=(h, w, c)).astype(npdt)


def _seg_device(gpu, seg, offset=0, pad=0):
    tdt = SEG_DTYPES[seg.dtype]
    h, w = seg.shape
    if offset or pad:
        wide = torch.zeros((h, w + offset + pad), dtype=tdt, device=gpu)
        wide[:, offset:offset + w] = torch.from_numpy(np.ascontiguousarray(seg)).to(gpu)
        return wide[:, offset:offset + w]
    return torch.from_numpy(np.ascontiguousarray(seg)).to(gpu)


def _run(gpu, seg, img, mode="total_intensity", threshold=0.0, nuc=None, offset=0, pad=0, **kw):
    from ark_analysis_amd import som_device
    got = som_device.cell_quantify(_seg_device(gpu, seg, offset, pad), torch.from_numpy(img).to(gpu), mode=mode,
                                   threshold=threshold, nuc=_seg_device(gpu, nuc) if nuc is not None else None, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def _check(got, want, seg=None, img=None, mode="total_intensity"):
    for k in ("keys", "count", "sums", "bbox"):
        assert np.array_equal(got[k], want[k]), k
    if "nuc" in want:
        assert np.array_equal(got["nuc_keys"], want["nuc_keys"])
        assert np.array_equal(got["nuc"], want["nuc"]), np.flatnonzero(got["nuc"] != want["nuc"])[:10]
    if mode != "center_weighting":
        bad = np.argwhere(got["values"] != want["values"])
        assert bad.size == 0, (bad[:5], got["values"][tuple(bad[0])], want["values"][tuple(bad[0])])
        return
    cells = ctr.cell_coords(seg)
    im = img if img.ndim == 3 else img[:, :, None]
    for i, lab in enumerate(want["keys"]):
        bound = ctr.center_weighting_bound(cells[int(lab)], im)
        assert np.all(np.abs(got["values"][i] - want["values"][i]) <= bound), (lab, got["values"][i], want["values"][i])


@pytest.mark.parametrize("dt", list(IMG_DTYPES))
@pytest.mark.parametrize("c", [1, 2, 22, 40, 100])
def test_total_intensity_every_dtype_and_width(gpu, dt, c):
    rs = np.random.RandomState(c * 7 + len(dt))
    h, w = 96, 200
    seg = ctr.voronoi_labels(h, w, 60, seed=c, dtype=np.int32)
    img = _image(rs, h, w, c, IMG_DTYPES[dt][0])
    _check(_run(gpu, seg, img), ctr.quantify(seg, img))


@pytest.mark.parametrize("mode", ["positive_pixel", "center_weighting"])
@pytest.mark.parametrize("dt", ["u16", "i32", "f32", "f64"])
@pytest.mark.parametrize("c", [1, 3, 22, 130])
def test_other_extractions(gpu, mode, dt, c):
    rs = np.random.RandomState(c + len(mode))
    h, w = 80, 150
    seg = ctr.voronoi_labels(h, w, 40, seed=c + 1, dtype=np.uint16)
    img = _image(rs, h, w, c, IMG_DTYPES[dt][0])
    from ark_analysis_amd.segmentation.marker_quantification import _threshold_for
    for t in ([0, 2.5] if mode == "positive_pixel" else [0]):
        thr = _threshold_for(img.dtype, t)
        _check(_run(gpu, seg, img, mode=mode, threshold=thr), ctr.quantify(seg, img, mode, t), seg, img, mode)


@pytest.mark.parametrize("segdt", [np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64])
def test_label_dtypes_strides_and_both_tables(gpu, segdt):
    rs = np.random.RandomState(3)
    h, w = 70, 133
    seg = ctr.voronoi_labels(h, w, 50, seed=5, dtype=np.int64)
    if np.dtype(segdt).itemsize >= 4:   # a sparse key range (binary search by the K10 rule) next to the compact ones
        seg = np.where(seg > 0, seg * 100000 + 7, 0)
    elif segdt == np.uint16:
        seg = np.where(seg > 0, seg * 1000 + 7, 0)
    seg = seg.astype(segdt)
    img = _image(rs, h, w, 5, np.float32)
    want = ctr.quantify(seg, img)
    for offset, pad in [(0, 0), (3, 5), (1, 64)]:
        for force in (False, True):
            _check(_run(gpu, seg, img, offset=offset, pad=pad, force_search=force), want)


def test_int32_extreme_labels(gpu):
    rs = np.random.RandomState(4)
    seg = np.zeros((64, 90), np.int64)
    seg[:20, :30] = 2 ** 31 - 1
    seg[20:40, :] = 2 ** 31 - 2
    seg[40:, 50:] = 1
    seg[45, 10] = 2 ** 30
    img = _image(rs, 64, 90, 4, np.float32)
    for force in (False, True):
        _check(_run(gpu, seg, img, force_search=force), ctr.quantify(seg, img))
    from ark_analysis_amd import som_device
    bad = torch.from_numpy(np.full((4, 4), 2 ** 31, np.int64)).to(gpu)
    with pytest.raises(NotImplementedError):
        som_device.cell_quantify(bad, torch.zeros((4, 4, 1), device=gpu))


@pytest.mark.parametrize("c", [1, 3])
def test_giant_and_fragmented_labels(gpu, c):
    rs = np.random.RandomState(6)
    h, w = 512, 512
    seg = np.ones((h, w), np.int32)            # one label over the whole image, 262 144 pixels
    seg[100:110, 200:260] = 2
    img = _image(rs, h, w, c, np.float32)
    _check(_run(gpu, seg, img), ctr.quantify(seg, img))
    seg = ctr.fragment(ctr.voronoi_labels(h, w, 800, seed=2), [5, 17, 333], pieces=12)
    _check(_run(gpu, seg, img), ctr.quantify(seg, img))


def test_nuclear_overlap_ties_none_and_overflow(gpu):
    rs = np.random.RandomState(8)
    h, w = 120, 160
    seg = ctr.voronoi_labels(h, w, 30, seed=9, background=0.0)
    nuc = np.zeros_like(seg)
    nuc[::3, ::3] = rs.randint(1, 400, size=nuc[::3, ::3].shape)   # many small nuclei: > 2 per cell
    nuc[:, :8] = 0
    lab = seg[60, 80]
    cell = np.argwhere(seg == lab)
    nuc[seg == lab] = 0
    nuc[tuple(cell[:4].T)] = 900             # a tie: 4 pixels of 900 and 4 of 901, 900 wins
    nuc[tuple(cell[4:8].T)] = 901
    nuc[seg == seg[5, 2]] = 0                # a cell without a nucleus
    img = _image(rs, h, w, 3, np.float32)
    want = ctr.quantify(seg, img, nuc=nuc)
    assert (want["nuc"] == -1).any()
    for cap in (0, 1, 2, 128):
        _check(_run(gpu, seg, img, nuc=nuc, nuc_capacity=cap), want)
    _check(_run(gpu, seg, img, nuc=nuc, nuc_capacity=1, force_search=True), want)


@pytest.mark.parametrize("size,c", [(1024, 22), (2048, 40)])
def test_full_size_voronoi(gpu, size, c):
    rs = np.random.RandomState(size)
    seg = ctr.voronoi_labels(size, size, 20000, seed=size)
    img = _image(rs, size, size, c, np.float32)
    nuc = np.where(seg % 3 == 0, seg, 0)
    got = _run(gpu, seg, img, nuc=nuc)
    want = ctr.quantify(seg, img, nuc=nuc)
    _check(got, want)


def test_empty_segmentation(gpu):
    img = np.ones((8, 8, 2), np.float32)
    got = _run(gpu, np.zeros((8, 8), np.int32), img, nuc=np.zeros((8, 8), np.int32))
    assert got["keys"].size == 0 and got["values"].shape == (0, 2) and got["nuc"].size == 0


# ---- generate_cell_table on the device ----------------------------------------------------------------------------
def test_generate_cell_table_fixtures(gpu, tmp_path):
    from tests.test_cell_table import check_fixture_cases
    check_fixture_cases(tmp_path)


def test_generate_cell_table_against_numpy(gpu, tmp_path):
    from tests.test_cell_table import check_numpy_cases
    check_numpy_cases(tmp_path)


def test_table_feeds_create_c2pc_data_and_train_cell_som(gpu, tmp_path):
    from tests.test_cell_table import check_downstream
    check_downstream(tmp_path)
