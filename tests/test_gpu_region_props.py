"""pxsom_region_shape and pxsom_region_hull on the GPU against tests/region_props_reference.py: the raw
integers equal, the float columns the host derives from them within the derived tolerances (region_props_reference
.compare), and generate_cell_table with the property lists named against the same call through the host stand-in."""
import numpy as np
import pandas as pd
import pytest
import torch

from ark_analysis_amd.segmentation import regionprops_extraction as rpe
from tests import cell_table_reference as ctr
from tests import region_props_reference as rpr
from tests.test_cell_table import write_cohort

pytestmark = pytest.mark.gpu


def device_raw(gpu, seg, off=0, pad=0, expect_left_out=None, **kwargs):
    """som_device.region_props of a host label image (placed in a wider buffer: row stride off + w + pad) as host
    arrays, the cells the device leaves out -- exactly those with a box past 64 x 64 -- filled by the host route."""
    from ark_analysis_amd import som_device
    h, w = seg.shape
    buf = np.zeros((h, off + w + pad), dtype=seg.dtype)
    buf[:, off:off + w] = seg
    view = torch.from_numpy(buf).to(gpu)[:, off:off + w]
    got = som_device.region_props(view, **kwargs)
    torch.cuda.synchronize()
    raw = {k: v.cpu().numpy() for k, v in got.items()}
    box = raw["bbox"].astype(np.int64)
    big = ((box[:, 1] - box[:, 0] + 1 > 64) | (box[:, 3] - box[:, 2] + 1 > 64)) & (raw["count"] > 0)
    np.testing.assert_array_equal(raw["left_out"], big.astype(np.int32))
    assert not raw["hull"][big].any()
    if expect_left_out is not None:
        assert int(big.sum()) == expect_left_out
    thresholds = {k: v for k, v in kwargs.items() if k in rpe.CONCAVITY_DEFAULTS}
    return rpe.fill_left_out(raw, seg, **thresholds)


def check(gpu, seg, ref=None, **kwargs):
    raw = device_raw(gpu, seg, **kwargs)
    if ref is None:
        ref = rpr.reference(seg)
    rpr.compare(raw, rpe.morphology(raw), ref)
    return raw


# ---- Voronoi images: one tile, tile borders, the full case ------------------------------------------------------------
@pytest.mark.parametrize("h, w, cells, seed", [(64, 64, 20, 1), (200, 200, 30, 2), (1024, 1024, 5000, 3)])
def test_voronoi(gpu, h, w, cells, seed):
    seg, ref = rpr.settled(lambda s: rpr.voronoi(h, w, cells, seed=s), seed)
    check(gpu, seg, ref)


# ---- label images: dtypes, strides, both key-table routes ------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return rpr.settled(lambda s: ctr.fragment(rpr.voronoi(70, 150, 25, seed=s, first_label=3), [5], pieces=4, seed=s), 4)


@pytest.mark.parametrize("segdt", [np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64])
def test_label_dtypes_and_row_stride(gpu, small, segdt):
    seg, ref = small
    check(gpu, seg.astype(segdt), ref, off=3, pad=5)
    check(gpu, seg.astype(segdt), ref, force_search=True)


def test_labels_near_int32_max_take_the_search_route(gpu, small):
    from ark_analysis_amd import _capi
    seg, ref = small
    keys = ref["keys"]
    far = np.linspace(1, 2**31 - 1, keys.size).astype(np.int64)         # ascending, the last one INT32_MAX
    far[1:-1] -= np.arange(keys.size - 2) % 3
    lut = np.zeros(int(keys.max()) + 1, dtype=np.int64)
    lut[keys] = far
    moved = lut[seg].astype(np.int32)
    assert moved.max() == 2**31 - 1
    assert _capi.lib().pxsom_region_shape_workspace_bytes(keys.size, int(far[0]), int(far[-1]), 0) == 0   # no dense LUT
    want = dict(ref, keys=far)
    check(gpu, moved, want)
    check(gpu, moved.astype(np.int64), want, off=1, pad=2)


# ---- cell shapes ------------------------------------------------------------------------------------------------------------
def shapes_image():
    """One image with: a fragmented label, cells touching all four borders, two cells whose hulls overlap each other's
    pixels, boxes of exactly 64 x 64, 65 x 64 and 64 x 65, and a ring and a C whose concavity is larger than 150 px."""
    seg = np.zeros((230, 300), dtype=np.int32)
    seg[0:5, 100:160:2] = 1                   # fragmented, along the top border
    seg[0:230, 0:2] = 2                       # the left border, 230 rows: the host route
    seg[225:230, 10:60] = 3                   # the bottom border
    seg[100:140, 297:300] = 4                 # the right border
    seg[10:74, 10:74] = np.where(rpr.ring(64, 40), 5, 0)          # exactly 64 x 64, a hole of 1600 px
    seg[10:75, 80:144] = 6                    # 65 x 64
    seg[11:74, 85:140] = 0                    # ... hollow, so the host route has a concavity to count
    seg[10:74, 150:215] = 7                   # 64 x 65
    seg[80:100, 10:30] = np.where(rpr.c_shape(20, 14), 8, 0)      # a C: 14 x 17 = 238 px
    seg[83:94, 14:24] = 9                     # a cell inside the C's mouth: inside its hull
    seg[120:160, 20:24] = 10                  # an L ...
    seg[156:160, 20:60] = 10
    seg[122:150, 30:58] = 11                  # ... with a square inside its hull, the L inside the square's not
    seg[170:200, 100:103] = 12                # two bars whose hulls cross
    seg[184:187, 90:130] = 13
    seg[186, 101] = 13
    return seg


def test_cell_shapes(gpu):
    seg = shapes_image()
    ref = rpr.reference(seg)
    by = dict(zip(ref["keys"].tolist(), ref["hull"][:, 3].tolist()))
    assert by[5] == 1 and by[8] == 1 and by[6] == 1
    check(gpu, seg, ref, expect_left_out=3)           # labels 2, 6, 7
    check(gpu, seg, ref, force_search=True, off=2, pad=1)


def test_reuses_the_tables_of_cell_quantify(gpu, small):
    from ark_analysis_amd import som_device
    seg, ref = small
    seg_t = torch.from_numpy(seg).to(gpu)
    q = som_device.cell_quantify(seg_t, torch.zeros(seg.shape + (1,), dtype=torch.uint8, device=gpu))
    got = som_device.region_props(seg_t, keys=q["keys"], count=q["count"], sums=q["sums"], bbox=q["bbox"])
    assert got["count"] is q["count"] and got["bbox"] is q["bbox"]
    raw = {k: v.cpu().numpy() for k, v in got.items()}
    assert raw["left_out"].sum() == 1          # the fragmented label: its box is wider than 64
    rpe.fill_left_out(raw, seg)
    rpr.compare(raw, rpe.morphology(raw), ref)
    with pytest.raises(ValueError, match="go together"):
        som_device.region_props(seg_t, count=q["count"])


@pytest.mark.parametrize("h, w", [(40, 50), (64, 64), (70, 90)])
def test_one_label_fills_the_image(gpu, h, w):
    seg = np.full((h, w), 21, dtype=np.int32)
    raw = check(gpu, seg, expect_left_out=int(h > 64 or w > 64))
    assert raw["hull"][0, 0] == h * w and raw["shape"][0, 3] == 2 * h + 2 * w - 4


def test_empty_segmentation_and_thresholds(gpu):
    raw = device_raw(gpu, np.zeros((33, 70), dtype=np.int32))
    assert all(raw[k].shape[0] == 0 for k in ("keys", "count", "sums", "bbox", "shape", "hull", "left_out"))
    slit = np.zeros((12, 110), dtype=np.int32)      # too wide for the device; the square below is not
    slit[5:8, 4:106] = 9
    slit[6, 5:105] = 0
    box = np.zeros((40, 40), dtype=np.int32)
    box[4:34, 4:34] = np.where(rpr.ring(30, 10), 3, 0)          # a hole of 100 px, p = 36, p^2 / a = 12.96
    for seg in (slit, box):
        for thr in ({}, {"max_compactness": 100}, {"max_compactness": 12}, {"large_concavity_minimum": 99},
                    {"small_concavity_minimum": 101}):
            raw = device_raw(gpu, seg, **thr)
            np.testing.assert_array_equal(raw["hull"], rpr.reference(seg, **thr)["hull"], err_msg=str(thr))


def test_concavity_area_on_a_threshold(gpu):
    """A concavity of exactly small_concavity_minimum (or large_concavity_minimum) pixels does not count: '>' on the
    device, pinned with integer-exact areas (answers by hand, as in tests/test_region_props.py), and p^2 / a = 100 / 10
    exactly on max_compactness pins '<'."""
    from tests.test_region_props import notched
    seg = np.zeros((12, 30), dtype=np.int32)
    seg[2:8, 3:10] = np.where(notched(), 4, 0)
    seg[3:9, 15:22] = np.where(notched(), 6, 0)
    for thr, want in (({}, 0), ({"small_concavity_minimum": 9}, 1),
                      ({"max_compactness": 5, "large_concavity_minimum": 10}, 0),
                      ({"max_compactness": 5, "large_concavity_minimum": 9}, 1),
                      ({"small_concavity_minimum": 9, "max_compactness": 10}, 0),
                      ({"small_concavity_minimum": 9, "max_compactness": 10.5}, 1)):
        raw = device_raw(gpu, seg, expect_left_out=0, **thr)
        assert raw["hull"][:, 3].tolist() == [want, want], thr
        assert raw["hull"][:, 0].tolist() == [42, 42]
        np.testing.assert_array_equal(raw["hull"], rpe.host_raw(seg, **thr)["hull"])


def test_get_single_compartment_props(gpu, small):
    """The entry point without a cell_quantify result to reuse: region_props makes its own key table and statistics."""
    from ark_analysis_amd.segmentation import marker_quantification as mq
    seg, ref = small
    got = mq.get_single_compartment_props(seg, list(rpe.REGIONPROPS_BASE), list(rpe.REGIONPROPS_SINGLE_COMP))
    base, single, _ = rpe.resolve_lists(None, None, [])
    pd.testing.assert_frame_equal(got, rpe.props_frame(rpe.host_raw(seg), base, single), check_exact=True)
    np.testing.assert_array_equal(got["label"], ref["keys"])


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nuclear", [False, True])
def test_generate_cell_table_end_to_end(gpu, tmp_path, monkeypatch, nuclear):
    from ark_analysis_amd.segmentation import marker_quantification as mq
    from tests.test_region_props import _host_region_raw, morph_cohort
    fovs, channels, images, segs = morph_cohort(n_fovs=2, h=90, w=120)
    big = segs["fov0_whole_cell.tiff"].copy()
    big[big == big[45, 60]] = 0
    big[5:75, 5:8] = 77                                # a cell the device leaves to the host route
    segs["fov0_whole_cell.tiff"] = rpr.reference(big, drop=True)[0]
    seg_dir, tiff_dir = write_cohort(str(tmp_path), images, segs, channels)
    args = dict(nuclear_counts=nuclear, regionprops_multi_comp=["nc_ratio"],
                regionprops_kwargs={"small_concavity_minimum": 3})
    got = mq.generate_cell_table(seg_dir, tiff_dir, **args)
    monkeypatch.setattr(mq, "_region_raw", _host_region_raw)
    want = mq.generate_cell_table(seg_dir, tiff_dir, **args)
    assert ("nc_ratio" in got[0].columns) == nuclear and 77 in set(got[0]["label"])
    for a, b in zip(got, want):
        pd.testing.assert_frame_equal(a, b, check_exact=True)     # same integers, same host formulas: the same bits
