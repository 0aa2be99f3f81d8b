"""Seeded fuzz of the K17 kernels -- pxsom_region_shape and pxsom_region_hull, called through the C ABI so that every
output sits in a guarded buffer -- against tests/region_props_reference.py, in the style of tests/test_gpu_fuzz_images.py:
random sizes 1 .. 130 per side, random cell counts, every label dtype, strided views, both key-table routes, labels up to
INT32_MAX, random thresholds.  Every case ends in a comparison: none is skipped.  PXSOM_FUZZ_CASES / PXSOM_FUZZ_SEED
set the number of cases and the seed."""
import numpy as np
import pytest

from ark_analysis_amd.segmentation import regionprops_extraction as rpe
from tests import region_props_reference as rpr
from tests.test_gpu_fuzz_images import CASES, SEED, SEG_NP, _guard_intact, _sentinel, _view1d, _view2d, lut_route

pytestmark = pytest.mark.gpu

ROUTES = ("lut", "search", "sparse")
# area thresholds between the integers where the areas of these small images crowd: no area can sit on one, so the
# reference clears no cell for them (on 2 it would clear every second cell) and areas on both sides of each are common
THRESHOLDS = ({}, {"small_concavity_minimum": 2.5}, {"max_compactness": 14.5}, {"large_concavity_minimum": 25.5},
              {"small_concavity_minimum": 0, "max_compactness": 1e9})


def region_cases(seed, count):
    """``count`` cases, route classes in turn: an image of 1 .. 130 pixels per side holding Voronoi cells, rectangles
    and scattered fragments, its reference (cells with a concavity on a threshold cleared), and how to lay it out."""
    rs = np.random.RandomState(seed)
    cases = []
    for i in range(count):
        route = ROUTES[i % len(ROUTES)]
        npdt = SEG_NP[int(rs.randint(len(SEG_NP)))]
        h, w = int(rs.randint(1, 131)), int(rs.randint(1, 131))
        if rs.rand() < 0.3:                    # around the device route's limit and the tile sizes
            h, w = int(rs.choice([31, 32, 33, 63, 64, 65, 66, 128, 129])), int(rs.choice([63, 64, 65, 66, 127, 128, 130]))
        top = 250 if npdt == np.uint8 else 3000
        n_cells = int(rs.randint(1, max(2, min(top - 5, h * w // 6 + 2))))
        thr = dict(THRESHOLDS[int(rs.randint(len(THRESHOLDS)))])
        seg = rpr.voronoi(h, w, n_cells, seed=int(rs.randint(1 << 30)), background=float(rs.choice([0.0, 0.1, 0.6])))
        for j in range(int(rs.randint(0, 4))):                       # rectangles, hollow ones among them
            r0, c0 = int(rs.randint(h)), int(rs.randint(w))
            r1, c1 = int(rs.randint(r0, h)) + 1, int(rs.randint(c0, w)) + 1
            seg[r0:r1, c0:c1] = n_cells + 1 + j
            if rs.rand() < 0.5 and r1 - r0 > 2 and c1 - c0 > 2:
                seg[r0 + 1:r1 - 1, c0 + 1:c1 - int(rs.randint(0, 2))] = 0
        if rs.rand() < 0.4:                                            # a fragmented label
            pts = rs.rand(h, w) < 0.03
            seg[pts] = n_cells + 5
        seg, ref = rpr.reference(seg.astype(np.int64), drop=True, **thr)
        keys = ref["keys"]
        if route == "sparse" and npdt in (np.int32, np.uint32, np.int64) and keys.size:
            far = np.unique(rs.randint(1, 2**31 - 1, size=4 * keys.size + 8).astype(np.int64))
            far = np.sort(rs.permutation(far)[:keys.size])
            far[-1] = 2**31 - 1
            lut = np.zeros(int(keys.max()) + 1, dtype=np.int64)
            lut[keys] = far
            seg, ref = lut[seg], dict(ref, keys=far)
        keys = ref["keys"]
        force = route == "search" or (route == "sparse" and bool(rs.rand() < 0.3))
        cases.append({"i": i, "route": route, "seg": seg.astype(npdt), "ref": ref, "thr": thr, "force": force,
                      "off": int(rs.randint(0, 5)), "pad": int(rs.randint(0, 7)), "stats": bool(rs.rand() < 0.5),
                      "lut": bool(keys.size) and not force and lut_route(keys.size, keys[0], keys[-1])})
    return cases


def _guarded(gpu, shape, npdt):
    arr = np.zeros(shape, dtype=npdt)
    fill = _sentinel(npdt)
    buf, view = _view1d(gpu, np.full(shape, fill, dtype=npdt), 7, 9, fill)
    return buf, view, slice(7, 7 + arr.size), fill


def test_fuzz_region_props(gpu):
    import torch
    from ark_analysis_amd import _capi, som_device
    lib = _capi.lib()
    compared = 0
    for case in region_cases(SEED + 47, CASES):
        seg, ref, thr = case["seg"], case["ref"], dict(rpe.CONCAVITY_DEFAULTS, **case["thr"])
        h, w = seg.shape
        n = int(ref["keys"].size)
        tag = "case %d: route=%s seg %s %dx%d cells=%d off=%d pad=%d force_search=%s lut=%s stats=%s thresholds=%r " \
              "(PXSOM_FUZZ_SEED=%d)" % (case["i"], case["route"], seg.dtype, h, w, n, case["off"], case["pad"],
                                        case["force"], case["lut"], case["stats"], case["thr"], SEED)
        _, seg_t = _view2d(gpu, seg, case["off"], case["pad"])
        ld = seg_t.stride(0) if h > 1 else w
        keys_t = torch.from_numpy(ref["keys"].astype(np.int32)).to(gpu)
        kmin, kmax = (int(ref["keys"][0]), int(ref["keys"][-1])) if n else (0, 0)
        flags = som_device.REGION_FORCE_SEARCH if case["force"] else 0
        wsb = lib.pxsom_region_shape_workspace_bytes(n, kmin, kmax, flags)
        assert (wsb > 0) == case["lut"], tag
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=gpu)
        bufs = {"shape": _guarded(gpu, (n, 6), np.int64), "hull": _guarded(gpu, (n, 4), np.int64),
                "left_out": _guarded(gpu, (n,), np.int32), "count": _guarded(gpu, (n,), np.int64),
                "sums": _guarded(gpu, (n, 2), np.int64), "bbox": _guarded(gpu, (n, 4), np.int32)}
        ptr = {k: v[1].data_ptr() for k, v in bufs.items()}
        code = som_device.SEG_DTYPES[seg_t.dtype]
        if not case["stats"]:          # the tables come from the caller: K12's, here the reference's
            bufs["count"][1].copy_(torch.from_numpy(ref["count"]).to(gpu))
            bufs["sums"][1].copy_(torch.from_numpy(ref["sums"]).to(gpu))
            bufs["bbox"][1].copy_(torch.from_numpy(ref["bbox"].astype(np.int32)).to(gpu))
        rc = lib.pxsom_region_shape(seg_t.data_ptr(), code, ld, h, w, keys_t.data_ptr() if n else None, n, kmin, kmax,
                                    ptr["shape"], ptr["count"] if case["stats"] else None,
                                    ptr["sums"] if case["stats"] else None, ptr["bbox"] if case["stats"] else None,
                                    ws.data_ptr(), wsb, flags, _capi.stream_ptr())
        _capi.check(rc, "pxsom_region_shape " + tag)
        rc = lib.pxsom_region_hull(seg_t.data_ptr(), code, ld, h, w, keys_t.data_ptr() if n else None, n, ptr["count"],
                                   ptr["bbox"], float(thr["small_concavity_minimum"]), float(thr["max_compactness"]),
                                   float(thr["large_concavity_minimum"]), ptr["hull"], ptr["left_out"],
                                   _capi.stream_ptr())
        _capi.check(rc, "pxsom_region_hull " + tag)
        torch.cuda.synchronize()
        for name, (buf, _, region, fill) in bufs.items():
            assert _guard_intact(buf.cpu().numpy(), region, fill), tag + ": stores outside " + name
        raw = {k: v[1].cpu().numpy() for k, v in bufs.items()}
        raw["keys"] = ref["keys"]
        box = ref["bbox"]
        big = (box[:, 1] - box[:, 0] + 1 > 64) | (box[:, 3] - box[:, 2] + 1 > 64)
        try:
            np.testing.assert_array_equal(raw["left_out"], big.astype(np.int32))
            assert not raw["hull"][big].any()
            rpe.fill_left_out(raw, seg, **thr)
            rpr.compare(raw, rpe.morphology(raw), ref)
        except AssertionError as e:
            raise AssertionError(tag + ": " + str(e)) from e
        compared += 1
    assert compared == CASES          # the share of skipped cases is 0
