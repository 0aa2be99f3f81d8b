"""pxsom_nuclear_overlaps, pxsom_split_apply and the chain som_device.split_large_nuclei on the GPU against the numpy
statements of tests/split_nuclei_reference.py (checked against the reference's own outputs in test_split_nuclei.py):
every table entry and every pixel compared exactly."""
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from tests import split_nuclei_reference as snr
from tests import test_split_nuclei as cpu

pytestmark = pytest.mark.gpu

SENTINEL = 0x5B


def strided(gpu, plane, layout, fill=SENTINEL):
    """The plane on the device as a view: contiguous, at an offset inside a wider buffer, or with padded rows."""
    h, w = plane.shape
    if layout == "contiguous":
        return torch.from_numpy(np.ascontiguousarray(plane)).to(gpu)
    top, left, right = (2, 3, 5) if layout == "offset" else (0, 0, 9)
    padded = np.full((h + 2 * top, w + left + right), fill, dtype=plane.dtype)
    padded[top:top + h, left:left + w] = plane
    return torch.from_numpy(padded).to(gpu)[top:top + h, left:left + w]


def sentinel_out(gpu, h, w, dtype, layout):
    """(buffer, view): an output plane inside a buffer of sentinels."""
    top, left, right = {"contiguous": (1, 0, 0), "offset": (2, 3, 5), "padded": (1, 0, 9)}[layout]
    buf = torch.from_numpy(np.full((h + 2 * top, w + left + right), SENTINEL, dtype=dtype)).to(gpu)
    return buf, buf[top:top + h, left:left + w]


def around_untouched(buf, view_shape, layout):
    h, w = view_shape
    top, left, right = {"contiguous": (1, 0, 0), "offset": (2, 3, 5), "padded": (1, 0, 9)}[layout]
    host = buf.cpu().numpy().copy()
    host[top:top + h, left:left + w] = SENTINEL
    return bool((host == SENTINEL).all())


def check_tables(gpu, cell, nuc, layout="padded", force_search=False):
    """nuclear_overlaps against pair_tables, every entry."""
    from ark_analysis_amd import som_device
    keys, nuc_keys, best, inside, area = som_device.nuclear_overlaps(strided(gpu, cell, layout), strided(gpu, nuc, layout, 0x5C),
                                                                     force_search=force_search)
    ck, nk, wbest, winside, warea = snr.pair_tables(cell, nuc)
    assert keys.dtype == nuc_keys.dtype == best.dtype == inside.dtype == torch.int32 and area.dtype == torch.int64
    np.testing.assert_array_equal(keys.cpu().numpy(), ck)
    np.testing.assert_array_equal(nuc_keys.cpu().numpy(), nk)
    np.testing.assert_array_equal(best.cpu().numpy(), wbest)
    np.testing.assert_array_equal(inside.cpu().numpy(), winside)
    np.testing.assert_array_equal(area.cpu().numpy(), warea)


def check_chain(gpu, cell, nuc, ids, min_size=15, layout="padded", force_search=False, want=None):
    """split_large_nuclei on strided views into an output between sentinels, against the vectorised statement."""
    from ark_analysis_amd import som_device
    if want is None:
        want = snr.split_vec(cell, nuc, ids, min_size)[0]
    buf, out = sentinel_out(gpu, cell.shape[0], cell.shape[1], nuc.dtype, layout)
    got = som_device.split_large_nuclei(strided(gpu, cell, layout), strided(gpu, nuc, layout, 0x5C), ids, min_size=min_size,
                                        out=out, force_search=force_search)
    assert got.data_ptr() == out.data_ptr() and got.dtype == out.dtype
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert around_untouched(buf, cell.shape, layout)
    return got


# ---- the hand-built plane -----------------------------------------------------------------------------------------
def test_hand_plane_every_decision_on_its_edge(gpu):
    cell, nuc, _ = snr.hand_plane()
    rng = np.random.default_rng(0)
    for route in (False, True):
        check_tables(gpu, cell, nuc, force_search=route)
        for kind in snr.ID_KINDS:
            ids = snr.ids_of(kind, cell, rng)
            want, n = snr.split_loop(cell, nuc, ids)
            assert n >= 1
            check_chain(gpu, cell, nuc, ids, force_search=route, want=want)
    ids = snr.ids_of("ascending", cell, rng)
    for min_size in (0, 14, 15, 16, 29, 30, 10 ** 6):
        check_chain(gpu, cell, nuc, ids, min_size=min_size, want=snr.split_loop(cell, nuc, ids, min_size)[0])
    g = cpu._g24()
    for name in ("hand_ascending", "hand_duplicates", "hand_min0"):
        p = "s_%s_" % name
        check_chain(gpu, g[p + "cell"], g[p + "nuc"], g[p + "ids"], int(g[p + "min_size"]), want=g[p + "out"])


def test_default_cell_ids_are_every_label_ascending(gpu):
    from ark_analysis_amd import som_device
    cell, nuc, _ = snr.hand_plane()
    got = som_device.split_large_nuclei(torch.from_numpy(cell).to(gpu), torch.from_numpy(nuc).to(gpu))
    np.testing.assert_array_equal(got.cpu().numpy(), snr.split_loop(cell, nuc, np.arange(1, 12))[0])
    with pytest.raises(IndexError, match="cell id 12 "):
        som_device.split_large_nuclei(torch.from_numpy(cell).to(gpu), torch.from_numpy(nuc).to(gpu), [1, 12])


# ---- dtypes and layouts -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_96():
    cell, nuc = snr.voronoi_case(96, 130, 40, 3)
    ids = np.unique(cell)
    ids = ids[ids != 0]
    rng = np.random.default_rng(5)
    wants = {kind: (snr.ids_of(kind, cell, rng),) for kind in snr.ID_KINDS}
    wants = {kind: (v[0], snr.split_vec(cell, nuc, v[0])[0]) for kind, v in wants.items()}
    for arr in (cell, nuc) + tuple(w[1] for w in wants.values()):
        arr.setflags(write=False)
    return cell, nuc, wants


@pytest.mark.parametrize("cell_dtype", snr.LABEL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_dtype_pair_layout_and_route(gpu, case_96, cell_dtype):
    cell, nuc, wants = case_96
    kinds = list(snr.ID_KINDS)
    for j, nuc_dtype in enumerate(snr.LABEL_DTYPES):
        c, n = cell.astype(cell_dtype), nuc.astype(nuc_dtype)
        for k, layout in enumerate(snr.FUZZ_LAYOUTS):
            route = bool((j + k) & 1)
            ids, want = wants[kinds[(j + k) % len(kinds)]]
            check_chain(gpu, c, n, ids, layout=layout, force_search=route, want=want.astype(nuc_dtype))
        check_tables(gpu, c, n, layout="offset", force_search=bool(j & 1))


def test_larger_case_with_dropped_new_pieces(gpu):
    cell, nuc = snr.voronoi_case(200, 257, 150, 5)
    rng = np.random.default_rng(6)
    check_tables(gpu, cell, nuc)
    for kind in snr.ID_KINDS:
        ids = snr.ids_of(kind, cell, rng)
        check_chain(gpu, cell, nuc, ids, force_search=kind in ("reversed", "subset"))


# ---- sparse keys, overflow ----------------------------------------------------------------------------------------
def test_sparse_labels_near_the_ends_of_int32(gpu):
    cell, nuc, _ = snr.hand_plane()
    top = 2 ** 31 - 1
    cell_map = np.zeros(12, np.int64)
    cell_map[1:] = [1, 2, 70000, 70001, 2 ** 24 + 5, 2 ** 30, 2 ** 30 + 1, top - 3, top - 2, top - 1, top]
    nuc_map = np.zeros(20, np.int64)
    nuc_map[11:] = [1, 900, 2 ** 20, 2 ** 20 + 1, 2 ** 29, 2 ** 30 + 7, top - 40, top - 39, top - 38]
    for cell_dtype, nuc_dtype in ((np.int32, np.int32), (np.int64, np.uint32), (np.uint32, np.int64)):
        c, n = cell_map[cell].astype(cell_dtype), nuc_map[nuc].astype(nuc_dtype)
        ids = np.unique(c)[1:].astype(np.int64)
        for route in (False, True):
            check_tables(gpu, c, n, force_search=route)
            if nuc_dtype == np.int32:       # top - 38 + 9 splits fits int32
                check_chain(gpu, c, n, ids[::-1].copy(), force_search=route, want=snr.split_loop(c, n, ids[::-1])[0])
            else:                           # the new labels may pass int32 in a wider plane
                check_chain(gpu, c, n, ids, force_search=route, want=snr.split_loop(c, n, ids)[0])
    # labels a wider plane holds past int32 name nothing: they are refused before any launch
    from ark_analysis_amd import som_device
    wide = torch.from_numpy(np.where(nuc == 19, 2 ** 31 + 5, nuc.astype(np.int64))).to(gpu)
    with pytest.raises(NotImplementedError, match="2147483647"):
        som_device.split_large_nuclei(torch.from_numpy(cell).to(gpu), wide)


def test_overflow_of_a_uint8_plane_writes_nothing(gpu, monkeypatch):
    from ark_analysis_amd import som_device
    cell, nuc, _ = snr.hand_plane()
    high = np.where(nuc == 19, 250, nuc).astype(np.uint8)
    buf, out = sentinel_out(gpu, 24, 70, np.uint8, "padded")

    def never(*args, **kwargs):
        raise AssertionError("the write pass was launched")
    monkeypatch.setattr(sys.modules[som_device.split_large_nuclei.__module__], "split_nuclei_apply", never)
    with pytest.raises(ValueError, match="uint8"):
        som_device.split_large_nuclei(torch.from_numpy(cell).to(gpu), torch.from_numpy(high).to(gpu), out=out)
    assert bool((buf == SENTINEL).all())
    monkeypatch.undo()
    check_chain(gpu, cell, high, np.arange(1, 7), want=snr.split_loop(cell, high, np.arange(1, 7))[0])      # 255 fits


# ---- capacity -----------------------------------------------------------------------------------------------------
def test_capacity_protocol_of_the_c_entry(gpu):
    """64 x 64 with alternating cell labels over one nucleus: every pixel is a run.  A capacity one below the runs gives
    -1 and leaves the outputs and the words around the workspace as they were; the exact capacity works."""
    from ark_analysis_amd import _capi, som_device
    lib = _capi.lib()
    h = w = 64
    cell = (np.arange(h * w).reshape(h, w) % 2 + 1).astype(np.int16)
    nuc = np.full((h, w), 7, np.uint8)
    ct, nt = torch.from_numpy(cell).to(gpu), torch.from_numpy(nuc).to(gpu)
    ck = torch.tensor([1, 2], dtype=torch.int32, device=gpu)
    nk = torch.tensor([7], dtype=torch.int32, device=gpu)
    n = torch.full((4,), -7, dtype=torch.int32, device=gpu)

    def call(area, best, capacity, ws, wsb, flags=0, **bad):
        a = dict(cd=1, nd=0, ldc=w, ldn=w, h=h, n_cells=2)
        a.update(bad)
        return lib.pxsom_nuclear_overlaps(ct.data_ptr(), a["cd"], a["ldc"], nt.data_ptr(), a["nd"], a["ldn"], a["h"], w,
                                          ck.data_ptr(), a["n_cells"], 1, 2, nk.data_ptr(), 1, 7, 7, area, best, capacity,
                                          n[1:].data_ptr(), ws, wsb, flags, _capi.stream_ptr())
    assert call(None, None, 0, None, 0) == 0
    assert n.tolist() == [-7, 0, h * w, -7]
    runs = h * w
    for capacity, flags in ((runs - 1, 0), (runs, 0), (runs, 1), (runs + 77, 0)):
        wsb = lib.pxsom_nuclear_overlaps_workspace_bytes(capacity, 2, 1, 2, 1, 7, 7, flags)
        assert wsb > 0
        ws = torch.full((wsb + 512,), 0x5A, dtype=torch.uint8, device=gpu)
        area = torch.full((3,), -7, dtype=torch.int64, device=gpu)
        best = torch.full((4, 2), -7, dtype=torch.int32, device=gpu)
        assert call(area[1:].data_ptr(), best[1:].data_ptr(), capacity, ws[256:].data_ptr(), wsb, flags) == 0
        torch.cuda.synchronize()
        assert (ws[:256] == 0x5A).all() and (ws[256 + wsb:] == 0x5A).all()
        if capacity < runs:
            assert n.tolist() == [-7, -1, runs, -7]
            assert (area == -7).all() and (best == -7).all()
        else:
            assert n.tolist() == [-7, 2, runs, -7]
            assert area.tolist() == [-7, h * w, -7]
            assert best.tolist() == [[-7, -7], [0, h * w // 2], [0, h * w // 2], [-7, -7]]
    with pytest.raises(RuntimeError, match="do not fit"):
        som_device.nuclear_overlaps(ct, nt, capacity=runs - 1)
    assert som_device.nuclear_overlaps(ct, nt, capacity=runs)[3].tolist() == [h * w // 2] * 2
    # bad arguments: refused before any HIP call, the limit in the message
    wsb = lib.pxsom_nuclear_overlaps_workspace_bytes(runs, 2, 1, 2, 1, 7, 7, 0)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=gpu)
    area, best = torch.zeros(1, dtype=torch.int64, device=gpu), torch.zeros((2, 2), dtype=torch.int32, device=gpu)
    ok = (area.data_ptr(), best.data_ptr(), runs, ws.data_ptr(), wsb)
    assert call(*ok) == 0
    for bad in (dict(cd=6), dict(nd=-1), dict(ldc=w - 1), dict(ldn=0), dict(h=0), dict(n_cells=-1)):
        assert call(*ok, **bad) == -1, bad
    assert call(*ok, flags=2) == -1 and b"flags" in lib.pxsom_last_error()
    assert call(area.data_ptr(), best.data_ptr(), 0, ws.data_ptr(), wsb) == -1
    assert call(area.data_ptr(), best.data_ptr(), (1 << 27) + 1, ws.data_ptr(), wsb) == -1
    assert b"134217728" in lib.pxsom_last_error()
    assert call(area.data_ptr(), best.data_ptr(), runs, ws.data_ptr(), wsb - 1) == -1
    assert call(area.data_ptr(), best.data_ptr(), runs, None, wsb) == -1
    assert call(area.data_ptr(), None, runs, ws.data_ptr(), wsb) == -1
    assert lib.pxsom_nuclear_overlaps_workspace_bytes(0, 2, 1, 2, 1, 7, 7, 0) == 0
    assert lib.pxsom_nuclear_overlaps_workspace_bytes((1 << 27) + 1, 2, 1, 2, 1, 7, 7, 0) == 0
    torch.cuda.synchronize()


def test_apply_tables_labels_outside_the_keys_and_bad_arguments(gpu):
    """The write pass alone: labels in no key table are copied through (nuclei) or split nothing (cells), whatever
    their value; bad arguments are refused."""
    from ark_analysis_amd import _capi, som_device
    rs = np.random.RandomState(21)
    h, w = 33, 131
    cell = rs.randint(0, 9, size=(h, w)).astype(np.int64)
    nuc = rs.randint(0, 7, size=(h, w)).astype(np.int64)
    cell[3, 5], cell[4, 6], nuc[7, 7], nuc[8, 8], nuc[9, 9] = 2 ** 40, -3, -2 ** 35, 2 ** 31, 2 ** 62
    ck, nk = np.array([1, 2, 3, 5, 8], np.int32), np.array([2, 3, 4, 6], np.int32)       # cells 4, 6, 7 and nuclei 1, 5: no key
    chosen = np.array([0, 1, 1, 3, -1], np.int32)
    cell_value = np.array([100, -1, 0, 2 ** 33, 55], np.int64)
    nuc_value = np.array([2, 0, 4, 6], np.int64)
    want = cpu.numpy_apply(cell, nuc, ck.astype(np.int64), nk.astype(np.int64), chosen, cell_value, nuc_value)
    to = lambda a: torch.from_numpy(a).to(gpu)       # noqa: E731
    for route in (False, True):
        buf, out = sentinel_out(gpu, h, w, np.int64, "offset")
        got = som_device.split_nuclei_apply(strided(gpu, cell, "padded"), strided(gpu, nuc, "offset"), to(ck), to(nk), to(chosen),
                                            to(cell_value), to(nuc_value), out=out, force_search=route)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert around_untouched(buf, (h, w), "offset")
    assert int(want[7, 7]) == -2 ** 35 and int(want[9, 9]) == 2 ** 62 and (want == 2 ** 33).any() and (want == 100).any()
    with pytest.raises(ValueError, match="chosen"):
        som_device.split_nuclei_apply(to(cell), to(nuc), to(ck), to(nk), to(chosen[:-1]), to(cell_value), to(nuc_value))
    lib = _capi.lib()
    ct, nt, out = to(cell), to(nuc), torch.zeros((h, w), dtype=torch.int64, device=gpu)
    tck, tnk, tch, tcv, tnv = to(ck), to(nk), to(chosen), to(cell_value), to(nuc_value)
    wsb = lib.pxsom_split_apply_workspace_bytes(5, 1, 8, 4, 2, 6, 0)
    ws = torch.zeros(max(wsb, 1), dtype=torch.uint8, device=gpu)

    def call(**bad):
        a = dict(cd=5, ldc=w, h=h, ldo=w, flags=0, out=out.data_ptr(), ws=ws.data_ptr(), wsb=wsb, chosen=tch.data_ptr())
        a.update(bad)
        return lib.pxsom_split_apply(ct.data_ptr(), a["cd"], a["ldc"], nt.data_ptr(), 5, w, a["h"], w, tck.data_ptr(), 5, 1, 8,
                                     tnk.data_ptr(), 4, 2, 6, a["chosen"], tcv.data_ptr(), tnv.data_ptr(), a["out"],
                                     a["ldo"], a["ws"], a["wsb"], a["flags"], _capi.stream_ptr())
    assert call() == 0
    for bad in (dict(cd=7), dict(ldc=w - 1), dict(h=-1), dict(ldo=w - 1), dict(flags=4), dict(out=None), dict(chosen=None)):
        assert call(**bad) == -1, bad
    if wsb:
        assert call(wsb=wsb - 1) == -1 and call(ws=None) == -1
    torch.cuda.synchronize()


# ---- many nuclei, empty planes, determinism ------------------------------------------------------------------------
def test_a_cell_meeting_300_nuclei(gpu):
    h, w = 40, 90
    cell = np.ones((h, w), np.int32)
    cell[:, 80:] = 2
    nuc = np.zeros((h, w), np.int32)
    flat = nuc.reshape(-1)
    flat[:3200:8] = np.arange(400) + 1000                  # 400 nuclei of one pixel (some painted over below) ...
    nuc[20:23, 10:40] = 77                                 # ... and one of 90 pixels, 20 more in cell 2
    nuc[20:22, 80:90] = 77
    nuc[30:32, 0:30] = 2000                                # a tie at 60 pixels among two, the smaller label wins
    nuc[33:35, 0:30] = 1999
    nuc[20:22, 40:80] = 0
    check_tables(gpu, cell, nuc)
    check_tables(gpu, cell, nuc, force_search=True)
    ck, nk, best, inside, _ = snr.pair_tables(cell, nuc)
    assert nk.size >= 300 and int(nk[best[0]]) == 77 and int(inside[0]) == 90
    check_chain(gpu, cell, nuc, [1, 2], want=snr.split_loop(cell, nuc, [1, 2])[0])
    nuc[20:23, 10:40] = 0                                  # now the tie decides
    ck, nk, best, inside, _ = snr.pair_tables(cell, nuc)
    assert int(nk[best[0]]) == 1999 and int(inside[0]) == 60
    check_tables(gpu, cell, nuc)
    check_chain(gpu, cell, nuc, [2, 1], min_size=0, want=snr.split_loop(cell, nuc, [2, 1], 0)[0])


def test_empty_planes(gpu):
    cell, nuc, _ = snr.hand_plane()
    zero = np.zeros_like(cell)
    for c, n in ((zero, nuc), (cell, zero), (zero, zero), (zero[:1, :1], zero[:1, :1])):
        ids = np.unique(c)[1:]
        check_tables(gpu, c, n, layout="contiguous")
        check_chain(gpu, c, n, ids, layout="contiguous", want=snr.split_loop(c, n, ids)[0] if n.any() else n)
    tiny = np.where(nuc == 19, 19, 0)[:, :14]              # 4 pixels of a nucleus and no cell: removed as small
    tiny[20, 10:] = 19
    assert int((tiny == 19).sum()) == 4
    check_chain(gpu, zero[:, :14], tiny, [], layout="contiguous", want=np.zeros_like(tiny))


def test_two_runs_give_equal_bytes(gpu):
    from ark_analysis_amd import som_device
    cell, nuc = snr.voronoi_case(200, 257, 150, 5)
    ct, nt = torch.from_numpy(cell).to(gpu), torch.from_numpy(nuc).to(gpu)
    first = [t.clone() for t in som_device.nuclear_overlaps(ct, nt)]
    plane = som_device.split_large_nuclei(ct, nt).clone()
    for route in (False, True):
        again = som_device.nuclear_overlaps(ct, nt, force_search=route)
        for a, b in zip(first, again):
            assert torch.equal(a, b)
        assert torch.equal(plane, som_device.split_large_nuclei(ct, nt, force_search=route))


# ---- field size ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1024, 2048])
def test_field_size_against_the_vectorised_statement(gpu, side):
    from ark_analysis_amd import som_device
    cell, nuc = snr.voronoi_case(side, side, 20000, side)
    ids = np.unique(cell)
    ids = ids[ids != 0]
    want, n = snr.split_vec(cell, nuc, ids)
    assert n > 500
    ct, nt = torch.from_numpy(cell).to(gpu), torch.from_numpy(nuc.astype(np.uint16)).to(gpu)
    got = som_device.split_large_nuclei(ct, nt, force_search=side == 1024)
    assert got.dtype == torch.uint16
    np.testing.assert_array_equal(got.cpu().numpy(), want.astype(np.uint16))


# ---- generate_cell_table ------------------------------------------------------------------------------------------
def test_generate_cell_table_against_the_reference_frames_and_the_numpy_frames(gpu, tmp_path):
    from ark_analysis_amd import image_io
    from ark_analysis_amd.segmentation import marker_quantification as mq
    import os
    seg_dir, tiff_dir, segs, got = cpu.check_cell_table_fixture(tmp_path)          # against g24
    # the numpy frames: the table of the planes split beforehand by the statement, without the flag
    pre_dir = os.path.join(str(tmp_path), "pre")
    os.makedirs(pre_dir)
    for name, seg in segs.items():
        if name.endswith("_nuclear.tiff"):
            cell = segs[name.replace("_nuclear", "_whole_cell")]
            ids = np.unique(cell)
            seg = snr.split_loop(cell, seg, ids[ids != 0])[0]
        image_io.write_image(os.path.join(pre_dir, name), seg)
    want = mq.generate_cell_table(pre_dir, tiff_dir, fast_extraction=True, nuclear_counts=True)
    for a, b in zip(got, want):
        pd.testing.assert_frame_equal(a, b, check_exact=True)
    # once with the regionprops lists, nc_ratio among them
    lists = dict(regionprops_base=["label", "area", "centroid", "perimeter", "major_axis_length", "minor_axis_length"],
                 regionprops_single_comp=["major_minor_axis_ratio"], regionprops_multi_comp=["nc_ratio"])
    got = mq.generate_cell_table(seg_dir, tiff_dir, nuclear_counts=True, split_large_nuclei=True, **lists)
    want = mq.generate_cell_table(pre_dir, tiff_dir, nuclear_counts=True, **lists)
    plain = mq.generate_cell_table(seg_dir, tiff_dir, nuclear_counts=True, **lists)
    assert "nc_ratio" in got[0].columns and "area_nuclear" in got[0].columns
    for a, b in zip(got, want):
        pd.testing.assert_frame_equal(a, b, check_exact=True)
    assert not got[0]["nc_ratio"].equals(plain[0]["nc_ratio"])
