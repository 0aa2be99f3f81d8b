"""Cell cluster masks on CPU: the numpy statement of pxsom_segmask (tests/cell_mask_reference.py) against the g15
fixtures of the reference (tests/golden/make_golden_cell_masks.py), the host logic of the drop-in functions of
ark_analysis_amd.utils.data_utils with their one device entry point swapped for that statement, the argument checks of
the new exports, and generate_and_save_cell_cluster_masks under a two-rank gloo group."""
import ctypes
import os
import socket

import numpy as np
import pandas as pd
import pytest

from tests import cell_mask_reference as cr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FOVS = ["fov0", "fov1", "fov2"]


def _g(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def _numpy_device(seg, erode=None, connectivity=1, background=0, table=None, unassigned=0, out_dtype=None):
    keys, values = (None, None) if table is None else table
    return cr.segmask(seg, erode, connectivity, background, keys, values, unassigned, out_dtype)


@pytest.fixture
def du(monkeypatch):
    from ark_analysis_amd.utils import data_utils
    monkeypatch.setattr(data_utils, "_segmask_device", _numpy_device)
    return data_utils


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, a.shape, b.dtype, b.shape)
    assert np.array_equal(a, b), int((a != b).sum())


# ---- the numpy statement against the reference -------------------------------------------------------------------
def test_reference_erosion_equals_fixtures():
    g = _g("g15_erode")
    seg = g["seg"]
    _same(cr.erode(seg), g["default"])
    _same(cr.erode(seg, 2, "thick")[..., None], g["c2_thick_hw1"])
    _same(cr.erode(seg, 1, "inner", 0), g["c1_inner"])
    _same(cr.erode(seg, 2, "inner", 7), g["c2_inner_bg7"])
    _same(cr.erode(g["seg16"], 2, "thick"), g["u16_c2_thick"])
    _same(cr.erode(g["seg8"]), g["u8_default"])


def _cmd_table(fov_col, label_col, cluster_col, g, prefix=""):
    return pd.DataFrame({fov_col: g[prefix + "table_fov"], label_col: g[prefix + "table_label"],
                         cluster_col: g[prefix + "table_cluster"]})


def test_reference_lookup_equals_fixtures(du):
    g = _g("g15_label_cells")
    table = _cmd_table("fov", "label", "cell_meta_cluster", g)
    cmd = du.ClusterMaskData(table, "fov", "label", "cell_meta_cluster")
    for fov in ("fov2", "fov10", "fov1"):
        rows = cmd.fov_mapping(fov)
        keys, values = cr.table_from_mapping(dict(zip(rows["label"], rows["cluster_id"])))
        _same(cr.segmask(g["seg_" + fov], keys=keys, values=values, unassigned=int(g["unassigned_id"]),
                         out_dtype=np.int16), g["mask_" + fov])
    big = g["wide_seg"]
    keys = np.concatenate([[0], g["wide_label"]]).astype(np.int32)       # with the background row 0 -> 0
    ids = pd.DataFrame({"k": np.unique(g["wide_cluster"])})
    ids["id"] = np.arange(1, len(ids) + 1)
    values = np.concatenate([[0], pd.DataFrame({"k": g["wide_cluster"]}).merge(ids, on="k")["id"].to_numpy()])
    want = g["wide_mask"]
    assert want.min() < 0 and int(g["wide_unassigned_id"]) > 32767        # the int16 wrap is exercised
    _same(cr.segmask(big, keys=keys, values=values, unassigned=int(g["wide_unassigned_id"]), out_dtype=np.int16), want)


def test_reference_float_lookup_equals_fixtures():
    g = _g("g15_map_values")
    vals = np.where(np.isfinite(g["values"]), g["values"], 0.0)
    k, v = cr.table_from_mapping(dict(zip(g["labels"].astype(np.int32), vals)))
    _same(cr.segmask(g["seg"], keys=k, values=v, unassigned=0.0, out_dtype=np.float64), g["series"])
    _same(cr.segmask(g["seg"], keys=k, values=v, unassigned=-2.5, out_dtype=np.float64), g["series_unassigned"])
    k, v = cr.table_from_mapping(dict(zip(g["arr_labels"], g["arr_values"])))
    _same(cr.segmask(g["seg"], keys=k, values=v, unassigned=0.0, out_dtype=np.float64), g["ndarray"])


def test_reference_wraps_and_casts():
    seg = np.array([[2 ** 32 + 5, -1, 7]], dtype=np.int64)
    _same(cr.segmask(seg, keys=[-1, 5], values=[10, 20], unassigned=3, out_dtype=np.int32),
          np.array([[20, 10, 3]], dtype=np.int32))
    _same(cr.segmask(np.array([[4294967295]], dtype=np.uint32), keys=[-1], values=[40000], out_dtype=np.int16),
          np.array([[40000 - 65536]], dtype=np.int16))
    _same(cr.segmask(seg, out_dtype=np.int16), seg.astype(np.int16))


# ---- the drop-in functions (host logic) against the reference ----------------------------------------------------
def test_erode_mask_dropin(du):
    g = _g("g15_erode")
    seg = g["seg"]
    _same(du.erode_mask(seg), g["default"])
    _same(du.erode_mask(seg[..., None], connectivity=2, mode="thick", background=0), g["c2_thick_hw1"])
    _same(du.erode_mask(seg, connectivity=1, mode="inner", background=0), g["c1_inner"])
    _same(du.erode_mask(seg, connectivity=2, mode="inner", background=7), g["c2_inner_bg7"])
    _same(du.erode_mask(g["seg16"], connectivity=2, mode="thick"), g["u16_c2_thick"])
    _same(du.erode_mask(g["seg8"]), g["u8_default"])


def test_erode_mask_host_path_for_float_and_bool(du):
    g = _g("g15_erode")
    seg = g["seg"]
    got = du.erode_mask(seg.astype(np.float64), connectivity=2, mode="inner", background=7)
    _same(got, g["c2_inner_bg7"].astype(np.float64))
    b = seg > 40
    want = np.where(cr.boundaries(b.astype(np.uint8)), 0, b)
    _same(du.erode_mask(b), want)


def test_erode_mask_modes_out_of_scope(du):
    seg = np.ones((4, 4), dtype=np.int32)
    for mode in ("outer", "subpixel", "thin"):
        with pytest.raises(NotImplementedError):
            du.erode_mask(seg, mode=mode)


def test_cluster_mask_data_dropin(du):
    g = _g("g15_label_cells")
    cmd = du.ClusterMaskData(_cmd_table("fov", "label", "cell_meta_cluster", g), "fov", "label", "cell_meta_cluster")
    assert cmd.mapping.to_csv(index=False) == str(g["mapping_text"])
    assert cmd.cluster_names == g["cluster_names"].tolist()
    assert cmd.unique_fovs == g["unique_fovs"].tolist()
    assert cmd.unassigned_id == int(g["unassigned_id"]) and isinstance(cmd.unassigned_id, np.int32)
    assert cmd.n_clusters == int(g["n_clusters"])
    assert list(cmd.cluster_name_id.columns) == ["cell_meta_cluster", "cluster_id"]
    with pytest.raises(ValueError):
        cmd.fov_mapping("fov99")


def test_label_cells_by_cluster_dropin(du):
    g = _g("g15_label_cells")
    cmd = du.ClusterMaskData(_cmd_table("fov", "label", "cell_meta_cluster", g), "fov", "label", "cell_meta_cluster")
    for fov in ("fov2", "fov10", "fov1"):
        _same(du.label_cells_by_cluster(fov, cmd, g["seg_" + fov]), g["mask_" + fov])
        _same(du.label_cells_by_cluster(fov, cmd, g["seg_" + fov][..., None]), g["mask_" + fov])

    class _Labelled:            # anything with .values, as an xarray DataArray
        def __init__(self, a):
            self.values = a
    _same(du.label_cells_by_cluster("fov1", cmd, _Labelled(g["seg_fov1"][None])), g["mask_fov1"])
    with pytest.raises(ValueError):
        du.label_cells_by_cluster("fov99", cmd, g["seg_fov1"])
    wide = pd.DataFrame({"fov": "fovw", "label": g["wide_label"], "k": g["wide_cluster"]})
    cmd_w = du.ClusterMaskData(wide, "fov", "label", "k")
    _same(du.label_cells_by_cluster("fovw", cmd_w, g["wide_seg"]), g["wide_mask"])


def test_map_segmentation_labels_dropin(du):
    g = _g("g15_map_values")
    _same(du.map_segmentation_labels(pd.Series(g["labels"]), pd.Series(g["values"]), g["seg"]), g["series"])
    _same(du.map_segmentation_labels(pd.Series(g["labels"]), pd.Series(g["values"]), g["seg"][None], unassigned_id=-2.5),
          g["series_unassigned"])
    got = du.map_segmentation_labels(g["arr_labels"], g["arr_values"], g["seg"])
    assert np.array_equal(got, g["ndarray"], equal_nan=True) and got.dtype == np.float64


def test_relabel_segmentation_dropin(du):
    seg = np.array([[1, 2, 3], [0, 2, 9]], dtype=np.int32)
    got = du.relabel_segmentation({1: 10, 2: 20, 0: 0, 9: 90}, np.int32(5), seg, _dtype=np.int32)
    _same(got, np.array([[10, 20, 5], [0, 20, 90]], dtype=np.int32))
    got = du.relabel_segmentation({1: 0.5, 3: -1.25}, 7.0, seg)
    _same(got, np.array([[0.5, 7.0, -1.25], [7.0, 7.0, 7.0]]))


def _write_inputs(td, g):
    from ark_analysis_amd import image_io
    seg_dir = os.path.join(td, "deepcell_output")
    os.makedirs(seg_dir)
    os.makedirs(os.path.join(td, "masks"))
    for fov in FOVS:
        image_io.write_image(os.path.join(seg_dir, fov + "_whole_cell.tiff"), g["seg_" + fov])
    with open(os.path.join(td, "names.csv"), "w") as f:
        f.write(str(g["names_text"]))
    table = pd.DataFrame({"fov": g["table_fov"], "label": g["table_label"], "cell_meta_cluster_rename": g["table_cluster"],
                          "kmeans_neighborhood": g["table_kmeans"]})
    return seg_dir, table


def _check_saved(td, g, kinds=("cell", "neighborhood")):
    from ark_analysis_amd import image_io
    assert open(os.path.join(td, "names.csv")).read() == str(g["names_after_text"])
    for fov in FOVS:
        for kind in kinds:
            got = image_io.read_image(os.path.join(td, "masks", kind + "_masks", "%s_%s_mask.tiff" % (fov, kind)))
            _same(got, g[kind + "_" + fov])


def run_saved_masks(du, td, g):
    """The notebook's call, then the neighbourhood masks, on the fixture's FOVs."""
    seg_dir, table = _write_inputs(td, g)
    du.generate_and_save_cell_cluster_masks(fovs=FOVS, save_dir=os.path.join(td, "masks"), seg_dir=seg_dir,
                                            cell_data=table, cluster_id_to_name_path=os.path.join(td, "names.csv"),
                                            cell_cluster_col="cell_meta_cluster_rename", seg_suffix="_whole_cell.tiff",
                                            sub_dir="cell_masks", name_suffix="_cell_mask")
    du.generate_and_save_neighborhood_cluster_masks(fovs=FOVS, save_dir=os.path.join(td, "masks"), seg_dir=seg_dir,
                                                    neighborhood_data=table, sub_dir="neighborhood_masks",
                                                    name_suffix="_neighborhood_mask")


def test_generate_and_save_dropin(du, tmp_path):
    g = _g("g15_saved_masks")
    run_saved_masks(du, str(tmp_path), g)
    _check_saved(str(tmp_path), g)
    cmd = du.ClusterMaskData(pd.DataFrame({"fov": g["table_fov"], "label": g["table_label"],
                                           "c": g["table_cluster"]}), "fov", "label", "c")
    _same(du.generate_cluster_mask("fov1", os.path.join(str(tmp_path), "deepcell_output"), cmd), g["cell_fov1"])


def test_generate_and_save_errors(du, tmp_path):
    g = _g("g15_saved_masks")
    td = str(tmp_path)
    seg_dir, table = _write_inputs(td, g)
    kw = dict(save_dir=os.path.join(td, "masks"), seg_dir=seg_dir, cell_data=table,
              cluster_id_to_name_path=os.path.join(td, "names.csv"), cell_cluster_col="cell_meta_cluster_rename")
    os.remove(os.path.join(seg_dir, "fov2_whole_cell.tiff"))
    with pytest.raises(ValueError):                                        # missing segmentation file
        du.generate_and_save_cell_cluster_masks(fovs=["fov0", "fov2"], **kw)
    from ark_analysis_amd import image_io
    image_io.write_image(os.path.join(seg_dir, "fov7_whole_cell.tiff"), g["seg_fov0"])
    with pytest.raises(ValueError):                                        # a FOV the cell table lacks
        du.generate_and_save_cell_cluster_masks(fovs=["fov7"], **kw)
    with pytest.raises(FileNotFoundError):                                 # no segmentation directory
        du.generate_cluster_mask("fov0", os.path.join(td, "nowhere"),
                                 du.ClusterMaskData(table, "fov", "label", "cell_meta_cluster_rename"))


# ---- argument checks of the new exports, no GPU needed -------------------------------------------------------------
def test_segmask_argument_checks():
    from ark_analysis_amd import _capi
    L = _capi.lib()
    buf = (ctypes.c_int32 * 64)()
    out = (ctypes.c_int32 * 64)()
    p, o = ctypes.addressof(buf), ctypes.addressof(out)
    keys = (ctypes.c_int32 * 2)(1, 5)
    vals = (ctypes.c_int32 * 2)(3, 4)
    kp, vp = ctypes.addressof(keys), ctypes.addressof(vals)

    def call(seg_dtype=3, h=4, w=4, ld=4, mode=0, conn=1, n_keys=-1, kmin=0, kmax=0, unassigned=0.0, out_dtype=3,
             ldo=4, ws=None, wsb=0, flags=0, seg=p, outp=o):
        return L.pxsom_segmask(seg, seg_dtype, h, w, ld, mode, conn, 0, kp, vp, n_keys, kmin, kmax, unassigned, outp,
                               out_dtype, ldo, ws, wsb, flags, None)
    bad = -1
    assert call(seg_dtype=6) == bad and call(seg_dtype=-1) == bad and call(seg_dtype=7) == bad
    assert call(out_dtype=0) == bad and call(out_dtype=7) == bad
    assert call(mode=3) == bad and call(mode=-1) == bad and call(mode=1, conn=0) == bad
    assert call(h=0) == bad and call(w=0) == bad and call(ld=3) == bad and call(ldo=3) == bad
    assert call(flags=2) == bad and call(seg=None) == bad and call(outp=None) == bad
    assert call(n_keys=2, kmin=5, kmax=1) == bad
    assert call(n_keys=2, kmin=1, kmax=5, unassigned=0.5) == bad           # integer output, fractional default
    assert call(n_keys=2, kmin=1, kmax=5, wsb=0) == bad                    # dense route without its workspace
    assert call(mode=1, conn=2, outp=p) == bad                             # erosion in place
    assert "pxsom_segmask" in L.pxsom_last_error().decode()
    assert L.pxsom_segmask_workspace_bytes(2, 1, 5) == 5 * 4
    assert L.pxsom_segmask_workspace_bytes(0, 1, 5) == 0
    assert L.pxsom_segmask_workspace_bytes(3, -5, 2 ** 31 - 1) == 0        # sparse: binary search
    assert L.pxsom_segmask_workspace_bytes(2, 5, 1) == 0


def test_segmask_wrapper_checks():
    import torch
    from ark_analysis_amd import som_device
    with pytest.raises(ValueError):
        som_device.segmask_table([3, 1], [1, 2], "cpu")
    with pytest.raises(ValueError):
        som_device.segmask_table([1, 1], [1, 2], "cpu")
    with pytest.raises(ValueError):
        som_device.segmask_table([1, 2], [1], "cpu")
    k, v, lo, hi = som_device.segmask_table([-4, 9], [1.5, 2.5], "cpu", float_values=True)
    assert (lo, hi) == (-4, 9) and v.dtype == torch.float64 and k.dtype == torch.int32
    with pytest.raises(ValueError):       # host tensor: the pass runs in HBM only
        som_device.segmentation_mask(torch.zeros((4, 4), dtype=torch.int32))


# ---- two ranks (gloo) ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, td, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from tests import oracle_backend
    from ark_analysis_amd.utils import data_utils
    data_utils._segmask_device = _numpy_device
    oracle_backend.join_cpu_group(rank, world)
    g = _g("g15_saved_masks")
    if rank == 0:
        _write_inputs(td, g)
    from ark_analysis_amd import distributed as d
    d.init_from_env()
    d.barrier()
    table = pd.DataFrame({"fov": g["table_fov"], "label": g["table_label"], "cell_meta_cluster_rename": g["table_cluster"]})
    data_utils.generate_and_save_cell_cluster_masks(fovs=FOVS, save_dir=os.path.join(td, "masks"),
                                                    seg_dir=os.path.join(td, "deepcell_output"), cell_data=table,
                                                    cluster_id_to_name_path=os.path.join(td, "names.csv"),
                                                    cell_cluster_col="cell_meta_cluster_rename", sub_dir="cell_masks",
                                                    name_suffix="_cell_mask")
    written = sorted(f for f in os.listdir(os.path.join(td, "masks", "cell_masks")))
    np.savez(out_path % rank, world=dist.get_world_size(), written=np.array(written))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_generate_and_save(tmp_path):
    import torch.multiprocessing as mp
    td = str(tmp_path)
    out_path = os.path.join(td, "rank%d.npz")
    mp.start_processes(_worker, args=(2, _free_port(), td, out_path), nprocs=2, join=True, start_method="spawn")
    g = _g("g15_saved_masks")
    _check_saved(td, g, kinds=("cell",))
    for r in range(2):
        res = np.load(out_path % r)
        assert int(res["world"]) == 2
        assert res["written"].tolist() == ["%s_cell_mask.tiff" % f for f in FOVS]
