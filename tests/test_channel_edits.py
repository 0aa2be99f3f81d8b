"""Channel edits on CPU: the g16 fixtures of the reference (tests/golden/make_golden_channel_edits.py) against the host
logic of smooth_channels / filter_with_nuclear_mask with their device entry points swapped for scipy / numpy
(tests/channel_edit_reference.py), the argument checks, file naming, the shape-keeping segmentation reader, the checks
of the two new exports, and both functions under a two-rank gloo group."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import channel_edit_reference as cer

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
DTYPES = ["uint8", "uint16", "int16", "int32", "float32"]
SHAPES = ["s37x53", "s5x3", "s1x64"]
SIGMAS = {"sig2": 2, "sig6": 6, "sig0": 0, "list": [1, 3, 2.5]}
FOVS = ["fov0", "fov1", "fov2"]


def _g(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, a.shape, b.dtype, b.shape)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), int((a != b).sum())


@pytest.fixture
def pcu(monkeypatch):
    from ark_analysis_amd.phenotyping import pixel_cluster_utils
    monkeypatch.setattr(pixel_cluster_utils, "_blur_device", cer.blur_standin)
    monkeypatch.setattr(pixel_cluster_utils, "_zero_device", cer.zero_standin)
    return pixel_cluster_utils


def write_smooth_inputs(td, g):
    from ark_analysis_amd import image_io
    for dt in DTYPES:
        os.makedirs(os.path.join(td, dt, "TIFs"), exist_ok=True)
        for ch in SHAPES:
            image_io.write_image(os.path.join(td, dt, "TIFs", ch + ".tiff"), g[f"in_{dt}_{ch}"])


def check_smooth_outputs(td, g, tag):
    from ark_analysis_amd import image_io
    for dt in DTYPES:
        for ch in SHAPES:
            _same(image_io.read_image(os.path.join(td, dt, "TIFs", ch + "_smoothed.tiff")), g[f"out_{tag}_{dt}_{ch}"])


def write_nuclear_inputs(td, g):
    from ark_analysis_amd import image_io
    tiff_dir = os.path.join(td, "tiffs")
    for fov in FOVS + ["rect"]:
        os.makedirs(os.path.join(tiff_dir, fov), exist_ok=True)
        for ch in ("chanA", "chanB"):
            image_io.write_image(os.path.join(tiff_dir, fov, ch + ".tiff"), g[f"img_{fov}_{ch}"])
    for kind in ("i64", "i32", "flat"):
        os.makedirs(os.path.join(td, "seg_" + kind), exist_ok=True)
        for fov in FOVS + (["rect"] if kind == "flat" else []):
            cer.write_shaped(os.path.join(td, "seg_" + kind, fov + "_nuclear.tiff"), g[f"seg_{kind}_{fov}"])
    return tiff_dir


def run_and_check_nuclear(pcu, td, g):
    from ark_analysis_amd import image_io
    tiff_dir = write_nuclear_inputs(td, g)
    for kind in ("i64", "i32", "flat"):
        for ch in ("chanA", "chanB"):
            for exclude in (True, False):
                pcu.filter_with_nuclear_mask(FOVS, tiff_dir, os.path.join(td, "seg_" + kind), ch, exclude=exclude)
                suffix = "_nuc_exclude.tiff" if exclude else "_nuc_include.tiff"
                for fov in FOVS:
                    _same(image_io.read_image(os.path.join(tiff_dir, fov, ch + suffix)),
                          g[f"out_{kind}_{ch}_{int(exclude)}_{fov}"])
    assert str(g["rect_error"]) == "IndexError"
    with pytest.raises(IndexError):
        pcu.filter_with_nuclear_mask(["rect"], tiff_dir, os.path.join(td, "seg_flat"), "chanA")


# ---- the fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference is not on this machine")
def test_regenerated_fixtures_match(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_channel_edits.py")], check=True, env=env,
                   capture_output=True, timeout=600)
    for name in ("g16_smooth", "g16_nuclear", "g16_cohort"):
        new, old = np.load(str(tmp_path / (name + ".npz"))), _g(name)
        assert sorted(new.files) == sorted(old.files), name
        for k in old.files:
            if name == "g16_cohort" and k == "post_values":      # see channel_edit_reference.check_cohort
                np.testing.assert_array_max_ulp(new[k], old[k], cer.POST_ULPS)
            else:
                _same(new[k], old[k])


def test_fixtures_are_live_scipy():
    """The recorded blur is scipy's own (the reference calls nothing else), including the truncation examples."""
    import scipy.ndimage as ndimage
    g = _g("g16_smooth")
    for tag, sig in SIGMAS.items():
        for dt in DTYPES:
            for j, ch in enumerate(SHAPES):
                s = sig[j] if isinstance(sig, list) else sig
                _same(ndimage.gaussian_filter(g[f"in_{dt}_{ch}"], s), g[f"out_{tag}_{dt}_{ch}"])
    assert np.all(g["const_57250"] == 57249) and np.all(g["const_14198"] == 14196)
    assert ndimage.gaussian_filter1d(np.array([0, 0, 0, 0, 100, 0, 0, 0, 0], np.uint8), 1).tolist() == \
        [0, 0, 5, 24, 39, 24, 5, 0, 0]


# ---- smooth_channels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(SIGMAS))
def test_smooth_channels_matches_reference(pcu, tmp_path, tag):
    g = _g("g16_smooth")
    td = str(tmp_path)
    write_smooth_inputs(td, g)
    pcu.smooth_channels(DTYPES, td, "TIFs", SHAPES, SIGMAS[tag])
    check_smooth_outputs(td, g, tag)


def test_smooth_channels_arguments(pcu, tmp_path):
    from ark_analysis_amd import image_io
    g = _g("g16_smooth")
    td = str(tmp_path)
    write_smooth_inputs(td, g)
    listing = sorted(os.listdir(os.path.join(td, "uint8", "TIFs")))
    pcu.smooth_channels(DTYPES, td, "TIFs", None, 2)
    pcu.smooth_channels(DTYPES, td, "TIFs", [], "not checked")
    with pytest.raises(ValueError, match="same length"):
        pcu.smooth_channels(DTYPES, td, "TIFs", SHAPES, [1, 2])
    for bad in (1.5, True, np.int64(2), (1, 2, 3)):
        with pytest.raises(ValueError, match="single integer"):
            pcu.smooth_channels(DTYPES, td, "TIFs", SHAPES, bad)
    # a sigma past the radius limit: refused before any file is written, even where it is not the first channel
    for bad in (17, [2, 3, 16.125]):
        with pytest.raises(NotImplementedError, match="16.125"):
            pcu.smooth_channels(DTYPES, td, "TIFs", SHAPES, bad)
    assert sorted(os.listdir(os.path.join(td, "uint8", "TIFs"))) == listing
    # a missing channel raises what the pixel-matrix reader raises; FOVs before it are written
    os.remove(os.path.join(td, "int16", "TIFs", "s5x3.tiff"))
    with pytest.raises(FileNotFoundError, match="s5x3"):
        pcu.smooth_channels(DTYPES, td, "TIFs", SHAPES, 2)
    for dt in ("uint8", "uint16"):
        _same(image_io.read_image(os.path.join(td, dt, "TIFs", "s1x64_smoothed.tiff")), g[f"out_sig2_{dt}_s1x64"])
    # no sub folder
    os.makedirs(os.path.join(td, "flat"))
    image_io.write_image(os.path.join(td, "flat", "c.tiff"), g["in_uint16_s37x53"])
    pcu.smooth_channels(["flat"], td, None, ["c"], 6)
    _same(image_io.read_image(os.path.join(td, "flat", "c_smoothed.tiff")), g["out_sig6_uint16_s37x53"])


def test_sigma_limit():
    from ark_analysis_amd import som_device
    for ok in (16, 16.12, 0, -3, 1e-16):
        som_device.check_blur_sigma(ok)
    for bad in (16.125, 17, 100.0):
        with pytest.raises(NotImplementedError, match="radius limit"):
            som_device.check_blur_sigma(bad)


# ---- filter_with_nuclear_mask ---------------------------------------------------------------------------------------
def test_filter_with_nuclear_mask_matches_reference(pcu, tmp_path):
    run_and_check_nuclear(pcu, str(tmp_path), _g("g16_nuclear"))


def test_filter_with_nuclear_mask_arguments(pcu, tmp_path, capsys):
    g = _g("g16_nuclear")
    pcu.filter_with_nuclear_mask(FOVS, "", None, "chanA")
    assert capsys.readouterr().out == str(g["no_seg_stdout"])
    with pytest.raises(FileNotFoundError):
        pcu.filter_with_nuclear_mask(FOVS, "", str(tmp_path / "bad_seg_path"), "chanA")
    td = str(tmp_path)
    tiff_dir = write_nuclear_inputs(td, g)
    with pytest.raises(FileNotFoundError):          # no segmentation with that suffix
        pcu.filter_with_nuclear_mask(FOVS, tiff_dir, os.path.join(td, "seg_i64"), "chanA", nuc_seg_suffix="_x.tiff")
    with pytest.raises(FileNotFoundError):          # no such channel
        pcu.filter_with_nuclear_mask(FOVS, tiff_dir, os.path.join(td, "seg_i64"), "chanZ")


def test_segmentation_reader(tmp_path):
    """What skimage.io.imread returns for the files the reference's test writes (io.imsave of an int64 (1, 10, 10)
    array: one page, tifffile shape description) and for deepcell's 2-D int32 masks (deflate); read_image, which the
    cell masks use, cannot read the first and stays as it is."""
    from PIL import UnidentifiedImageError
    from ark_analysis_amd import image_io
    rs = np.random.RandomState(3)
    a = rs.randint(1, 16, size=(1, 10, 10))
    cer.write_shaped(str(tmp_path / "a.tiff"), a)
    _same(image_io.read_tiff_shaped(str(tmp_path / "a.tiff")), a)
    _same(cer.read_shaped(str(tmp_path / "a.tiff")), a)
    with pytest.raises(UnidentifiedImageError):
        image_io.read_image(str(tmp_path / "a.tiff"))
    b = rs.randint(0, 900, size=(13, 7)).astype(np.int32)
    cer.write_shaped(str(tmp_path / "b.tiff"), b, compress=True)
    _same(image_io.read_tiff_shaped(str(tmp_path / "b.tiff")), b)
    _same(image_io.read_image(str(tmp_path / "b.tiff")), b)
    for dt in (np.uint8, np.int16, np.uint16, np.int32, np.float32):           # write_image's files: plain (H, W)
        c = rs.randint(0, 100, size=(5, 6)).astype(dt)
        image_io.write_image(str(tmp_path / "c.tiff"), c)
        _same(image_io.read_tiff_shaped(str(tmp_path / "c.tiff")), c)
    for dt in (np.uint32, np.int64, np.uint64, np.float64, np.int8):
        d = rs.randint(0, 100, size=(1, 4, 3)).astype(dt)
        cer.write_shaped(str(tmp_path / "d.tiff"), d)
        _same(image_io.read_tiff_shaped(str(tmp_path / "d.tiff")), d)


def test_cohort_cells_20_22_26(som_backend, pcu, tmp_path, capsys):
    if som_backend != "oracle":
        pytest.skip("the device run is in test_gpu_channel_edits.py")
    from ark_analysis_amd.fov_tables import read_dataframe
    from ark_analysis_amd import image_io
    from ark_analysis_amd.phenotyping import pixie_preprocessing
    g, want = cer.cohort_inputs(), _g("g16_cohort")
    td = str(tmp_path)
    os.makedirs(os.path.join(td, "pixel_output_dir"))
    tiff_dir, seg_dir = cer.write_cohort(td, g, image_io.write_image)
    channels = cer.run_cohort(td, tiff_dir, seg_dir, pcu, pixie_preprocessing)
    assert capsys.readouterr().out == str(want["stdout"])
    cer.check_cohort(cer.cohort_outputs(td, channels, read_dataframe), want, _same)


# ---- the exports ----------------------------------------------------------------------------------------------------
def test_new_export_argument_checks():
    from ark_analysis_amd import _capi
    L = _capi.lib()
    a, b, c = (ctypes.c_float * 64)(), (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    pa, pb, pc = ctypes.addressof(a), ctypes.addressof(b), ctypes.addressof(c)
    wts = (ctypes.c_double * 3)(0.25, 0.5, 0.25)
    pw = ctypes.addressof(wts)

    def blur(i=pa, o=pb, t=pc, h=8, w=8, dtype=7, weights=pw, radius=1):
        return L.pxsom_gaussian_blur_plane(i, o, t, h, w, dtype, weights, radius, None)
    bad, unsupported = -1, -2                 # PXSOM_ERR_INVALID_ARG, PXSOM_ERR_UNSUPPORTED
    for dtype in (-1, 4, 5, 6, 8):
        assert blur(dtype=dtype) == bad
    assert blur(h=0) == bad and blur(w=0) == bad and blur(i=None) == bad and blur(o=None) == bad
    assert blur(t=None) == bad and blur(weights=None) == bad and blur(t=pa) == bad and blur(t=pb) == bad
    assert blur(radius=65) == unsupported and blur(radius=-1) == unsupported
    assert "pxsom_gaussian_blur_plane" in L.pxsom_last_error().decode()

    def zero(img=pa, idt=7, seg=pb, sdt=3, n=64, exclude=1):
        return L.pxsom_zero_by_seg(img, idt, seg, sdt, n, exclude, None)
    for idt in (-1, 4, 5, 6, 8):
        assert zero(idt=idt) == bad
    for sdt in (-1, 6, 7):
        assert zero(sdt=sdt) == bad
    assert zero(n=-1) == bad and zero(img=None) == bad and zero(seg=None) == bad and zero(exclude=2) == bad
    assert "pxsom_zero_by_seg" in L.pxsom_last_error().decode()
    assert zero(n=0, img=None, seg=None) == 0                          # nothing to do: no HIP call either


def test_wrapper_checks():
    import torch
    from ark_analysis_amd import som_device
    with pytest.raises(ValueError):           # host tensors: the passes run in HBM only
        som_device.gaussian_blur_plane(torch.zeros((4, 4), dtype=torch.float32), 2.0)
    with pytest.raises(ValueError):
        som_device.zero_by_segmentation(torch.zeros((4, 4), dtype=torch.float32), torch.zeros((4, 4), dtype=torch.int32))


# ---- two ranks (gloo) -----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, td):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from tests import oracle_backend
    from ark_analysis_amd.phenotyping import pixel_cluster_utils as pcu
    pcu._blur_device = cer.blur_standin
    pcu._zero_device = cer.zero_standin
    oracle_backend.join_cpu_group(rank, world)
    from ark_analysis_amd import distributed as d
    d.init_from_env()
    gs, gn = _g("g16_smooth"), _g("g16_nuclear")
    if rank == 0:
        write_smooth_inputs(td, gs)
        write_nuclear_inputs(td, gn)
    d.barrier()
    pcu.smooth_channels(DTYPES, td, "TIFs", SHAPES, [1, 3, 2.5])
    pcu.filter_with_nuclear_mask(FOVS, os.path.join(td, "tiffs"), os.path.join(td, "seg_i64"), "chanB")
    # every rank sees every file when the calls return
    check_smooth_outputs(td, gs, "list")
    from ark_analysis_amd import image_io
    for fov in FOVS:
        _same(image_io.read_image(os.path.join(td, "tiffs", fov, "chanB_nuc_exclude.tiff")), gn[f"out_i64_chanB_1_{fov}"])
    assert dist.get_world_size() == 2
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_write_what_one_rank_writes(tmp_path):
    import torch.multiprocessing as mp
    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
