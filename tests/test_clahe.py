"""Adaptive histogram equalisation of fibre segmentation (K27) without a GPU: the numpy / scipy statement of
tests/clahe_reference.py against the g30 fixture, the index facts the kernels rely on, the statement's own properties,
contrast_adjusted_channel and fiber_watershed_inputs_from_channel with their device entries swapped for that statement, the
refusals, the debug files, the ABI."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage

from ark_analysis_amd import image_io
from ark_analysis_amd.segmentation import fiber_segmentation as fs
from tests import clahe_reference as cr
from tests import fiber_markers_reference as fmr
from tests import frangi_reference as fr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
FIXTURE = "g30_clahe.npz"


@pytest.fixture(scope="module")
def g30():
    return np.load(os.path.join(GOLDEN, FIXTURE))


@pytest.fixture(scope="module")
def cases():
    return cr.fixture_cases()


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture
def statement_as_device(monkeypatch):
    monkeypatch.setattr(fs, "_contrast_device", cr.contrast_device)
    monkeypatch.setattr(fs, "_channel_watershed_inputs_device", cr.channel_watershed_inputs_device)
    return fs


# ---- the statement against the fixture ---------------------------------------------------------------------------------------
def test_statement_equals_the_fixture(g30, cases):
    assert json.loads(str(g30["names"])) == list(cases) and len(cases) == 14
    assert json.loads(str(g30["branch_names"])) == list(cr.BRANCHES)
    reached = np.zeros(len(cr.BRANCHES), np.int64)
    stored_in_full = 0
    for name, (x, k, clip_limit) in cases.items():
        assert int(g30["k_" + name]) == k and float(g30["clip_limit_" + name]) == clip_limit
        assert int(g30["clim_" + name]) == cr.clip_limit_count(k, clip_limit)
        result, gray, maps, raw = cr.equalize_adapthist(x, k, clip_limit)
        assert same(result, g30["result_" + name]), name
        if x.size <= cr.FULL_LIMIT:
            stored_in_full += 1
            assert same(gray, g30["gray_" + name]) and same(raw, g30["raw_" + name]), name
            assert same(maps.astype(np.uint16), g30["maps_" + name]), name
        else:
            for key, a in (("gray", gray), ("maps", maps.astype(np.uint16)), ("raw", raw)):
                assert digest(a) == str(g30["sha256_%s_%s" % (key, name)]), (name, key)
        reached += g30["branches_" + name]
    assert stored_in_full >= 8
    assert (reached > 0).all(), dict(zip(cr.BRANCHES, reached.tolist()))          # the file reaches every branch
    # the clip limits of the cases the issue names
    assert [int(g30["clim_" + n]) for n in ("bars_k32", "smooth_k32_clim3", "bars_k32_noclip", "bars_16x16_k8", "bars_32x32_k16")] \
        == [10, 3, cr.NR, 1, 2]
    branches = dict(zip(cr.BRANCHES, g30["branches_smooth_k32_clim3"].tolist()))
    assert branches["loop_all_indices"] == branches["loop_second_pass"] == branches["break_no_progress"] == 4
    branches = dict(zip(cr.BRANCHES, g30["branches_bars_k32"].tolist()))
    assert branches["bin_incr"] and branches["mid"] and branches["excess_below_zero"]
    assert dict(zip(cr.BRANCHES, g30["branches_bars_k32_noclip"].tolist()))["no_excess"] == 4


def test_chained_case_carries_every_later_stage(g30):
    channel = cr.chain_channel()
    contrast, gray, maps, raw = cr.contrast_adjust(channel, float(g30["chain_blur"]), int(g30["chain_k"]))
    assert same(contrast, g30["chain_contrast"]) and same(gray, g30["chain_gray"]) and same(raw, g30["chain_raw"])
    assert same(maps.astype(np.uint16), g30["chain_maps"])
    ridges = fr.frangi(contrast, fr.SIGMAS, fr.BETA, fr.GAMMA, fr.SCALE)
    assert same(ridges, g30["chain_ridges"])
    s = fmr.stages(ridges, float(g30["cutoff"]), float(g30["sobel_blur"]))
    for key in ("fg", "dist", "counts", "markers", "elev", "elevation"):
        assert same(s[key], g30["chain_" + key]), key
    assert [s["t0"], s["t1"]] == g30["chain_thr"].tolist()
    assert (np.bincount(g30["chain_markers"].ravel(), minlength=3) > 0).all()


def test_generator_reproduces_the_fixture(tmp_path):
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_clahe.py")], check=True, env=env, stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / FIXTURE), np.load(os.path.join(GOLDEN, FIXTURE))
    assert sorted(new.files) == sorted(old.files)
    for key in old.files:
        assert new[key].dtype == old[key].dtype and np.array_equal(new[key], old[key]), key
    assert os.path.getsize(os.path.join(GOLDEN, FIXTURE)) <= 211804          # g28's size, the bound g29 keeps


def test_every_recalled_convention_is_named():
    assert set(cr.RECALLED_CLAHE) == {"grey_levels", "bin_size", "pad", "tile_origin", "clim", "clip_phases", "map_scale", "map_pad",
                                      "coefficients", "corner_order", "truncation", "rescales", "round"}
    assert all(isinstance(v, str) and v for v in cr.RECALLED_CLAHE.values())
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "K27" in design and "parity with skimage itself is unpinned" in design.lower().replace("\n", " ")


# ---- the index facts the kernels use -------------------------------------------------------------------------------------------
SIZES_AND_K = [((2, 2), 1), ((2, 2), 2), ((3, 5), 2), ((3, 5), 3), ((8, 8), 8), ((9, 7), 7), ((17, 33), 4), ((17, 33), 5),
               ((16, 24), 8), ((40, 90), 7), ((33, 31), 3), ((35, 29), 5), ((64, 64), 32)]


def test_tiles_cover_the_plane_from_its_origin_with_one_reflection():
    for (h, w), k in SIZES_AND_K:
        gray = (np.arange(h * w, dtype=np.uint16).reshape(h, w) * 65) % cr.NR            # bin = index mod 252: positions show
        img, ps, nh, hist = cr.tile_histograms(gray, k)
        assert ps == k // 2 and nh == [-(-h // k), -(-w // k)]
        assert img.shape[0] % k == 0 and img.shape[1] % k == 0 and [s // k for s in img.shape] == [n + 1 for n in nh]
        bins = gray // 65
        for ty in range(nh[0]):
            rows = np.arange(ty * k, (ty + 1) * k)
            assert rows.max() < h + k <= 2 * h                                           # one reflection always suffices
            rows = np.where(rows >= h, 2 * (h - 1) - rows, rows)
            assert rows.min() >= 0
            for tx in range(nh[1]):
                cols = np.arange(tx * k, (tx + 1) * k)
                cols = np.where(cols >= w, 2 * (w - 1) - cols, cols)
                assert cols.min() >= 0
                want = np.bincount(bins[np.ix_(rows, cols)].ravel(), minlength=256)
                assert np.array_equal(hist[ty * nh[1] + tx], want), ((h, w), k, ty, tx)


def interpolate_by_index(gray, maps, k):
    """The interpolation as the kernel forms it: no padded plane, p = r + k // 2, b = p // k, j = p % k per axis."""
    h, w = gray.shape
    nty, ntx = maps.shape[:2]
    bins = (gray // 65).astype(np.int64)
    py, px = np.arange(h) + k // 2, np.arange(w) + k // 2
    by, jy, bx, jx = py // k, py % k, px // k, px % k
    ty = [np.clip(by - 1, 0, nty - 1), np.clip(by, 0, nty - 1)]
    tx = [np.clip(bx - 1, 0, ntx - 1), np.clip(bx, 0, ntx - 1)]
    cr_, cc_ = jy / k, jx / k
    wy, wx = [1 - cr_, cr_], [1 - cc_, cc_]
    acc = np.zeros((h, w), np.float32)
    for er, ec in ((0, 0), (0, 1), (1, 0), (1, 1)):
        mapped = maps[ty[er][:, None], tx[ec][None, :], bins]
        acc += (mapped * (wy[er][:, None] * wx[ec][None, :])).astype(np.float32)
    return acc.astype(np.uint16)


def test_interpolation_by_index_equals_the_statement():
    for (h, w), k in SIZES_AND_K:
        for name in ("noise", "fibres"):
            plane = cr.patterns(h, w)[name]
            _, gray, maps, raw = cr.equalize_adapthist(plane, k)
            assert np.array_equal(interpolate_by_index(gray, maps, k), raw), ((h, w), k, name)


def test_the_minimum_of_the_divided_plane_is_the_divided_minimum():
    rs = np.random.RandomState(27)
    for _ in range(200):
        b = rs.random_sample((5, 7)) * 10.0 ** rs.randint(-8, 8)
        assert (b / b.max()).min() == b.min() / b.max() and (b / b.max()).max() == 1.0
    # so the statement's first rescale over the divided plane is the quantisation over (min / max, 1.0)
    channel = cr.chain_channel()
    b = scipy.ndimage.gaussian_filter(channel, sigma=2)
    x = b / b.max()
    lo, hi = b.min() / b.max(), 1.0
    gray = np.round((np.clip(x, lo, hi) - lo) / (hi - lo) * (cr.NR - 1) + 0).astype(np.uint16)
    assert np.array_equal(gray, cr.contrast_adjust(channel, 2, 8)[1])


# ---- the statement's own properties ----------------------------------------------------------------------------------------
def test_outputs_lie_in_the_unit_interval_with_both_ends(g30, cases):
    for name, (x, k, clip_limit) in cases.items():
        result = g30["result_" + name]
        assert result.min() >= 0.0 and result.max() <= 1.0, name
        if name == "constant":
            assert x.min() == x.max() == 1.0 and (result == result[0, 0]).all()
        else:
            assert result.min() == 0.0 and result.max() == 1.0, name


def test_a_power_of_two_factor_changes_nothing(cases):
    for name in ("bars_16x16_k8", "odd_35x29_k5", "smooth_k32_clim3"):
        x, k, clip_limit = cases[name]
        want = cr.equalize_adapthist(x, k, clip_limit)
        for factor in (2.0 ** -20, 4.0, 2.0 ** 40):
            got = cr.equalize_adapthist(x * factor, k, clip_limit)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, factor)


def test_clip_limit_zero_disables_clipping():
    x = cr.fixture_cases()["bars_k32_noclip"][0]
    _, gray, maps, _ = cr.equalize_adapthist(x, 32, 0.0)
    _, _, _, hist = cr.tile_histograms(gray, 32)
    assert np.array_equal(maps.reshape(-1, 256), cr.map_histogram(hist, 0, cr.NR - 1, 1024))
    assert cr.clip_limit_count(32, 0.0) == cr.clip_limit_count(32, -1.0) == cr.NR


# ---- the host functions over the swapped statement ---------------------------------------------------------------------------
def divisor_for(channel, k):
    return channel.shape[0] / (k + 0.5)              # image.shape[0] / divisor = k + 0.5, which int() takes to k


def test_contrast_adjusted_channel_equals_the_fixture(statement_as_device, g30):
    for name, (channel, k, clip_limit) in cr.fixture_channels().items():
        if clip_limit != cr.CLIP_LIMIT:
            continue
        got = fs.contrast_adjusted_channel(channel, blur=2, contrast_scaling_divisor=divisor_for(channel, k))
        assert same(got, g30["result_" + name]), name
    channel = cr.fixture_channels()["bars_16x16_k8"][0]
    assert np.array_equal(fs.contrast_adjusted_channel(channel.astype(np.float32).astype(np.float64), contrast_scaling_divisor=2),
                          fs.contrast_adjusted_channel(channel.astype(np.float32), 2, 2))
    # the defaults are the reference's: blur 2, fov_len / 128
    big = cr.patterns(256, 20)["fibres"]
    assert np.array_equal(fs.contrast_adjusted_channel(big), cr.contrast_adjust(big, 2, 2)[0])


def test_the_device_entries_receive_checked_arguments(monkeypatch):
    calls = []

    def entry(channel, blur, kernel_size, clip_limit):
        calls.append((channel.dtype, channel.shape, blur, kernel_size, clip_limit))
        return np.zeros(channel.shape, np.float32)

    monkeypatch.setattr(fs, "_contrast_device", entry)
    got = fs.contrast_adjusted_channel(np.ones((12, 9), np.int16), blur=1, contrast_scaling_divisor=4)
    assert calls == [(np.float64, (12, 9), 1.0, 3.0, 0.01)] and got.dtype == np.float64
    assert all(type(v) is float for v in calls[0][2:])

    def chain(channel, blur, kernel_size, sigmas, ridge_cutoff, sobel_blur, thresholds):
        calls.append((channel.dtype, blur, kernel_size, sigmas, ridge_cutoff, sobel_blur, thresholds))
        z = np.zeros(channel.shape)
        return z.astype(np.float32), z, z, (0.5, 1.5), z.astype(np.int64), z.astype(np.int64)

    monkeypatch.setattr(fs, "_channel_watershed_inputs_device", chain)
    inputs, ridges, contrast = fs.fiber_watershed_inputs_from_channel(np.ones((8, 9), np.float32), contrast_scaling_divisor=2,
                                                                      ridge_cutoff=0.25, sobel_blur=2)
    assert calls[1] == (np.float64, 2.0, 4.0, [1.0, 3.0, 5.0, 7.0, 9.0], 0.25, 2, fs.threshold_multiotsu_from_histogram)
    assert isinstance(inputs, fs.WatershedInputs) and inputs.markers.dtype == np.int32 and inputs.thresholds.tolist() == [0.5, 1.5]
    assert ridges.dtype == np.float64 and contrast.dtype == np.float64


def test_chain_from_channel_equals_the_fixture(statement_as_device, g30):
    channel = cr.chain_channel()
    divisor = channel.shape[0] / int(g30["chain_k"])
    inputs, ridges, contrast = fs.fiber_watershed_inputs_from_channel(channel, blur=float(g30["chain_blur"]), contrast_scaling_divisor=divisor,
                                                                      ridge_cutoff=float(g30["cutoff"]), sobel_blur=float(g30["sobel_blur"]))
    assert same(contrast, g30["chain_contrast"]) and same(ridges, g30["chain_ridges"])
    assert same(inputs.distance_transformed, g30["chain_dist"]) and same(inputs.thresholds, g30["chain_thr"])
    assert same(inputs.markers, g30["chain_markers"]) and same(inputs.elevation_map, g30["chain_elevation"])
    # the chain is contrast_adjusted_channel followed by fiber_watershed_inputs_from_contrast
    assert np.array_equal(contrast, fs.contrast_adjusted_channel(channel, contrast_scaling_divisor=divisor))
    monkey = pytest.MonkeyPatch()
    monkey.setattr(fs, "_ridge_watershed_inputs_device", fr.ridge_watershed_inputs_device)
    try:
        again, again_ridges = fs.fiber_watershed_inputs_from_contrast(contrast)
    finally:
        monkey.undo()
    assert np.array_equal(again_ridges, ridges) and np.array_equal(again.markers, inputs.markers)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_clahe_arguments():
    from ark_analysis_amd import som_device
    from ark_analysis_amd.som_device import planes
    for name in ("clahe_arguments", "equalize_adapthist", "contrast_adjust", "channel_watershed_inputs", "CLAHE_GREY_LEVELS", "CLAHE_NBINS"):
        assert getattr(som_device, name) is getattr(planes, name), name
    assert planes.CLAHE_GREY_LEVELS == cr.NR and planes.CLAHE_NBINS == cr.NBINS
    assert planes.clahe_arguments((64, 64), 32) == (32, 10, 16383 / 1024)
    assert planes.clahe_arguments((64, 64), 32, 0.003) == (32, 3, 16383 / 1024)
    assert planes.clahe_arguments((16, 24), 8.9) == (8, 1, 16383 / 64)
    assert planes.clahe_arguments((16, 24), np.float32(16), clip_limit=0.0) == (16, cr.NR, 16383 / 256)
    assert planes.clahe_arguments((16, 24), 16, clip_limit=-1) == (16, cr.NR, 16383 / 256)
    assert planes.clahe_arguments([2, 2], 2, nbins=256) == (2, 1, 16383 / 4)
    assert planes.clahe_arguments((1024, 1024), 1024 / 128)[:2] == (8, 1)
    for k, clip_limit in ((32, 0.01), (32, 0.003), (8, 0.01), (16, 0.01), (5, 0.0), (7, 2.0)):
        assert planes.clahe_arguments((64, 64), k, clip_limit)[1] == cr.clip_limit_count(k, clip_limit)
    for shape in ((1, 8), (8, 1), (8,), (2, 3, 4), ()):
        with pytest.raises(ValueError, match="H, W >= 2"):
            planes.clahe_arguments(shape, 1)
    for nbins in (128, 255, 257, 0, None, True):
        with pytest.raises(NotImplementedError, match="only 256 bins"):
            planes.clahe_arguments((8, 8), 2, nbins=nbins)
    for bad in (0, 0.99, -3, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite and at least 1"):
            planes.clahe_arguments((8, 8), bad)
    for bad in (9, 8.0 + 1, 100):
        with pytest.raises(NotImplementedError, match="beyond the shorter side"):
            planes.clahe_arguments((8, 12), bad)
    assert planes.clahe_arguments((8, 12), 8.99)[0] == 8
    for bad in ((2, 2), [4, 4], np.array([2, 2]), None):
        with pytest.raises(NotImplementedError, match="scalar kernel size"):
            planes.clahe_arguments((8, 8), bad)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="clip_limit must be finite"):
            planes.clahe_arguments((8, 8), 2, clip_limit=bad)
    import torch
    with pytest.raises(ValueError, match="2-D float64 HBM tensor"):
        som_device.equalize_adapthist(torch.zeros((4, 4), dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="float64 HBM tensor"):
        som_device.contrast_adjust(torch.zeros((4, 4), dtype=torch.float64))


def test_refusals_of_the_host_functions(statement_as_device):
    x = np.add.outer(np.arange(16.0), np.arange(12.0)) + 1.0
    for call in (lambda image=x, **kw: fs.contrast_adjusted_channel(image, **kw),
                 lambda image=x, **kw: fs.fiber_watershed_inputs_from_channel(image, **kw)):
        for bad in (np.zeros(5), np.zeros((2, 3, 4)), np.zeros((0, 4))):
            with pytest.raises(ValueError, match="non-empty \\[H, W\\]"):
                call(bad)
        for shape in ((1, 7), (7, 1)):
            with pytest.raises(ValueError, match="H, W >= 2"):
                call(np.ones(shape), contrast_scaling_divisor=1)
        with pytest.raises(ValueError, match="finite and at least 1"):
            call()                                                      # 16 / 128: the reference divides by zero there
        with pytest.raises(ValueError, match="finite and at least 1"):
            call(contrast_scaling_divisor=16.5)
        with pytest.raises(NotImplementedError, match="beyond the shorter side"):
            call(contrast_scaling_divisor=1)                            # k = 16 > 12
        for bad in (0, -2, np.nan, np.inf):
            with pytest.raises(ValueError, match="contrast_scaling_divisor"):
                call(contrast_scaling_divisor=bad)
        for bad in (-1, np.nan, np.inf):
            with pytest.raises(ValueError, match="blur must be finite"):
                call(contrast_scaling_divisor=4, blur=bad)
        with pytest.raises(NotImplementedError, match="sigma 17.0 is beyond the radius limit"):
            call(contrast_scaling_divisor=4, blur=17)
        with_nan = x.copy()
        with_nan[3, 4] = np.nan
        with pytest.raises(ValueError, match="image must be finite"):
            call(with_nan, contrast_scaling_divisor=4)
        with_inf = x.copy()
        with_inf[3, 4] = np.inf
        with pytest.raises(ValueError, match="image must be finite"):
            call(with_inf, contrast_scaling_divisor=4)
        for dark in (np.zeros((16, 12)), -x):
            with pytest.raises(ValueError, match="positive pixel"):
                call(dark, contrast_scaling_divisor=4)
    assert fs.contrast_adjusted_channel(x, contrast_scaling_divisor=4).shape == (16, 12)
    assert fs.contrast_adjusted_channel(x, contrast_scaling_divisor=4, blur=0).shape == (16, 12)
    with pytest.raises(ValueError, match="at least one sigma"):
        fs.fiber_watershed_inputs_from_channel(x, contrast_scaling_divisor=4, fiber_widths=[])
    with pytest.raises(NotImplementedError, match="sigma 17"):
        fs.fiber_watershed_inputs_from_channel(x, contrast_scaling_divisor=4, sobel_blur=17)


# ---- the debug files ---------------------------------------------------------------------------------------------------------
def test_debug_files(statement_as_device, g30, tmp_path):
    channel = cr.chain_channel()
    divisor = channel.shape[0] / int(g30["chain_k"])
    got = fs.contrast_adjusted_channel(channel, contrast_scaling_divisor=divisor, out_dir=str(tmp_path), fov="fov3", debug=True)
    assert os.listdir(tmp_path / "_debug") == ["fov3_contrast_adjusted.tiff"]
    saved = image_io.read_image(str(tmp_path / "_debug" / "fov3_contrast_adjusted.tiff"))
    assert saved.dtype == np.float32 and np.array_equal(saved, g30["chain_contrast"].astype(np.float32))
    assert np.array_equal(got, g30["chain_contrast"])
    chain_dir = tmp_path / "chain"
    chain_dir.mkdir()
    fs.fiber_watershed_inputs_from_channel(channel, contrast_scaling_divisor=divisor, out_dir=str(chain_dir), fov="fov4", debug=True)
    assert sorted(os.listdir(chain_dir / "_debug")) == ["fov4_contrast_adjusted.tiff", "fov4_frangi_filter.tiff",
                                                        "fov4_ridges_thresholded.tiff", "fov4_thresholded.tiff"]
    read = lambda name: image_io.read_image(str(chain_dir / "_debug" / ("fov4_%s.tiff" % name)))      # noqa: E731
    assert np.array_equal(read("contrast_adjusted"), saved)
    assert np.array_equal(read("frangi_filter"), g30["chain_ridges"].astype(np.float32))
    assert np.array_equal(read("thresholded"), g30["chain_markers"])
    assert np.array_equal(read("ridges_thresholded"), g30["chain_dist"].astype(np.float32))
    for call in (fs.contrast_adjusted_channel, fs.fiber_watershed_inputs_from_channel):
        call(channel, contrast_scaling_divisor=divisor, out_dir=str(tmp_path / "quiet"), fov="fov3", debug=False)
        call(channel, contrast_scaling_divisor=divisor, debug=True)
        assert not (tmp_path / "quiet").exists()
        with pytest.raises(FileNotFoundError):
            call(channel, contrast_scaling_divisor=divisor, out_dir=str(tmp_path / "missing"), fov="fov3", debug=True)
        with pytest.raises(ValueError, match="need fov"):
            call(channel, contrast_scaling_divisor=divisor, out_dir=str(tmp_path), debug=True)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pxsom_plane_divide", "pxsom_clahe_quantize", "pxsom_clahe_workspace_bytes", "pxsom_clahe_equalize")


def test_abi_symbols_and_refusals():
    from ark_analysis_amd import _capi
    header = open(os.path.join(ROOT, "include", "pxsom.h")).read()
    assert _capi.ABI_VERSION == 9 and "K27" in header
    lib = _capi.lib()
    assert lib.pxsom_abi_version() == 9
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and re.search(r"\b%s\(" % name, header) and hasattr(lib, name), name
    invalid, unsupported = -1, -2                       # PXSOM_ERR_INVALID_ARG, PXSOM_ERR_UNSUPPORTED
    # host arrays stand in for the device buffers: every call below is refused before any HIP call
    src, out = np.zeros(64), np.zeros(64)
    gray, raw, maps = np.zeros(64, np.uint16), np.zeros(64, np.uint16), np.zeros(4 * 256, np.uint16)
    need = lib.pxsom_clahe_workspace_bytes(8, 8, 4)
    assert need == 16 + 4 * 512 + 128 and lib.pxsom_clahe_workspace_bytes(8, 8, 8) == 16 + 512 + 128
    for h, w, k in ((1, 8, 1), (8, 1, 1), (8, 8, 0), (8, 8, 9), (8, 12, 9), (65536, 65536, 8)):
        assert lib.pxsom_clahe_workspace_bytes(h, w, k) == 0
    ws = np.zeros(need // 8 + 2, np.float64)             # 8-byte aligned storage; the 16-byte aligned address inside it
    S, O, G, R, M = src.ctypes.data, out.ctypes.data, gray.ctypes.data, raw.ctypes.data, maps.ctypes.data
    W = (ws.ctypes.data + 15) // 16 * 16

    def refused(name, code, args):
        rc = getattr(lib, name)(*args)
        assert rc == code and lib.pxsom_last_error().decode().startswith(name), (name, args, rc)

    def but(good, order, **changes):
        args = list(good)
        for key, value in changes.items():
            args[order.index(key)] = value
        return args

    order = ("src", "h", "w", "ld", "lo", "hi", "gray", "ldg", "stream")
    good = [S, 8, 8, 8, 0.0, 1.0, G, 8, None]
    for changes in (dict(src=None), dict(gray=None), dict(h=1), dict(w=1), dict(h=0), dict(w=-3), dict(ld=7), dict(ldg=7),
                    dict(src=S + 4), dict(gray=G + 1), dict(gray=S), dict(gray=S + 8 * 63), dict(src=G), dict(lo=2.0),
                    dict(lo=float("nan")), dict(hi=float("nan")), dict(lo=float("-inf")), dict(hi=float("inf"))):
        refused("pxsom_clahe_quantize", invalid, but(good, order, **changes))
    refused("pxsom_clahe_quantize", unsupported, but(good, order, h=65536, w=65536, ld=65536, ldg=65536, gray=G + (1 << 44)))
    refused("pxsom_clahe_quantize", unsupported, but(good, order, h=4 * 65535 + 1, w=2, ld=2, ldg=2, gray=G + (1 << 44)))

    order = ("plane", "h", "w", "ld", "divisor", "out", "ldo", "stream")
    good = [S, 8, 8, 8, 2.0, O, 8, None]
    for changes in (dict(plane=None), dict(out=None), dict(h=1), dict(w=1), dict(ld=7), dict(ldo=7), dict(plane=S + 4), dict(out=O + 4),
                    dict(divisor=0.0), dict(divisor=float("nan")), dict(divisor=float("inf")), dict(out=S + 8),
                    dict(out=S, ldo=9)):
        refused("pxsom_plane_divide", invalid, but(good, order, **changes))
    refused("pxsom_plane_divide", unsupported, but(good, order, h=65536, w=65536, ld=65536, ldo=65536, out=O + (1 << 44)))

    order = ("gray", "h", "w", "ld", "k", "clim", "map_scale", "out", "ldo", "maps", "raw", "ldr", "ws", "wsb", "stream")
    good = [G, 8, 8, 8, 4, 1, 16383 / 16, O, 8, M, R, 8, W, need, None]
    for changes in (dict(gray=None), dict(out=None), dict(ws=None), dict(h=1), dict(w=1), dict(ld=7), dict(ldo=7), dict(ldr=7),
                    dict(gray=G + 1), dict(out=O + 4), dict(maps=M + 2), dict(raw=R + 1), dict(ws=W + 8), dict(k=0), dict(k=-1),
                    dict(k=9), dict(clim=0), dict(clim=-5), dict(map_scale=0.0), dict(map_scale=-1.0),
                    dict(map_scale=float("nan")), dict(map_scale=float("inf")), dict(wsb=need - 1), dict(wsb=0),
                    dict(raw=G), dict(maps=G), dict(raw=M + 2 * 1000), dict(out=W), dict(ws=O - 16, out=O),
                    dict(gray=M, maps=M), dict(raw=W + 16)):
        refused("pxsom_clahe_equalize", invalid, but(good, order, **changes))
    refused("pxsom_clahe_equalize", invalid, but(good, order, w=12, k=9, ld=12, ldo=12, ldr=12))        # k > min(h, w)
    far = 1 << 44
    refused("pxsom_clahe_equalize", unsupported, but(good, order, h=65536, w=65536, ld=65536, ldo=65536, ldr=65536, k=8,
                                                     gray=G + far, out=O + 2 * far, maps=None, raw=None))
    for a in (src, out, gray, raw, maps, ws):
        assert not a.any()
    # NULL maps_out / raw_out are allowed: the refusal below is the workspace's, not theirs
    refused("pxsom_clahe_equalize", invalid, but(good, order, maps=None, raw=None, wsb=need - 1))


def test_the_kernel_unit_states_the_statement_constants():
    src = open(os.path.join(ROOT, "ark_analysis_amd", "csrc", "pxsom_clahe.hip")).read()
    assert "kBins = 256" in src and "kBinSize = 65" in src and "16383.0" in src and "fp contract(off)" in src
    kernels = src.split("namespace {", 1)[1].split("#pragma clang fp contract(fast)")[0]
    assert "asm" not in kernels and not re.search(r"\b(exp|pow|log|floor|ceil|round|fma|fmin|fmax)\(", kernels)


# ---- the reference's three entries still refuse as before ----------------------------------------------------------------------
def test_the_entries_still_refuse(tmp_path):
    assert fs._UNBUILT == ("the front half of fibre segmentation (equalize_adapthist, frangi, threshold_multiotsu, sobel, "
                           "watershed) is not implemented; from a segmented mask use fiber_objects, from saved "
                           "<fov>_fiber_labels.tiff files fiber_object_table_from_labels")
    with pytest.raises(NotImplementedError, match="segment_fibers: the front half of fibre segmentation"):
        fs.segment_fibers(None, "Collagen1", str(tmp_path), "fov1")
    (tmp_path / "data" / "fov1").mkdir(parents=True)
    image_io.write_image(str(tmp_path / "data" / "fov1" / "Collagen1.tiff"), np.zeros((4, 4), np.float32))
    with pytest.raises(NotImplementedError, match="run_fiber_segmentation: the front half"):
        fs.run_fiber_segmentation(str(tmp_path / "data"), "Collagen1", str(tmp_path))
    with pytest.raises(NotImplementedError, match="plot_fiber_segmentation_steps: the front half"):
        fs.plot_fiber_segmentation_steps(str(tmp_path / "data"), "fov1", "Collagen1")
    doc = fs.__doc__
    assert "Not built: ``watershed`` after the middle." in doc and "``equalize_adapthist`` before" not in doc
