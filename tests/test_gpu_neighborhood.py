"""pxsom_neighbor_counts on the GPU against the numpy statement of tests/neighborhood_reference.py (exact integer
equality: no tolerance), create_neighborhood_matrix on the HIP path against the g18 fixture of the reference, and the
chain cell table -> neighbourhood matrix -> k-means -> neighbourhood masks end to end."""
import os
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from tests import neighborhood_reference as nr
from tests import test_neighborhood as tn

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 257, 1000, 5000]
TYPE_COUNTS = [1, 2, 7, 33, 200]


def _cohort(rs, sizes, n_types, density=12.0, distlim=50.0):
    """FOVs of the given sizes on square fields sized for about ``density`` neighbours within distlim; a few cells sit on
    another cell's centroid, and every type is drawn (so some are absent from small FOVs)."""
    xy, types = [], []
    for m in sizes:
        side = max(np.sqrt(m * np.pi * distlim ** 2 / density), 1.0)
        pts = rs.uniform(0, side, (m, 2))
        if m >= 2:
            dup = rs.randint(0, m, size=max(1, m // 50))
            pts[dup] = pts[rs.randint(0, m, size=dup.size)]
        xy.append(pts)
        types.append(rs.randint(0, n_types, m))
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(xy).reshape(-1, 2), np.concatenate(types).astype(np.int64), seg


def _device(gpu, xy, types, seg, n_types, distlim, self_neighbor, type_dtype=torch.int64):
    from ark_analysis_amd import som_device
    got = som_device.neighbor_counts(torch.from_numpy(np.ascontiguousarray(xy)).to(gpu),
                                     torch.from_numpy(types).to(gpu).to(type_dtype), torch.from_numpy(seg).to(gpu),
                                     n_types, distlim, self_neighbor)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(xy), n_types)
    return got.cpu().numpy()


def _same(got, want):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("n_types", TYPE_COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_statement(gpu, n, n_types):
    """Several FOVs in one call -- n cells, an empty one, a small one, n again (one FOV of 5 000 plus a small one at the
    largest size) -- with both self_neighbor values, rows in random type order."""
    rs = np.random.RandomState(1000 * n + n_types)
    sizes = [n, 0, 300] if n >= 5000 else [n, 0, min(n, 37) + 3, n]
    xy, types, seg = _cohort(rs, sizes, n_types)
    for self_neighbor in (False, True):
        got = _device(gpu, xy, types, seg, n_types, 50, self_neighbor,
                      torch.int32 if n_types % 2 else torch.int64)
        _same(got, nr.neighbor_counts(xy, types, seg, n_types, 50, self_neighbor))


def test_only_empty_fovs_and_no_cells(gpu):
    xy, types = np.zeros((0, 2)), np.zeros(0, dtype=np.int64)
    for seg in (np.array([0]), np.array([0, 0, 0])):
        assert _device(gpu, xy, types, seg.astype(np.int64), 4, 50, False).shape == (0, 4)


def test_exact_tie_grid(gpu):
    """The 20 x 20 grid of pitch 10: the 3 376 ordered pairs at exactly 50 are excluded at distlim 50 and included one
    float32 above it."""
    gy, gx = np.mgrid[0:20, 0:20]
    xy = np.stack([gy.ravel(), gx.ravel()], 1).astype(np.float64) * 10
    rs = np.random.RandomState(3)
    types = rs.randint(0, 3, len(xy)).astype(np.int64)
    seg = np.array([0, len(xy)], dtype=np.int64)
    above = float(np.nextafter(np.float32(50), np.float32(60)))
    totals = {}
    for distlim in (50, above, np.float64(50), 50.0):
        got = _device(gpu, xy, types, seg, 3, distlim, False)
        _same(got, nr.neighbor_counts(xy, types, seg, 3, distlim, False))
        totals[distlim] = int(got.sum())
    assert totals[above] - totals[50] == 3376


def test_coincident_cells(gpu):
    """130 cells on one point, 70 on another 10 away: at float32 distance 0 a cell is a neighbour only with
    self_neighbor."""
    rs = np.random.RandomState(4)
    xy = np.concatenate([np.tile([[1 / 3, 2 / 7]], (130, 1)), np.tile([[1 / 3, 2 / 7 + 10]], (70, 1))])
    types = rs.randint(0, 5, 200).astype(np.int64)
    seg = np.array([0, 200], dtype=np.int64)
    hist = lambda t: np.bincount(t, minlength=5)      # noqa: E731
    for self_neighbor in (False, True):
        got = _device(gpu, xy, types, seg, 5, 50, self_neighbor)
        _same(got, nr.neighbor_counts(xy, types, seg, 5, 50, self_neighbor))
        want = np.empty((200, 5), dtype=np.int64)
        want[:130] = hist(types[130:]) + (hist(types[:130]) if self_neighbor else 0)
        want[130:] = hist(types[:130]) + (hist(types[130:]) if self_neighbor else 0)
        _same(got, want)


def test_rows_keep_the_callers_order(gpu):
    """Permuting the cells inside each FOV permutes the rows of the result and nothing else."""
    rs = np.random.RandomState(5)
    sizes = [700, 0, 129, 300]
    xy, types, seg = _cohort(rs, sizes, 11)
    base = _device(gpu, xy, types, seg, 11, 37.5, False)
    perm = np.concatenate([a + rs.permutation(b - a) for a, b in zip(seg[:-1], seg[1:])]).astype(np.int64)
    _same(_device(gpu, xy[perm], types[perm], seg, 11, 37.5, False), base[perm])
    by_type = np.concatenate([a + np.argsort(types[a:b], kind="stable") for a, b in zip(seg[:-1], seg[1:])]).astype(np.int64)
    _same(_device(gpu, xy[by_type], types[by_type], seg, 11, 37.5, False), base[by_type])


def test_raw_call_writes_every_entry_and_nothing_else(gpu):
    """The C entry on rows already sorted by type, into a slice of a buffer filled with a sentinel: every entry of the
    slice is written (absent types and rows of no FOV as zeros), nothing outside it."""
    from ark_analysis_amd import _capi, som_device
    rs = np.random.RandomState(6)
    n_types = 9
    xy, types, seg = _cohort(rs, [300, 0, 70, 515], n_types)
    types[types == 4] = 5                       # a type no cell has
    types[seg[2]:seg[3]] = 7                    # a FOV of one type
    order = np.concatenate([a + np.argsort(types[a:b], kind="stable") for a, b in zip(seg[:-1], seg[1:])])
    xy, types = xy[order], types[order]
    n = len(xy)
    s_lim, s_zero = som_device.neighbor_thresholds(50)
    guard = 1024
    sentinel = 0x5A5A5A5A
    for self_neighbor in (0, 1):
        buf = torch.full((guard + n * n_types + guard,), sentinel, dtype=torch.int32, device=gpu)
        xy_d, ty_d = torch.from_numpy(xy).to(gpu), torch.from_numpy(types.astype(np.int32)).to(gpu)
        seg_d = torch.from_numpy(seg).to(gpu)
        rc = _capi.lib().pxsom_neighbor_counts(xy_d.data_ptr(), ty_d.data_ptr(), seg_d.data_ptr(), len(seg) - 1, n,
                                               n_types, s_lim, s_zero, self_neighbor,
                                               buf.data_ptr() + guard * 4, _capi.stream_ptr())
        _capi.check(rc, "pxsom_neighbor_counts")
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:guard] == sentinel).all() and (host[guard + n * n_types:] == sentinel).all()
        got = host[guard:guard + n * n_types].reshape(n, n_types)
        _same(got, nr.neighbor_counts(xy, types, seg, n_types, 50, bool(self_neighbor)))
        assert (got[:, 4] == 0).all()


def test_wrapper_argument_errors(gpu):
    from ark_analysis_amd import som_device
    xy = torch.zeros((4, 2), dtype=torch.float64, device=gpu)
    ty = torch.zeros(4, dtype=torch.int64, device=gpu)
    seg = torch.tensor([0, 4], device=gpu)
    with pytest.raises(ValueError, match="float64"):
        som_device.neighbor_counts(xy.float(), ty, seg, 2, 50)
    with pytest.raises(ValueError, match="n_types"):
        som_device.neighbor_counts(xy, ty + 2, seg, 2, 50)
    with pytest.raises(ValueError, match="offsets"):
        som_device.neighbor_counts(xy, ty, torch.tensor([0, 3], device=gpu), 2, 50)
    with pytest.raises(ValueError, match="offsets"):
        som_device.neighbor_counts(xy, ty, torch.tensor([0, 5, 4], device=gpu), 2, 50)


def test_create_neighborhood_matrix_hip_equals_fixture(gpu):
    tn.check_fixture_cases()


def test_compute_neighbor_counts_hip(gpu):
    tn.check_per_fov_function()


def test_cluster_matrix_results_hip_with_injected_labels(gpu, monkeypatch):
    tn.check_cluster_matrix_results(monkeypatch.setattr)


def test_neighborhood_masks_end_to_end(gpu, tmp_path):
    """Cell table -> create_neighborhood_matrix -> generate_cluster_matrix_results (k-means on the host) ->
    generate_and_save_neighborhood_cluster_masks: every cell's pixels hold its k-means neighbourhood, cells the analysis
    dropped hold the unassigned id, background stays 0."""
    from ark_analysis_amd import image_io
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from ark_analysis_amd.utils import data_utils
    from tests import cell_table_reference as ctr
    rs = np.random.RandomState(7)
    seg_dir, fovs, frames, segs = os.path.join(str(tmp_path), "seg"), ["fov0", "fov1"], [], {}
    os.makedirs(seg_dir)
    for i, fov in enumerate(fovs):
        seg = ctr.voronoi_labels(96, 128, 60, seed=i + 1)
        segs[fov] = seg
        image_io.write_image(os.path.join(seg_dir, fov + "_whole_cell.tiff"), seg)
        labels = np.unique(seg[seg > 0])
        cen = np.array([np.argwhere(seg == lab).mean(axis=0) for lab in labels])
        frames.append(pd.DataFrame({"cell_size": [int((seg == lab).sum()) for lab in labels],
                                    "chan0": rs.rand(len(labels)), "chan1": rs.rand(len(labels)), "label": labels,
                                    "fov": fov, "centroid-0": cen[:, 0], "centroid-1": cen[:, 1],
                                    "cell_meta_cluster": rs.choice(["a", "b", "c"], len(labels))}))
    table = pd.concat(frames, ignore_index=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        counts, _ = na.create_neighborhood_matrix(table, distlim=14)
    assert 0 < len(counts) < len(table)             # some cells have no neighbour that close
    k = 3
    cells, per_type, means = na.generate_cluster_matrix_results(table, counts, k)
    assert set(cells["kmeans_neighborhood"]) == set(range(1, k + 1)) and len(cells) == len(counts)
    assert per_type.to_numpy().sum() == len(cells) and list(means.columns) == ["chan0", "chan1"]
    data_utils.generate_and_save_neighborhood_cluster_masks(fovs, str(tmp_path), seg_dir, cells,
                                                            name_suffix="_neighborhood_mask")
    for fov in fovs:
        mask = image_io.read_image(os.path.join(str(tmp_path), fov + "_neighborhood_mask.tiff"))
        rows = cells[cells["fov"] == fov]
        lut = np.full(int(segs[fov].max()) + 1, k + 1, dtype=np.int16)
        lut[0] = 0
        lut[rows["label"].to_numpy()] = rows["kmeans_neighborhood"].to_numpy()
        assert mask.dtype == np.int16 and np.array_equal(mask, lut[segs[fov]])
