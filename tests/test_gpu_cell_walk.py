"""The three kernels over one FOV walk (pxsom_fovwalk.h: K13 neighbour counts, K14 nearest-cell means, K20 close-pair
counts) held to one another on the GPU, exactly: none of them can drift from the shared pair test and walk alone.  The
numpy statements stay the oracle of each kernel in its own tests."""
import numpy as np
import pytest
import torch

from tests.test_gpu_close_pairs import _points

pytestmark = pytest.mark.gpu

FOV_SIZES = [1, 63, 64, 65, 0, 257, 513]    # 963 cells, four workgroups: FOVs begin and end inside blocks, one is
N_TYPES, DISTLIM = 3, 50                     # empty, one spans three tiles


@pytest.fixture(scope="module")
def cells(gpu):
    rs = np.random.RandomState(963)
    xy, seg = _points(rs, FOV_SIZES, distlim=float(DISTLIM))
    types = rs.randint(0, N_TYPES, size=len(xy))
    assert len(xy) == 963 and all((types == t).any() for t in range(N_TYPES))
    return (torch.from_numpy(xy).to(gpu), torch.from_numpy(types).to(gpu), torch.from_numpy(seg).to(gpu), types, seg)


@pytest.mark.parametrize("self_neighbor", [False, True])
def test_close_pairs_of_one_hot_sets_are_the_neighbour_counts_summed(cells, self_neighbor):
    from ark_analysis_amd import som_device
    xy_d, types_d, seg_d, types, seg = cells
    counts = som_device.neighbor_counts(xy_d, types_d, seg_d, N_TYPES, DISTLIM, self_neighbor).cpu().numpy()
    one_hot = torch.ones_like(types_d) << types_d
    pairs = som_device.close_pair_counts(xy_d, one_hot, one_hot, seg_d, N_TYPES, N_TYPES, DISTLIM,
                                         self_neighbor).cpu().numpy()
    want = np.zeros((len(FOV_SIZES), N_TYPES, N_TYPES), dtype=np.int64)
    for f in range(len(FOV_SIZES)):
        rows = slice(seg[f], seg[f + 1])
        for s in range(N_TYPES):
            want[f, s] = counts[rows][types[rows] == s].sum(axis=0, dtype=np.int64)
    assert want.sum() > 0 and np.array_equal(pairs, want)


def test_a_nearest_cell_exists_where_a_neighbour_at_any_distance_is_counted(cells):
    from ark_analysis_amd import som_device
    xy_d, types_d, seg_d, _, _ = cells
    means = som_device.nearest_type_means(xy_d, types_d, seg_d, N_TYPES, 1).cpu().numpy()
    counts = som_device.neighbor_counts(xy_d, types_d, seg_d, N_TYPES, 1e9, False).cpu().numpy()
    finite = np.isfinite(means)
    assert finite.any() and not finite.all() and np.array_equal(finite, counts >= 1)
