"""Randomised parity sweep of K14 pxsom_nearest_type_means (som_device.nearest_type_means) against the numpy statement of
tests/cell_distance_reference.py: FOV sizes, number of FOVs (empty ones among them), number of types and how skewed their
shares are, k from 1 to 32, duplicated centroids and a coordinate scale from 1e-3 to 1e6, drawn at random (seeded).  Case i
first takes class i % R from a fixed list, then draws the rest within that class, so the default 12 cases visit every
class.  Equality is exact: float32 bit patterns, NaN in the same places; no case is skipped or tolerated.
``PXSOM_FUZZ_CASES`` / ``PXSOM_FUZZ_SEED`` as in test_gpu_fuzz_parity.py.  The generator is device-free
(tests/test_cell_distances.py checks it on CPU)."""
import os

import numpy as np
import pytest

from tests import cell_distance_reference as cr

CASES = int(os.environ.get("PXSOM_FUZZ_CASES", "12"))
SEED = int(os.environ.get("PXSOM_FUZZ_SEED", "20261017"))

# (k range, coordinate scale, layout)
CLASSES = [((1, 7), 1.0, "uniform"), ((8, 16), 1e-3, "uniform"), ((17, 32), 1e3, "lattice"), ((1, 32), 1.0, "lattice"),
           ((8, 8), 1e6, "uniform"), ((1, 7), 1e-3, "clumps"), ((9, 24), 1e3, "clumps"), ((1, 32), 1.0, "rational"),
           ((16, 17), 1e6, "rational"), ((1, 3), 1.0, "tiny_fovs"), ((1, 32), 1.0, "one_big"), ((32, 32), 1e-3, "lattice")]


def gen_case(i, seed=SEED):
    """Case i: dict(xy [n, 2] float64, types [n] int64, seg [F + 1] int64, n_types, k, cls)."""
    rs = np.random.RandomState((seed + 7919 * i) % (2 ** 32))
    (k_lo, k_hi), scale, layout = CLASSES[i % len(CLASSES)]
    k = int(rs.randint(k_lo, k_hi + 1))
    n_types = int(rs.choice([1, 2, 3, 5, 8, 20, 64]))
    if layout == "tiny_fovs":
        sizes = rs.randint(0, 9, size=rs.randint(200, 600)).tolist()
    elif layout == "one_big":
        sizes = [int(rs.randint(2000, 4000))]
    else:
        sizes = [int(rs.choice([0, 1, 2, 63, 64, 65, 255, 256, 257, rs.randint(3, 1500)])) for _ in range(rs.randint(1, 7))]
    share = rs.dirichlet(np.full(n_types, rs.choice([0.3, 1.0, 10.0])))          # skewed to even type shares
    xy = []
    for m in sizes:
        side = max(30.0 * np.sqrt(m), 8.0)
        if layout == "lattice":          # an integer lattice: every distance tied many times over
            cols = max(int(np.ceil(np.sqrt(max(m, 1)))), 1)
            idx = rs.permutation(cols * cols)[:m]
            pts = np.stack([idx // cols, idx % cols], 1) * float(rs.choice([1, 3, 10]))
        elif layout == "clumps":         # groups of coincident cells
            centres = rs.uniform(0, side, (max(m // 8, 1), 2))
            pts = centres[rs.randint(0, len(centres), m)]
        elif layout == "rational":       # centroids as the cell table makes them: sum / count
            pts = rs.randint(0, int(side * 40) + 1, (m, 2)) / rs.randint(20, 80, (m, 1))
        else:
            pts = rs.uniform(0, side, (m, 2))
            if m >= 2 and rs.randint(2):
                dup = rs.randint(0, m, size=max(1, m // 20))
                pts[dup] = pts[rs.randint(0, m, size=dup.size)]
        xy.append(np.asarray(pts, dtype=np.float64).reshape(m, 2) * scale)
    n = int(sum(sizes))
    return dict(xy=np.concatenate(xy).reshape(n, 2) if xy else np.zeros((0, 2)),
                types=rs.choice(n_types, n, p=share).astype(np.int64),
                seg=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), n_types=n_types, k=k,
                cls=((k_lo, k_hi), scale, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(CASES))
def test_fuzz_nearest_type_means(gpu, i):
    import torch
    from ark_analysis_amd import som_device
    from tests.test_cell_distances import assert_same_float32
    c = gen_case(i)
    got = som_device.nearest_type_means(torch.from_numpy(c["xy"]).to(gpu), torch.from_numpy(c["types"]).to(gpu),
                                        torch.from_numpy(c["seg"]).to(gpu), c["n_types"], c["k"])
    torch.cuda.synchronize()
    want = cr.nearest_type_means(c["xy"], c["types"], c["seg"], c["n_types"], c["k"])
    assert_same_float32(got.cpu().numpy(), want, repr((c["cls"], c["k"], c["n_types"])))
