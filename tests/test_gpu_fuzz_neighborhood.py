"""Randomised parity sweep of K13 pxsom_neighbor_counts (som_device.neighbor_counts) against the numpy statement of
tests/neighborhood_reference.py: FOV sizes, number of FOVs (empty ones among them), number of types, distlim, the scalar
type distlim arrives in (Python int, Python float, np.float32, np.float64 -- numpy compares the float32 distances in
float32 for the first three and in float64 for the last) and a coordinate scale from 1e-3 to 1e6, drawn at random
(seeded).  Case i first takes class i % R from a fixed list, then draws the rest within that class, so the default 12
cases visit every class.  Equality is exact.  ``PXSOM_FUZZ_CASES`` / ``PXSOM_FUZZ_SEED`` as in test_gpu_fuzz_parity.py.
The generator is device-free (tests/test_neighborhood.py checks it on CPU)."""
import os

import numpy as np
import pytest

from tests import neighborhood_reference as nr

CASES = int(os.environ.get("PXSOM_FUZZ_CASES", "12"))
SEED = int(os.environ.get("PXSOM_FUZZ_SEED", "20261016"))

# (scalar type of distlim, coordinate scale, layout)
CLASSES = [("int", 1.0, "uniform"), ("float", 1e-3, "uniform"), ("f32", 1e3, "lattice"), ("f64", 1.0, "lattice"),
           ("float", 1e6, "uniform"), ("f64", 1e-3, "clumps"), ("int", 1e3, "clumps"), ("f32", 1.0, "rational"),
           ("f64", 1e6, "rational"), ("float", 1.0, "tiny_fovs"), ("int", 1.0, "one_big"), ("f32", 1e-3, "lattice")]
SCALAR = {"int": int, "float": float, "f32": np.float32, "f64": np.float64}


def gen_case(i, seed=SEED):
    """Case i: dict(xy [n, 2] float64, types [n] int64, seg [F + 1] int64, n_types, distlim, self_neighbor, cls)."""
    rs = np.random.RandomState((seed + 7919 * i) % (2 ** 32))
    kind, scale, layout = CLASSES[i % len(CLASSES)]
    n_types = int(rs.choice([1, 2, 3, 5, 8, 20, 64, 150]))
    if layout == "tiny_fovs":
        sizes = rs.randint(0, 6, size=rs.randint(200, 600)).tolist()
    elif layout == "one_big":
        sizes = [int(rs.randint(2000, 4000))]
    else:
        sizes = [int(rs.choice([0, 1, 2, 63, 64, 65, 255, 256, 257, rs.randint(3, 1500)])) for _ in range(rs.randint(1, 7))]
    base = float(rs.choice([3, 10, 37.5, 50, 100.25]))         # distlim in units of `scale`
    xy = []
    for m in sizes:
        side = max(np.sqrt(m * np.pi * base ** 2 / rs.uniform(2, 30)), base / 4)
        if layout == "lattice":          # an integer lattice whose pitch divides distlim: many pairs at exactly distlim
            pitch = base / rs.choice([2, 5, 10]) if float(base).is_integer() else base / 3
            cols = max(int(np.ceil(np.sqrt(max(m, 1)))), 1)
            idx = rs.permutation(cols * cols)[:m]
            pts = np.stack([idx // cols, idx % cols], 1) * pitch
        elif layout == "clumps":         # groups of coincident cells
            centres = rs.uniform(0, side, (max(m // 8, 1), 2))
            pts = centres[rs.randint(0, len(centres), m)]
        elif layout == "rational":       # centroids as the cell table makes them: sum / count
            pts = rs.randint(0, int(side * 40) + 1, (m, 2)) / rs.randint(20, 80, (m, 1))
        else:
            pts = rs.uniform(0, side, (m, 2))
        xy.append(np.asarray(pts, dtype=np.float64).reshape(m, 2) * scale)
    distlim = base * scale
    if kind == "int":
        distlim = int(distlim) if float(distlim).is_integer() and distlim >= 1 else int(np.ceil(distlim))
    distlim = SCALAR[kind](distlim)
    n = int(sum(sizes))
    return dict(xy=np.concatenate(xy).reshape(n, 2) if xy else np.zeros((0, 2)),
                types=rs.randint(0, n_types, n).astype(np.int64),
                seg=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), n_types=n_types, distlim=distlim,
                self_neighbor=bool(rs.randint(2)), cls=(kind, scale, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(CASES))
def test_fuzz_neighbor_counts(gpu, i):
    import torch
    from ark_analysis_amd import som_device
    c = gen_case(i)
    got = som_device.neighbor_counts(torch.from_numpy(c["xy"]).to(gpu), torch.from_numpy(c["types"]).to(gpu),
                                     torch.from_numpy(c["seg"]).to(gpu), c["n_types"], c["distlim"], c["self_neighbor"])
    torch.cuda.synchronize()
    want = nr.neighbor_counts(c["xy"], c["types"], c["seg"], c["n_types"], c["distlim"], c["self_neighbor"])
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (c["cls"], c["distlim"], len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
