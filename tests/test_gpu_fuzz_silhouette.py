"""Randomised sweep of K15 pxsom_silhouette (som_device.silhouette_samples / silhouette_scores) against the numpy statement
of tests/silhouette_reference.py within the derived bound (|delta s_i| <= 8 (n + d) 2^-53, |delta score| <= 9 (n + d) 2^-53):
n up to 800, d up to 64, k up to 32, up to 4 labelings per call, drawn at random (seeded).  Case i first takes value class
i % 4 -- small integers, frequencies, values spread over ten decades, heavy duplication -- then draws the rest, so every
class is visited equally.  No case is skipped.  ``PXSOM_FUZZ_SEED`` as in test_gpu_fuzz_parity.py; ``PXSOM_SILHOUETTE_CASES``
sets the number of cases.  The generator is device-free."""
import os

import numpy as np
import pytest

from tests import silhouette_reference as sr

CASES = int(os.environ.get("PXSOM_SILHOUETTE_CASES", "200"))
SEED = int(os.environ.get("PXSOM_FUZZ_SEED", "20261017"))
CLASSES = ["integers", "frequencies", "decades", "duplicates"]
EDGE_N = [2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 800]
EDGE_D = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 20, 31, 32, 33, 63, 64]


def gen_case(i, seed=SEED):
    """Case i: dict(x [n, d] float64, labelings [M, n] int64, n_clusters [M], cls)."""
    rs = np.random.RandomState((seed + 7919 * i) % (2 ** 32))
    cls = CLASSES[i % len(CLASSES)]
    n = int(rs.choice(EDGE_N)) if rs.randint(3) == 0 else int(rs.randint(2, 801) if rs.randint(4) == 0 else rs.randint(2, 300))
    d = int(rs.choice(EDGE_D)) if rs.randint(2) else int(rs.randint(1, 65))
    if cls == "integers":
        x = rs.poisson(rs.choice([0.3, 2.0, 9.0]), size=(n, d)).astype(np.float64)
    elif cls == "frequencies":
        counts = rs.poisson(2.0, size=(n, d)).astype(np.float64)
        total = counts.sum(axis=1, keepdims=True)
        x = np.where(total > 0, counts / np.where(total > 0, total, 1), 0.0)
    elif cls == "decades":
        x = rs.standard_normal((n, d)) * 10.0 ** rs.uniform(-5, 5, size=(n, 1))
    else:
        few = rs.standard_normal((int(rs.randint(1, 6)), d)) * 10.0 ** rs.randint(-3, 4)
        x = few[rs.randint(0, len(few), n)]
    labelings, ks = [], []
    for _ in range(int(rs.randint(1, 5))):
        k = int(rs.choice([2, 3, 5, 10, 31, 32])) if rs.randint(2) else int(rs.randint(2, 33))
        lab = rs.choice(k, n, p=rs.dirichlet(np.full(k, rs.choice([0.2, 1.0, 10.0]))))      # skewed to even shares
        if cls == "duplicates" and rs.randint(2):
            lab = np.unique(x, axis=0, return_inverse=True)[1].reshape(-1) % k              # the clusters ARE the rows
        labelings.append(lab.astype(np.int64))
        ks.append(k)
    return dict(x=np.ascontiguousarray(x), labelings=np.stack(labelings), n_clusters=ks, cls=cls)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(CASES))
def test_fuzz_silhouette(gpu, i):
    import torch
    from ark_analysis_amd import som_device
    c = gen_case(i)
    x, lab = torch.from_numpy(c["x"]).to(gpu), torch.from_numpy(c["labelings"]).to(gpu)
    samples = som_device.silhouette_samples(x, lab, c["n_clusters"]).cpu().numpy()
    scores = som_device.silhouette_scores(x, lab, c["n_clusters"]).cpu().numpy()
    n, d = c["x"].shape
    what = repr((c["cls"], n, d, c["n_clusters"]))
    want = sr.silhouette_samples_for(c["x"], c["labelings"], c["n_clusters"])
    assert not np.isnan(samples).any(), what
    assert np.abs(samples - want).max() <= sr.sample_bound(n, d), what
    assert max(abs(s - sr.score(w)) for s, w in zip(scores, want)) <= sr.score_bound(n, d), what
