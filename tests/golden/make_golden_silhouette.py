#!/usr/bin/env python
"""Generates tests/golden/silhouette_sklearn.npz: sklearn.metrics.silhouette_samples (Euclidean; recorded from
scikit-learn 1.7.2) on three matrices of 700 rows and 7 columns, each under labelings with k = 2, 5 and 10:

  counts    integer neighbour counts (Poisson, rows without a neighbour redrawn), as create_neighborhood_matrix makes them:
            sklearn's ||x||^2 - 2 x.y + ||y||^2 is exact on them
  freqs     the same rows divided by their totals: the expansion cancels, and sklearn's answer is off by what
            tests/test_silhouette.py records
  distinct  integer rows drawn from a dozen distinct ones: most distances are exactly 0

The labelings are Voronoi cells of k rows of the matrix, found in integer arithmetic (ties to the first seed), so the
generator needs no k-means fit and gives the same labels on every machine; ``freqs`` takes the labels of ``counts``.

    python tests/golden/make_golden_silhouette.py      (needs scikit-learn)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed file.
"""
import os

import numpy as np
from sklearn.metrics import silhouette_samples

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.environ.get("PXSOM_GOLDEN_OUT", HERE)
N, D, KS = 700, 7, (2, 5, 10)
INPUTS = ("counts", "freqs", "distinct")


def voronoi_labels(rows, k, rs):
    """The cell of the nearest of k distinct rows (squared distances in int64: exact), ties to the first."""
    rows = rows.astype(np.int64)
    distinct = np.unique(rows, axis=0)
    seeds = distinct[rs.choice(len(distinct), k, replace=False)]
    d2 = ((rows[:, None, :] - seeds[None, :, :]) ** 2).sum(axis=2)
    return d2.argmin(axis=1).astype(np.int32)


def main():
    rs = np.random.RandomState(15)
    counts = rs.poisson(rs.choice([0.3, 2.0, 6.0], size=(N, D))).astype(np.float64)
    while (counts.sum(axis=1) == 0).any():
        empty = counts.sum(axis=1) == 0
        counts[empty] = rs.poisson(2.0, size=(int(empty.sum()), D))
    freqs = counts / counts.sum(axis=1, keepdims=True)
    dozen = rs.randint(0, 9, size=(12, D)).astype(np.float64)
    distinct = dozen[rs.randint(0, 12, size=N)]
    out = {"ks": np.array(KS), "counts_x": counts, "freqs_x": freqs, "distinct_x": distinct}
    for k in KS:
        out["counts_labels_k%d" % k] = out["freqs_labels_k%d" % k] = voronoi_labels(counts, k, rs)
        out["distinct_labels_k%d" % k] = voronoi_labels(distinct, k, rs)
        for name in INPUTS:
            out["%s_samples_k%d" % (name, k)] = silhouette_samples(out[name + "_x"], out["%s_labels_k%d" % (name, k)],
                                                                   metric="euclidean")
    path = os.path.join(OUT_DIR, "silhouette_sklearn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
