"""The numpy statement of pxsom_silhouette: Euclidean distances in the direct form in binary64
(differences, squares, a sum, the square root), per-cluster sums with math.fsum (correctly rounded, so the statement's own
summation error is one rounding), then sklearn's silhouette_samples rules.  Test infrastructure: the product never
imports this file."""
import math

import numpy as np

U = 2.0 ** -53


def sample_bound(n, d):
    """|device sample - statement sample|: both compute a distance within (d + 3) u, a sum of n of them in any order adds
    (n - 1) u, a, b and the quotient a few more, and |s| <= 1."""
    return 8 * (n + d) * U


def score_bound(n, d):
    return 9 * (n + d) * U


def cluster_sums(x, labels, k):
    """S [n, k]: S[i, c] = the sum of the distances from row i to the rows of cluster c."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    labels = np.asarray(labels).astype(np.int64)
    n = len(x)
    order = np.argsort(labels, kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=k))])
    xs = x[order]
    out = np.zeros((n, k))
    for i in range(n):
        diff = xs - x[i]
        dist = np.sqrt((diff * diff).sum(axis=1)).tolist()
        for c in range(k):
            out[i, c] = math.fsum(dist[seg[c]:seg[c + 1]])
    return out


def samples_from_sums(sums, labels, k):
    labels = np.asarray(labels).astype(np.int64)
    n = len(labels)
    counts = np.bincount(labels, minlength=k)
    rows = np.arange(n)
    own = counts[labels]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = sums[rows, labels] / (own - 1)
        means = sums / counts[None, :]
        means[:, counts == 0] = np.inf
        means[rows, labels] = np.inf
        b = means.min(axis=1)
        s = (b - a) / np.maximum(a, b)
    s[own == 1] = 0.0
    s[np.isnan(s)] = 0.0
    return s


def silhouette_samples(x, labels, k):
    return samples_from_sums(cluster_sums(x, labels, k), labels, k)


def silhouette_samples_for(x, labelings, n_clusters):
    """[M, n] samples of M labelings over one pass through the distances."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    labelings = [np.asarray(lab).astype(np.int64) for lab in labelings]
    n = len(x)
    plans = []
    for lab, k in zip(labelings, n_clusters):
        plans.append((np.argsort(lab, kind="stable"), np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=k))]),
                      np.zeros((n, k))))
    for i in range(n):
        diff = x - x[i]
        dist = np.sqrt((diff * diff).sum(axis=1))
        for order, seg, out in plans:
            ds = dist[order].tolist()
            for c in range(out.shape[1]):
                out[i, c] = math.fsum(ds[seg[c]:seg[c + 1]])
    return np.stack([samples_from_sums(out, lab, k) for (_, _, out), lab, k in zip(plans, labelings, n_clusters)])


def score(samples):
    return math.fsum(np.asarray(samples).tolist()) / len(samples)


def host_stand_in(x, labelings, n_clusters):
    """spatial_analysis_utils._silhouette_device's contract on the host: [M] scores."""
    labelings = np.asarray(labelings)
    assert labelings.ndim == 2 and labelings.shape[1] == len(x) and len(n_clusters) == len(labelings)
    for lab, k in zip(labelings, n_clusters):
        assert lab.min() >= 0 and lab.max() < k
    return np.array([score(s) for s in silhouette_samples_for(x, labelings, n_clusters)], dtype=np.float64)
