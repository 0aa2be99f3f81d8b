"""Neighbour counts and k-means labels of the reference's ``ark.analysis.spatial_analysis_utils``.

``compute_neighbor_counts`` takes a FOV's centroids where the reference takes its distance matrix: the counts come from
one pxsom_neighbor_counts launch and the N x N matrix is never built.  Not mirrored: ``calc_dist_matrix``
and its ``.xr`` files (xarray is not a dependency here), the distance-feature columns
(``append_distance_features_to_dataset``; the cell-distance analysis is ``cell_neighborhood_stats``), the enrichment statistics
(``compute_close_cell_num``, ``calculate_enrichment_stats``) and everything that plots.

``compute_kmeans_inertia`` and ``compute_kmeans_silhouette`` are the reference's sweeps over k: by default the k-means fits
stay on the host (as in ``generate_cluster_labels``), the silhouette scores of every k come from one pxsom_silhouette call
 in place of one ``sklearn.metrics.silhouette_score`` per k.  They return a ``pandas.Series`` indexed by
``cluster_num`` where the reference returns an ``xarray.DataArray``.

With ``kmeans="device"`` the three functions take their fits from ``kmeans_fits_device``: every (k, restart) is one
problem of a single pxsom_kmeans_lloyd call, so the nine fits of a sweep, or the ten restarts of the
labelling, share every pass over the rows.  The inits are drawn on the host with ``sklearn.cluster.kmeans_plusplus``."""
import warnings

import numpy as np
import pandas as pd

_CELL_LABEL, _CELL_TYPE = "label", "cell_meta_cluster"


# ---- device entry point (the CPU tests swap it for the numpy statement of the same contract) ------------------------
def _neighbor_counts_device(xy: np.ndarray, types: np.ndarray, seg: np.ndarray, n_types: int, distlim,
                            self_neighbor: bool) -> np.ndarray:
    """som_device.neighbor_counts on host arrays: ``xy`` [n, 2] float64, ``types`` [n] in [0, n_types), ``seg`` [F + 1]
    offsets -> [n, n_types] int32 on the host."""
    import torch
    from .. import _capi, som_device
    dev = _capi.require_gpu()
    counts = som_device.neighbor_counts(
        torch.from_numpy(np.ascontiguousarray(xy, dtype=np.float64)).to(dev),
        torch.from_numpy(np.ascontiguousarray(types, dtype=np.int32)).to(dev),
        torch.from_numpy(np.ascontiguousarray(seg, dtype=np.int64)).to(dev), n_types, distlim, self_neighbor)
    return counts.cpu().numpy()


def _silhouette_device(x: np.ndarray, labelings: np.ndarray, n_clusters) -> np.ndarray:
    """som_device.silhouette_scores on host arrays: ``x`` [n, d] float64, ``labelings`` [M, n] with labeling m in
    [0, n_clusters[m]) -> [M] float64 on the host."""
    import torch
    from .. import _capi, som_device
    dev = _capi.require_gpu()
    scores = som_device.silhouette_scores(
        torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev),
        torch.from_numpy(np.ascontiguousarray(labelings, dtype=np.int32)).to(dev), [int(k) for k in n_clusters])
    return scores.cpu().numpy()


def _kmeans_lloyd_device(x: np.ndarray, inits, tol: float, max_iter: int):
    """som_device.kmeans_lloyd on host arrays: ``x`` [n, d] float64, ``inits`` a list of [k_p, d] float64 centres ->
    ``(labels [P, n] int32, centres list of [k_p, d], inertia [P], n_iter [P])`` on the host."""
    import torch
    from .. import _capi, som_device
    dev = _capi.require_gpu()
    labels, centres, inertia, n_iter = som_device.kmeans_lloyd(
        torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev),
        [np.ascontiguousarray(c, dtype=np.float64) for c in inits], tol, max_iter)
    return labels.cpu().numpy(), [c.cpu().numpy() for c in centres], inertia, n_iter


def _freqs(counts: np.ndarray) -> np.ndarray:
    """counts / row total, 0 where a cell has no neighbour (the reference's NaN -> 0)."""
    total = counts.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        freqs = counts / total
    freqs[np.isnan(freqs)] = 0
    return freqs


def compute_neighbor_counts(current_fov_neighborhood_data, centroids, distlim, self_neighbor=False,
                            cell_label_col=_CELL_LABEL, cluster_name_col=_CELL_TYPE):
    """Per cell of one FOV, how many cells of each phenotype lie within ``distlim`` (the cell itself counts only with
    ``self_neighbor``; so does any cell at float32 distance 0, as in the reference).

    ``centroids`` is the ``[n, 2]`` array of the rows' centroids, in the rows' order; the reference passes the FOV's
    distance matrix here and looks the rows up by ``cell_label_col``, which this signature keeps for compatibility and
    does not need.  The distances are the reference's: binary64 Euclidean, rounded to float32, compared with
    ``distlim`` as numpy compares a float32 array with it.

    Returns ``(counts, freqs)``: float64 frames on the input's index whose columns are the FOV's sorted phenotype
    names; ``freqs = counts / neighbours of the cell``, 0 for a cell without neighbours.
    """
    data = current_fov_neighborhood_data
    xy = np.asarray(centroids, dtype=np.float64).reshape(-1, 2)
    if xy.shape[0] != len(data):
        raise ValueError("centroids must hold one (row, column) pair per row of the table: got %d for %d rows"
                         % (xy.shape[0], len(data)))
    codes, names = pd.factorize(data[cluster_name_col].to_numpy(), sort=True)
    n_names = len(names)
    codes = np.where(codes < 0, n_names, codes)      # a missing phenotype has no column: counted apart, then dropped
    counts = _neighbor_counts_device(xy, codes, np.array([0, len(data)]), n_names + 1, distlim, bool(self_neighbor))
    counts = counts[:, :n_names].astype(np.float64)
    columns = pd.Index(names, dtype=object) if n_names else pd.Index([], dtype=object)
    index = data.index.copy()
    return (pd.DataFrame(counts, columns=columns, index=index),
            pd.DataFrame(_freqs(counts), columns=columns, index=index.copy()))


_KMEANS_CHOICES = ("host", "device")
_KMEANS_TOL, _KMEANS_MAX_ITER = 1e-4, 300        # scikit-learn's defaults, which the reference leaves alone


def _check_kmeans(kmeans):
    if kmeans not in _KMEANS_CHOICES:
        raise ValueError("kmeans must be 'host' or 'device', got %r" % (kmeans,))


class _DeviceFit:
    """What the sweeps read of a fitted ``KMeans``: ``labels_``, ``inertia_``, ``cluster_centers_``."""

    def __init__(self, labels, inertia, centres):
        self.labels_, self.inertia_, self.cluster_centers_ = labels, inertia, centres


def kmeans_fits_device(values, ks, seed=42, n_init="auto"):
    """One k-means fit of the rows of ``values`` per k of ``ks``, all of them in one device call (pxsom_kmeans_lloyd,
    DESIGN.md K19): every (k, restart) is one problem and the problems share each pass over the rows.

    As ``KMeans`` does, the columns are centred by their mean first and the mean is added back to the centres; the
    tolerance is ``1e-4 *`` the mean of the column variances and ``max_iter`` is 300.  The initial centres come from
    ``sklearn.cluster.kmeans_plusplus`` on the host, with one ``numpy.random.RandomState(seed)`` per k carried through
    that k's ``n_init`` draws (``"auto"``: one draw).  Per k the restart of lowest inertia is kept, the first on a tie.

    Returns a list with, per k, an object holding ``labels_`` ([n] int32, 0-based), ``inertia_`` and
    ``cluster_centers_`` ([k, d])."""
    from sklearn.cluster import kmeans_plusplus
    x = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
    if x.ndim != 2:
        raise ValueError("kmeans_fits_device: values must be a matrix, got shape %s" % (x.shape,))
    if not np.isfinite(x).all():
        raise ValueError("kmeans_fits_device: values hold NaN or infinite entries")
    ks = [int(k) for k in ks]
    restarts = 1 if isinstance(n_init, str) and n_init == "auto" else int(n_init)
    if restarts < 1:
        raise ValueError("kmeans_fits_device: n_init must be 'auto' or >= 1, got %r" % (n_init,))
    n = len(x)
    if n == 0 or not ks:
        return [_DeviceFit(np.zeros(0, np.int32), 0.0, np.zeros((k, x.shape[1]))) for k in ks]
    if max(ks) > n:
        raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, max(ks)))
    tol = _KMEANS_TOL * float(np.mean(np.var(x, axis=0)))
    mean = x.mean(axis=0)
    x = x - mean
    inits = []
    for k in ks:
        rs = np.random.RandomState(seed)
        for _ in range(restarts):
            inits.append(np.ascontiguousarray(kmeans_plusplus(x, k, random_state=rs)[0], dtype=np.float64))
    labels, centres, inertia, _ = _kmeans_lloyd_device(x, inits, tol, _KMEANS_MAX_ITER)
    fits = []
    for at in range(0, len(inits), restarts):
        best = at + int(np.argmin(inertia[at:at + restarts]))        # the first of equal minima
        fits.append(_DeviceFit(np.asarray(labels[best], dtype=np.int32), float(inertia[best]), centres[best] + mean))
    return fits


def generate_cluster_labels(neighbor_mat_data, cluster_num, seed=42, *, kmeans="host"):
    """k-means labels 1 .. ``cluster_num`` of the rows of ``neighbor_mat_data`` (scikit-learn ``KMeans`` with
    ``n_init=10`` and ``random_state=seed``, on the host).  The same data gives the same clusters on every run; which
    number a cluster gets depends on the scikit-learn build.

    ``kmeans="device"``: the ten restarts run as one ``kmeans_fits_device`` call instead."""
    _check_kmeans(kmeans)
    if kmeans == "device":
        return kmeans_fits_device(neighbor_mat_data, [cluster_num], seed, 10)[0].labels_ + 1
    from sklearn.cluster import KMeans
    fit = KMeans(n_clusters=cluster_num, random_state=seed, n_init=10).fit(neighbor_mat_data)
    return fit.labels_ + 1


def _sweep_series(values, min_k, max_k):
    return pd.Series(np.asarray(values, dtype=np.float64), index=pd.Index(np.arange(min_k, max_k + 1), name="cluster_num"))


def _kmeans_sweep(neighbor_mat_data, min_k, max_k, seed, kmeans="host"):
    """The reference's fit for every k of the sweep: ``KMeans(n_clusters=k, random_state=seed, n_init='auto')``, or with
    ``kmeans="device"`` the fits of one ``kmeans_fits_device`` call."""
    if kmeans == "device":
        return kmeans_fits_device(neighbor_mat_data, range(min_k, max_k + 1), seed, "auto")
    from sklearn.cluster import KMeans
    return [KMeans(n_clusters=k, random_state=seed, n_init="auto").fit(neighbor_mat_data) for k in range(min_k, max_k + 1)]


def compute_kmeans_inertia(neighbor_mat_data, min_k=2, max_k=10, seed=42, *, kmeans="host"):
    """The k-means inertia of the rows of ``neighbor_mat_data`` for every k of ``min_k .. max_k`` (fits on the host, or
    all of them in one device call with ``kmeans="device"``).

    Returns a float64 ``pandas.Series`` whose index, named ``cluster_num``, runs ``min_k .. max_k``."""
    _check_kmeans(kmeans)
    return _sweep_series([fit.inertia_ for fit in _kmeans_sweep(neighbor_mat_data, min_k, max_k, seed, kmeans)],
                         min_k, max_k)


def _subsample_clusters(sub_dat, subsample, seed):
    """The reference's per-cluster subsample of a frame with a ``cluster`` column: ``subsample`` rows of every cluster,
    with replacement where the cluster is smaller."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=(DeprecationWarning, FutureWarning))   # apply over the grouping column
        return sub_dat.groupby("cluster").apply(
            lambda x: x.sample(subsample, replace=len(x) < subsample, random_state=seed)).reset_index(drop=True)


def _encode_labels(labels, n_rows):
    """Labels as 0 .. k' - 1 in sorted order (sklearn's LabelEncoder) and k'; sklearn's error unless 2 <= k' <= n - 1."""
    uniques, codes = np.unique(np.asarray(labels), return_inverse=True)
    if not 1 < len(uniques) < n_rows:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % len(uniques))
    return codes.reshape(-1), len(uniques)


def compute_kmeans_silhouette(neighbor_mat_data, min_k=2, max_k=10, seed=42, subsample=None, *, kmeans="host"):
    """The silhouette score (Euclidean) of the k-means clusters of ``neighbor_mat_data`` for every k of
    ``min_k .. max_k``.  The fits run on the host (``kmeans="device"``: all of them in one ``kmeans_fits_device`` call);
    the scores of the whole sweep come from one device call
    (pxsom_silhouette), or from one call per k under ``subsample`` -- the number of rows drawn from every cluster
    (with replacement from a smaller one) before scoring, as in the reference.

    Returns a float64 ``pandas.Series`` whose index, named ``cluster_num``, runs ``min_k .. max_k``."""
    _check_kmeans(kmeans)
    values = np.asarray(neighbor_mat_data, dtype=np.float64)
    if not np.isfinite(values).all():
        raise ValueError("compute_kmeans_silhouette: neighbor_mat_data holds NaN or infinite values")
    fits = _kmeans_sweep(neighbor_mat_data, min_k, max_k, seed, kmeans)
    if subsample is None:
        encoded = [_encode_labels(fit.labels_, len(values)) for fit in fits]
        scores = _silhouette_device(values, np.stack([codes for codes, _ in encoded]), [k for _, k in encoded])
        return _sweep_series(scores, min_k, max_k)
    scores = []
    for fit in fits:
        sub_dat = neighbor_mat_data.copy()
        sub_dat["cluster"] = fit.labels_
        sub_dat = _subsample_clusters(sub_dat, subsample, seed)
        codes, k = _encode_labels(sub_dat["cluster"].to_numpy(), len(sub_dat))
        rows = sub_dat.drop("cluster", axis=1).to_numpy(dtype=np.float64)
        scores.append(_silhouette_device(rows, codes[None, :], [k])[0])
    return _sweep_series(scores, min_k, max_k)
