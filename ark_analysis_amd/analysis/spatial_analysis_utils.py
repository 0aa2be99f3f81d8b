"""Neighbour counts, close-pair counts and k-means labels of the reference's ``ark.analysis.spatial_analysis_utils``.

``compute_neighbor_counts`` takes a FOV's centroids where the reference takes its distance matrix: the counts come from
one pxsom_neighbor_counts launch and the N x N matrix is never built.  ``compute_close_cell_num`` -- the
primitive under the enrichment statistics -- does the same: the cells positive for each marker, or of each phenotype,
are sets, a set is one bit of a 64-bit mask per cell, and the marker x marker table of close pairs is one
pxsom_close_pair_counts launch (more than 64 sets go through blocks of 64 x 64).
``get_pos_cell_labels_channel`` and ``get_pos_cell_labels_cluster`` are the reference's.  Not mirrored:
``calc_dist_matrix`` and its ``.xr`` files (xarray is not a dependency here), the distance-feature columns
(``append_distance_features_to_dataset``; the cell-distance analysis is ``cell_neighborhood_stats``), the bootstrap and
z-scores over ``compute_close_cell_num`` (``calculate_enrichment_stats``) and everything that plots.

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

from ..host_utils import verify_in_list
from ._cells import _to_device

_CELL_LABEL, _CELL_TYPE, _CELL_TYPE_NUM = "label", "cell_meta_cluster", "cell_meta_cluster_id"
_MASK_BITS = 64         # sets per pxsom_close_pair_counts launch: a set is a bit of a uint64 mask


# ---- device entry point (the CPU tests swap it for the numpy statement of the same contract) ------------------------
def _neighbor_counts_device(xy: np.ndarray, types: np.ndarray, seg: np.ndarray, n_types: int, distlim,
                            self_neighbor: bool) -> np.ndarray:
    """som_device.neighbor_counts on host arrays: ``xy`` [n, 2] float64, ``types`` [n] in [0, n_types), ``seg`` [F + 1]
    offsets -> [n, n_types] int32 on the host."""
    from .. import som_device
    xy, types, seg = _to_device(xy, np.float64), _to_device(types, np.int32), _to_device(seg, np.int64)
    return som_device.neighbor_counts(xy, types, seg, n_types, distlim, self_neighbor).cpu().numpy()


def _close_pair_counts_device(xy: np.ndarray, member_q: np.ndarray, member_c: np.ndarray, seg: np.ndarray, n_sets_q: int,
                              n_sets_c: int, distlim, self_neighbor: bool) -> np.ndarray:
    """som_device.close_pair_counts on host arrays: ``xy`` [n, 2] float64, ``member_q`` / ``member_c`` [n] uint64 masks,
    ``seg`` [F + 1] offsets -> [F, n_sets_q, n_sets_c] int64 on the host."""
    from .. import som_device
    as_i64 = lambda m: _to_device(np.asarray(m, dtype=np.uint64).view(np.int64), np.int64)  # noqa: E731
    mq = as_i64(member_q)
    mc = mq if member_c is member_q else as_i64(member_c)
    xy, seg = _to_device(xy, np.float64), _to_device(seg, np.int64)
    return som_device.close_pair_counts(xy, mq, mc, seg, n_sets_q, n_sets_c, distlim, self_neighbor).cpu().numpy()


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


def _pack_sets(member: np.ndarray) -> np.ndarray:
    """[n, S <= 64] bool -> [n] uint64 with bit s = column s."""
    bits = np.uint64(1) << np.arange(member.shape[1], dtype=np.uint64)
    return (member.astype(np.uint64) * bits).sum(axis=1, dtype=np.uint64)


def set_pair_counts(xy, seg, member_q, member_c, distlim, self_neighbor=False):
    """``[F, Sq, Sc]`` int64: per FOV (rows ``seg[f] .. seg[f + 1]``) and pair of sets, the ordered pairs (a, b) of
    cells with ``member_q[a, s]`` and ``member_c[b, t]`` at float32 distance ``< distlim`` (and ``!= 0`` unless
    ``self_neighbor``).  ``member_q`` [n, Sq] and ``member_c`` [n, Sc] are boolean; any number of sets: one
    pxsom_close_pair_counts launch per block of 64 row sets x 64 column sets."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    member_q, member_c = np.asarray(member_q, dtype=bool), np.asarray(member_c, dtype=bool)
    seg = np.asarray(seg, dtype=np.int64)
    n = xy.shape[0]
    if member_q.ndim != 2 or member_c.ndim != 2 or member_q.shape[0] != n or member_c.shape[0] != n:
        raise ValueError("set_pair_counts: the memberships must be [n, sets] with one row per centroid (n = %d), got %s "
                         "and %s" % (n, member_q.shape, member_c.shape))
    out = np.zeros((len(seg) - 1, member_q.shape[1], member_c.shape[1]), dtype=np.int64)
    same = member_c is member_q
    packed_c = {}
    for r in range(0, member_q.shape[1], _MASK_BITS):
        mq = _pack_sets(member_q[:, r:r + _MASK_BITS])
        for c in range(0, member_c.shape[1], _MASK_BITS):
            if c not in packed_c:
                packed_c[c] = mq if same and c == r else _pack_sets(member_c[:, c:c + _MASK_BITS])
            nq, nc = min(_MASK_BITS, member_q.shape[1] - r), min(_MASK_BITS, member_c.shape[1] - c)
            out[:, r:r + nq, c:c + nc] = _close_pair_counts_device(xy, mq, packed_c[c], seg, nq, nc, distlim,
                                                                   bool(self_neighbor))
    return out


def get_pos_cell_labels_channel(thresh, current_fov_channel_data, cell_labels, current_marker):
    """The labels (the entries of ``cell_labels``) of the cells whose ``current_marker`` column of
    ``current_fov_channel_data`` lies above ``thresh``."""
    return cell_labels[current_fov_channel_data[current_marker] > thresh]


def get_pos_cell_labels_cluster(pheno, current_fov_neighborhood_data, cell_label_col, cell_type_col):
    """The ``cell_label_col`` entries of the rows of ``current_fov_neighborhood_data`` whose ``cell_type_col`` equals
    ``pheno``."""
    data = current_fov_neighborhood_data
    return data.loc[:, cell_label_col][data[cell_type_col] == pheno]


def compute_close_cell_num(centroids, dist_lim, analysis_type, current_fov_data=None, current_fov_channel_data=None,
                           cluster_ids=None, cell_types_analyze=None, thresh_vec=None, cell_label_col=_CELL_LABEL,
                           cell_type_col=_CELL_TYPE_NUM, *, exact=False):
    """Per pair (j, k) of markers (``analysis_type="channel"``: column j of ``current_fov_channel_data`` above
    ``thresh_vec[j]``) or of phenotypes (``"cluster"``: ``cell_type_col == cluster_ids[j]``), how many ordered pairs of
    distinct cells of one FOV -- the first positive for j, the second for k -- lie at float32 distance ``< dist_lim`` and
    ``> 0``.

    ``centroids`` is the ``[n, 2]`` array of the centroids of the rows of ``current_fov_data``, in the rows' order
    (``current_fov_channel_data`` holds the same rows); the reference passes the FOV's distance matrix here and looks
    the cells up by label.  The result is the reference's whenever labels are unique within the FOV.
    ``cell_types_analyze`` is accepted and unused, as in the reference.

    Returns ``(close_num, mark1_num, mark1poslabels)``: the table, the number of positive cells per marker and their
    labels (a list of Series).  The reference sums into ``numpy.uint16``, so ``close_num`` is a uint16 array holding the
    count modulo 65 536; ``exact=True`` returns the int64 counts themselves.
    """
    verify_in_list(analysis_type=analysis_type, good_analyses=["cluster", "channel"])
    xy = np.asarray(centroids, dtype=np.float64).reshape(-1, 2)
    if xy.shape[0] != len(current_fov_data):
        raise ValueError("centroids must hold one (row, column) pair per row of the table: got %d for %d rows"
                         % (xy.shape[0], len(current_fov_data)))
    mark1poslabels, positive = [], []
    if analysis_type == "channel":
        if len(current_fov_channel_data) != len(current_fov_data):
            raise ValueError("current_fov_channel_data must hold the rows of current_fov_data: got %d for %d rows"
                             % (len(current_fov_channel_data), len(current_fov_data)))
        cell_labels = current_fov_data[cell_label_col]
        for j in range(len(thresh_vec)):
            marker = current_fov_channel_data.columns[j]
            mark1poslabels.append(get_pos_cell_labels_channel(thresh_vec[j], current_fov_channel_data, cell_labels,
                                                              marker))
            positive.append((current_fov_channel_data[marker] > thresh_vec[j]).to_numpy())
    else:
        for pheno in cluster_ids:
            mark1poslabels.append(get_pos_cell_labels_cluster(pheno, current_fov_data, cell_label_col, cell_type_col))
            positive.append((current_fov_data[cell_type_col] == pheno).to_numpy())
    mark1_num = [len(labels) for labels in mark1poslabels]
    member = np.stack(positive, axis=1) if positive else np.zeros((xy.shape[0], 0), dtype=bool)
    counts = set_pair_counts(xy, [0, xy.shape[0]], member, member, dist_lim, False)[0]
    return (counts if exact else counts.astype(np.uint16)), mark1_num, mark1poslabels


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
