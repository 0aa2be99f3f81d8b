"""The preprocessing of the reference's ``ark.spLDA.processing``: formatted cell tables, neighbourhood features and the
k-means diagnostics that help to choose a number of topics.

``featurize_cell_table`` builds one feature row per anchor cell from the cells within ``radius`` of it.  The reference
hands every FOV to ``spatial_lda.featurization.featurize_samples``, which builds one pandas sub-frame per anchor cell;
here the whole cohort is one pxsom_neighborhood_sums launch: per cell, the sum of the feature rows of
the cells of its FOV inside the radius, and their number.  ``spatial_lda`` is not a dependency and was not
available to compare against: what it does is taken as DESIGN.md K24 states it -- parity with spatial_lda itself
unpinned.  The one recalled choice that could differ, whether a cell at exactly ``radius`` belongs to the neighbourhood,
is ``RADIUS_TEST``.

``compute_topic_eda`` and ``gap_stat`` are the reference's with ``kmeans="host"`` (scikit-learn on the host, with
``seed`` as the only addition).  With ``kmeans="device"`` every topic number is fitted in one pxsom_kmeans_lloyd call
(``spatial_analysis_utils.kmeans_fits_device``, K19), the silhouette scores of all of them come from one
pxsom_silhouette call (K15), and every pooled within-cluster sum comes from K15's sums of distances
(``spatial_lda_utils.within_cluster_sums(pairs="device")``), so no pair matrix is built.

Not built: ``create_difference_matrices`` beyond its argument check (it is ``spatial_lda``'s
``make_merged_difference_matrices``), the model fit itself, the plotting helpers and the pickle helpers of
``ark.utils.spatial_lda_utils``."""
import copy

import numpy as np
import pandas as pd

from ..analysis import spatial_analysis_utils as sau
from ..analysis._cells import _to_device
from ..utils import spatial_lda_utils as spu

# How a cell at exactly `radius` from the anchor is treated: "lt" leaves it out (np.linalg.norm(...) < radius, as
# spatial_lda is recalled to do), "le" takes it in.  Recalled, not pinned against the library.
RADIUS_TEST = "lt"
RECALLED = {"radius_test": RADIUS_TEST, "include_anchors": True, "marker_threshold": 0.5}
_MARKER_THRESHOLD = 0.5


# ---- device entry point (the CPU tests swap it for the numpy statement of the same contract) ------------------------
def _neighborhood_sums_device(xy: np.ndarray, feats, seg: np.ndarray, radius):
    """som_device.neighborhood_sums on host arrays: ``xy`` [n, 2] float64, ``feats`` [n, p] float64 or None, ``seg``
    [F + 1] offsets -> ``(sums [n, p] float64, counts [n] int32)`` on the host, under ``RADIUS_TEST``."""
    from .. import som_device
    if RADIUS_TEST not in ("lt", "le"):
        raise ValueError("RADIUS_TEST must be 'lt' or 'le', got %r" % (RADIUS_TEST,))
    sums, counts = som_device.neighborhood_sums(
        _to_device(xy, np.float64), None if feats is None else _to_device(feats, np.float64), _to_device(seg, np.int64),
        radius, closed=RADIUS_TEST == "le")
    return sums.cpu().numpy(), counts.cpu().numpy()


def format_cell_table(cell_table, markers=None, clusters=None):
    """A cell table of one or more FOVs as the dict the spatial-LDA functions take: per FOV a frame with the columns
    ``cell_size``, ``x``, ``y``, ``cluster``, the ``markers`` and the all-true ``is_index`` and ``isimmune``, its rows
    those of the FOV (of the ``clusters``, when given) renumbered from 0; and under ``"fovs"``, ``"markers"`` and
    ``"clusters"`` the sorted FOV names and the two arguments."""
    spu.check_format_cell_table_args(cell_table=cell_table, markers=markers, clusters=clusters)
    keep_cols = copy.deepcopy(spu.BASE_COLS)
    if markers is not None:
        keep_cols += markers
    kept = cell_table.drop(columns=[c for c in cell_table.columns if c not in keep_cols])
    kept = kept.rename(columns={spu.CENTROID_0: "x", spu.CENTROID_1: "y", spu.CELL_TYPE: "cluster"})
    fovs = np.unique(kept[spu.FOV_ID])
    fov_dict = {}
    for fov in fovs:
        df = kept[kept[spu.FOV_ID] == fov].drop(columns=[spu.FOV_ID, spu.CELL_LABEL])
        if clusters is not None:
            df = df[df["cluster"].isin(clusters)]
        df["is_index"] = True
        df["isimmune"] = True
        fov_dict[fov] = df.reset_index(drop=True)
    fov_dict["fovs"] = fovs
    fov_dict["markers"] = markers
    fov_dict["clusters"] = clusters
    return fov_dict


def neighborhood_features(cell_table, featurization="cluster", radius=100, cell_index="is_index"):
    """The frame ``featurize_cell_table`` returns under ``"featurized_fovs"``, without the argument checks and the
    training split: one row per cell whose ``cell_index`` is true, indexed by ``(fov, position of the cell in that
    FOV's frame)`` -- FOVs in the order of ``cell_table["fovs"]``, cells in frame order.  The neighbourhood of an anchor
    is every cell of its FOV, itself included, at a distance ``sqrt(dx * dx + dy * dy)`` below ``radius`` in binary64
    (``RADIUS_TEST``).  One device call covers the cohort."""
    fovs = [f for f in np.asarray(cell_table["fovs"]).tolist()]
    frames = [cell_table[f] for f in fovs]
    sizes = [len(df) for df in frames]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)

    def column_block(cols):
        if not frames:
            return np.zeros((0, len(cols)), dtype=np.float64)
        return np.concatenate([df[cols].to_numpy(dtype=np.float64).reshape(len(df), len(cols)) for df in frames])
    xy = column_block(["x", "y"])

    if featurization == "cluster":
        values = np.concatenate([df["cluster"].to_numpy() for df in frames]) if frames else np.zeros(0)
        columns, codes = np.unique(values, return_inverse=True)
        columns = columns.tolist()
        feats = np.zeros((len(values), len(columns)), dtype=np.float64)
        feats[np.arange(len(values)), codes.reshape(-1)] = 1.0
    elif featurization == "marker":
        columns = list(cell_table["markers"])
        feats = (column_block(columns) > _MARKER_THRESHOLD).astype(np.float64)
    elif featurization == "avg_marker":
        columns = list(cell_table["markers"])
        feats = column_block(columns)
    else:
        columns, feats = ["count"], None

    sums, counts = _neighborhood_sums_device(xy, feats, seg, radius)

    anchors = np.concatenate([df[cell_index].to_numpy().astype(bool) for df in frames]) if frames else np.zeros(0, bool)
    rows = np.flatnonzero(anchors)
    fov_of_row = np.repeat(np.arange(len(fovs)), sizes)[rows]
    index = pd.MultiIndex.from_arrays(
        [np.asarray(fovs, dtype=object)[fov_of_row] if len(fovs) else np.zeros(0, dtype=object), rows - seg[fov_of_row]])
    if featurization == "count":
        data = counts[rows].astype(np.int64).reshape(-1, 1)
    elif featurization == "avg_marker":
        with np.errstate(divide="ignore", invalid="ignore"):
            data = sums[rows] / counts[rows].astype(np.float64)[:, None]
    else:
        data = sums[rows].astype(np.int64)      # sums of zeros and ones: exact
    return pd.DataFrame(data, index=index, columns=columns)


def featurize_cell_table(cell_table, featurization="cluster", radius=100, cell_index="is_index", n_processes=None,
                         train_frac=0.75, *, seed=None):
    """Statistics of the cellular neighbourhood of every reference cell of a formatted cell table
    (:func:`format_cell_table`), by ``featurization``:

    - ``cluster``: per cell cluster, the number of cells within ``radius`` of the cell that belong to it (one column per
      cluster value of the whole table, in sorted order);
    - ``marker``: per marker, the number of cells within ``radius`` with an expression above 0.5;
    - ``avg_marker``: per marker, the mean expression of the cells within ``radius``;
    - ``count``: the number of cells within ``radius`` (the column ``"count"``).

    ``cell_index`` names the boolean column of the reference cells, which count in their own neighbourhood.
    ``n_processes`` is accepted and ignored: the cohort is one device call (:func:`neighborhood_features`).
    ``train_frac`` of the rows, stratified by FOV, are drawn as training data with
    ``sklearn.model_selection.train_test_split``; ``seed`` is its ``random_state`` (None: unseeded, as the reference).
    As in the reference, a FOV with a single reference cell cannot be stratified and is scikit-learn's ValueError.

    Returns ``{"featurized_fovs": frame, "train_features": frame, "featurization": featurization}``."""
    spu.check_featurize_cell_table_args(cell_table=cell_table, featurization=featurization, radius=radius,
                                        cell_index=cell_index)
    from sklearn.model_selection import train_test_split
    featurized_fovs = neighborhood_features(cell_table, featurization, radius, cell_index)
    all_sample_idxs = featurized_fovs.index.map(lambda x: x[0])
    train_features_fraction, _ = train_test_split(featurized_fovs, test_size=1. - train_frac, stratify=all_sample_idxs,
                                                  random_state=seed)
    return {"featurized_fovs": featurized_fovs, "train_features": train_features_fraction,
            "featurization": featurization}


def create_difference_matrices(cell_table, features, training=True, inference=True):
    """Not built: the difference matrices are ``spatial_lda.featurization.make_merged_difference_matrices``.  The
    reference's argument check comes first."""
    if not training and not inference:
        raise ValueError("One or both of 'training' or 'inference' must be True")
    raise NotImplementedError("create_difference_matrices needs spatial_lda.featurization.make_merged_difference_matrices, "
                              "which is not built here")


def _feature_range(features):
    values = np.asarray(features, dtype=np.float64)
    return values.min(axis=0), values.max(axis=0), values.shape


def _gap_from_sums(w_kb, clust_inertia, num_boots):
    gap = np.log(w_kb).mean() - np.log(clust_inertia)
    s = np.log(w_kb).std() * np.sqrt(1 + 1 / num_boots)
    return gap, s


def _gap_stats_device(features, topics, pooled, num_boots, seed):
    """``{k: (gap, s)}`` for every k of ``topics`` with the loops swapped: per bootstrap draw one uniform array and one
    ``kmeans_fits_device`` call for all topic numbers, so the draws are shared across k."""
    mins, maxs, (n, p) = _feature_range(features)
    rs = np.random if seed is None else np.random.RandomState(seed)
    w_kb = {k: [] for k in topics}
    for b in range(num_boots):
        boot_array = rs.uniform(low=mins, high=maxs, size=(n, p))
        fits = sau.kmeans_fits_device(boot_array, topics, seed, "auto")
        for k, fit in zip(topics, fits):
            w_kb[k].append(spu.within_cluster_sums(data=boot_array, labels=fit.labels_, pairs="device"))
    return {k: _gap_from_sums(w_kb[k], pooled[k], num_boots) for k in topics}


def gap_stat(features, k, clust_inertia, num_boots=25, *, kmeans="host", seed=None):
    """The gap statistic of Tibshirani, Walther and Hastie (2001) of a k-means model with ``k`` clusters of
    ``features`` whose pooled within-cluster sum is ``clust_inertia``: ``num_boots`` reference samples are drawn
    uniformly over the range of every column, clustered, and scored with ``within_cluster_sums``.

    ``kmeans="host"``: the reference's ``MiniBatchKMeans(batch_size=1024, n_init="auto")`` and host pair sums;
    ``seed`` seeds the fits and a ``numpy.random.RandomState`` for the draws (None: numpy's global state, unseeded
    fits).  ``kmeans="device"``: ``kmeans_fits_device`` (full-batch Lloyd, K19) and the device pair sums (K15).

    Returns ``(gap, s)``: the mean log reference sum minus ``log(clust_inertia)``, and the standard deviation of the
    log reference sums times ``sqrt(1 + 1 / num_boots)``."""
    sau._check_kmeans(kmeans)
    if kmeans == "device":
        return _gap_stats_device(features, [k], {k: clust_inertia}, num_boots, seed)[k]
    from sklearn.cluster import MiniBatchKMeans
    mins, maxs, (n, p) = _feature_range(features)
    rs = np.random if seed is None else np.random.RandomState(seed)
    w_kb = []
    for b in range(num_boots):
        boot_array = rs.uniform(low=mins, high=maxs, size=(n, p))
        boot_clust = MiniBatchKMeans(n_clusters=k, batch_size=1024, n_init="auto", random_state=seed).fit(boot_array)
        w_kb.append(spu.within_cluster_sums(data=boot_array, labels=boot_clust.labels_))
    return _gap_from_sums(w_kb, clust_inertia, num_boots)


def compute_topic_eda(features, featurization, topics, silhouette=False, num_boots=None, *, kmeans="host", seed=None):
    """Metrics of k-means models of the featurised neighbourhoods ``features`` for every number of ``topics``, to help
    choose one: ``inertia``, ``silhouette`` (Euclidean silhouette score, when asked for), ``gap_stat`` and ``gap_sds``
    (when ``num_boots`` is given, at least 25) and ``cell_counts`` (per cluster, the column sums of its rows), each a
    dict keyed by the topic number; and ``"featurization"``.

    ``kmeans="host"`` is the reference with ``random_state=seed``.  ``kmeans="device"``: all topic numbers are fitted in
    one ``kmeans_fits_device`` call, their silhouette scores come from one device call, every pooled within-cluster sum
    from the device pair sums, and the bootstrap draws of the gap statistic are shared across the topic numbers (one
    uniform array and one device fit of all topic numbers per draw) where the reference draws afresh for every k.
    The device routes take at most 64 feature columns and 32 topics."""
    sau._check_kmeans(kmeans)
    if num_boots is not None and num_boots < 25:
        raise ValueError("Number of bootstrap samples must be at least 25")
    if min(topics) <= 2 or max(topics) >= features.shape[0] - 1:
        raise ValueError("Number of topics must be in [2, %d]" % (features.shape[0] - 1))
    topics = list(topics)
    stat_names = ["inertia", "silhouette", "gap_stat", "gap_sds", "cell_counts"]
    stats = {name: {} for name in stat_names}

    def cell_counts(labels, k):
        return pd.DataFrame.from_dict({i: features[labels == i].sum(axis=0) for i in range(k)})

    if kmeans == "host":
        # the reference's loop, one topic number after the other (which is also its order of random draws)
        from sklearn.cluster import KMeans
        from sklearn.metrics import silhouette_score
        for k in topics:
            cluster_fit = KMeans(n_clusters=k, n_init="auto", random_state=seed).fit(features)
            stats["inertia"][k] = cluster_fit.inertia_
            if silhouette:
                stats["silhouette"][k] = silhouette_score(features, cluster_fit.labels_, metric="euclidean")
            if num_boots is not None:
                pooled_within_ss = spu.within_cluster_sums(data=features, labels=cluster_fit.labels_)
                stats["gap_stat"][k], stats["gap_sds"][k] = gap_stat(features, k, pooled_within_ss, num_boots, seed=seed)
            stats["cell_counts"][k] = cell_counts(cluster_fit.labels_, k)
    else:
        fits = sau.kmeans_fits_device(features, topics, seed, "auto")
        for k, fit in zip(topics, fits):
            stats["inertia"][k] = fit.inertia_
            stats["cell_counts"][k] = cell_counts(fit.labels_, k)
        if silhouette:
            values = np.asarray(features, dtype=np.float64)
            encoded = [sau._encode_labels(fit.labels_, len(values)) for fit in fits]
            scores = sau._silhouette_device(values, np.stack([codes for codes, _ in encoded]), [k for _, k in encoded])
            stats["silhouette"] = {k: float(s) for k, s in zip(topics, scores)}
        if num_boots is not None:
            pooled = {k: spu.within_cluster_sums(data=features, labels=fit.labels_, pairs="device")
                      for k, fit in zip(topics, fits)}
            for k, (gap, s) in _gap_stats_device(features, topics, pooled, num_boots, seed).items():
                stats["gap_stat"][k], stats["gap_sds"][k] = gap, s

    stats["featurization"] = featurization
    return stats


def fov_density(cell_table, total_pix=1024 ** 2):
    """Per FOV of a formatted cell table: ``average_area`` (the mean cell size), ``cellular_density`` (the summed cell
    sizes over ``total_pix``) and ``total_cells``, each a dict keyed by FOV -- to help choose the radius."""
    average_area, cellular_density, total_cells = {}, {}, {}
    for i in cell_table["fovs"]:
        average_area[i] = cell_table[i].cell_size.mean()
        cellular_density[i] = np.sum(cell_table[i].cell_size) / total_pix
        total_cells[i] = cell_table[i].shape[0]
    return {"average_area": average_area, "cellular_density": cellular_density, "total_cells": total_cells}
