"""The neighbourhood matrix and its k-means clusters (the reference's ``ark.analysis.neighborhood_analysis``).

``create_neighborhood_matrix`` counts, per cell, the cells of each phenotype within ``distlim`` -- for every included FOV
in one device launch over the centroid columns of the cell table (pxsom_neighbor_counts).  The reference
reads one N x N distance matrix per FOV from ``dist_mat_dir``; here that directory is never opened.
``generate_cluster_matrix_results`` runs k-means over the counts on the host and builds the reference's three tables; its
first frame carries the ``kmeans_neighborhood`` column that ``utils.data_utils.generate_and_save_neighborhood_cluster_masks``
consumes.  Between the two, ``compute_cluster_metrics_inertia`` and ``compute_cluster_metrics_silhouette`` sweep k: the
fits on the host (or, with ``kmeans="device"`` in any of the three, in one pxsom_kmeans_lloyd call: DESIGN.md K19), the
silhouette scores of every k from one device call (pxsom_silhouette); they return a
``pandas.Series`` indexed by ``cluster_num`` where the reference returns an ``xarray.DataArray``.

The notebook's other two steps, the cell-distance and the diversity analysis, are in ``cell_neighborhood_stats``.

The mixing-score notebook: ``compute_cell_ratios`` and ``compute_mixing_score`` are the reference's, host code over a
neighbourhood matrix; ``compute_mixing_scores`` gives the scores of a whole cohort straight from the cell table -- the
target / reference interaction totals of every FOV are one pxsom_close_pair_counts launch with two sets,
so neither the distance files nor the neighbourhood matrix are needed.

Not mirrored: ``calc_dist_matrix`` and the ``.xr`` files (xarray is not a dependency here), the enrichment statistics
and the plots."""
import warnings

import numpy as np
import pandas as pd

from ..host_utils import verify_in_list
from . import spatial_analysis_utils
from ._cells import centroid_columns, fov_rows_and_segments

# the reference's column names (ark.settings)
_FOV_ID, _CELL_LABEL, _CELL_TYPE, _KMEANS_CLUSTER = "fov", "label", "cell_meta_cluster", "kmeans_neighborhood"
_CELL_SIZE, _CENTROIDS = "cell_size", ("centroid-0", "centroid-1")


def create_neighborhood_matrix(all_data, dist_mat_dir=None, included_fovs=None, distlim=50, self_neighbor=False,
                               fov_col=_FOV_ID, cell_label_col=_CELL_LABEL, cell_type_col=_CELL_TYPE, *,
                               centroid_cols=_CENTROIDS):
    """Per cell, the number of neighbours of each phenotype.

    Args:
        all_data (pandas.DataFrame): the cell table: FOV, label, phenotype and the two centroid columns.
        dist_mat_dir: accepted for the reference's positional order and never opened.  The result equals the
            reference's whenever the files there were written by ``calc_dist_matrix`` from this same table (what the
            notebook does) and labels are unique within a FOV: the distances are then those of ``centroid_cols``.
        included_fovs (list): FOVs to analyse (default: all).  The others keep rows of zeros, which are then dropped.
        distlim: neighbours lie at float32 distance ``< distlim``, compared as numpy compares a float32 array with it.
        self_neighbor (bool): count a cell (and any cell at float32 distance 0) as its own neighbour.
        centroid_cols: the two centroid columns of ``all_data``.

    Returns ``(counts, freqs)``: the three id columns, then one float64 column per phenotype in order of first
    appearance; ``freqs`` divides a cell's counts by its number of neighbours.  Cells without any neighbour are dropped
    (index reset), with a ``UserWarning`` when more than 5 % of all cells go.

    Under a process group every rank computes the whole table: it is one launch, with nothing to exchange.
    """
    if included_fovs is None:
        included_fovs = all_data[fov_col].unique()
    verify_in_list(fov_names=included_fovs, unique_fovs=all_data[fov_col].unique())
    centroid_cols = centroid_columns(all_data, centroid_cols, "create_neighborhood_matrix", "all_data")

    id_cols = [fov_col, cell_label_col, cell_type_col]
    ids = all_data[id_cols].reset_index(drop=True)
    type_codes, type_names = pd.factorize(ids[cell_type_col].to_numpy(), sort=False)   # order of first appearance
    if (type_codes < 0).any():
        raise ValueError("create_neighborhood_matrix: column %r holds missing values" % cell_type_col)
    n_cells, n_types = len(ids), len(type_names)

    # rows of the included FOVs, FOV by FOV in table order: one segment each
    fov_codes, fov_names = pd.factorize(ids[fov_col].to_numpy(), sort=False)
    wanted = np.isin(fov_codes, np.flatnonzero(pd.Index(fov_names).isin(list(included_fovs))))
    rows, seg = fov_rows_and_segments(np.where(wanted, fov_codes, -1), len(fov_names))

    counts = np.zeros((n_cells, n_types))
    freqs = np.zeros((n_cells, n_types))
    if len(rows):
        xy = all_data[centroid_cols].to_numpy(dtype=np.float64)[rows]
        got = spatial_analysis_utils._neighbor_counts_device(xy, type_codes[rows], seg, n_types, distlim,
                                                             bool(self_neighbor)).astype(np.float64)
        counts[rows] = got
        freqs[rows] = spatial_analysis_utils._freqs(got)

    keep = counts.sum(axis=1) != 0
    frames = []
    for values in (counts, freqs):
        frame = pd.concat([ids, pd.DataFrame(values, columns=pd.Index(list(type_names), dtype=object))], axis=1)
        frames.append(frame.loc[keep].reset_index(drop=True))
    if keep.sum() / n_cells < 0.95:
        warnings.warn(UserWarning("More than 5% of cells have no neighbor within the provided radius and have been "
                                  "omitted. We suggest increasing the distlim value to reduce the number of cells "
                                  "excluded from analysis."))
    return frames[0], frames[1]


def generate_cluster_matrix_results(all_data, neighbor_mat, cluster_num, seed=42, excluded_channels=None,
                                    included_fovs=None, cluster_label_col=_KMEANS_CLUSTER, fov_col=_FOV_ID,
                                    cell_type_col=_CELL_TYPE, label_col=_CELL_LABEL, pre_channel_col=_CELL_SIZE,
                                    post_channel_col=_CELL_LABEL, *, kmeans="host"):
    """k-means over the neighbourhood matrix (on the host, or with ``kmeans="device"`` its ten restarts in one device
    call: DESIGN.md K19), then the reference's three tables:

    - ``all_data`` restricted to the included FOVs and to cells of ``neighbor_mat``, with ``cluster_label_col`` attached;
    - clusters x phenotypes: how many cells of each phenotype a cluster holds (index ``Cluster<k>``);
    - clusters x channels: the mean of every column strictly between ``pre_channel_col`` and ``post_channel_col``
      (less ``excluded_channels``) per cluster.

    The labels come from ``spatial_analysis_utils.generate_cluster_labels``.
    """
    spatial_analysis_utils._check_kmeans(kmeans)
    if included_fovs is None:
        included_fovs = neighbor_mat[fov_col].unique()
    verify_in_list(fov_names=included_fovs, unique_fovs=all_data[fov_col].unique())
    if excluded_channels is not None:
        verify_in_list(columns_to_exclude=excluded_channels, column_names=all_data.columns)
    if cluster_num < 2:
        raise ValueError("Invalid k provided for clustering")

    mat = neighbor_mat[neighbor_mat[fov_col].isin(included_fovs)].copy()
    route = {} if kmeans == "host" else {"kmeans": kmeans}      # the default call is the one it has always been
    mat[cluster_label_col] = spatial_analysis_utils.generate_cluster_labels(
        mat.drop([fov_col, label_col, cell_type_col], axis=1), cluster_num, seed=seed, **route)

    clustered = all_data[all_data[fov_col].isin(included_fovs)].merge(
        mat[[fov_col, label_col, cluster_label_col]], on=[fov_col, label_col])

    sizes = clustered.groupby([cluster_label_col, cell_type_col]).size().reset_index(name="count")
    per_type = sizes.pivot(index=cluster_label_col, columns=cell_type_col, values="count").fillna(0).astype(int)
    per_type.index = ["Cluster" + str(c) for c in per_type.index]

    first = np.where(clustered.columns == pre_channel_col)[0][0] + 1
    last = np.where(clustered.columns == post_channel_col)[0][0]
    label_at = np.where(clustered.columns == cluster_label_col)[0][0]
    markers = clustered.iloc[:, list(range(first, last)) + [label_at]]
    if excluded_channels is not None:
        markers = markers.drop(excluded_channels, axis=1)
    means = markers.groupby([cluster_label_col]).mean()
    means.index = ["Cluster" + str(c) for c in means.index]
    return clustered, per_type, means


def _sweep_data(neighbor_mat, min_k, max_k, included_fovs, fov_col, label_col, cell_col):
    """The checks and the column handling the two sweeps share: the rows of the included FOVs without the id columns."""
    if included_fovs is None:
        included_fovs = neighbor_mat[fov_col].unique()
    if min_k < 2 or max_k < 2:
        raise ValueError("Invalid k provided for clustering")
    verify_in_list(fov_names=included_fovs, unique_fovs=neighbor_mat[fov_col].unique())
    data = neighbor_mat[neighbor_mat[fov_col].isin(included_fovs)]
    return data.drop([fov_col, label_col, cell_col], axis=1)


def compute_cluster_metrics_inertia(neighbor_mat, min_k=2, max_k=10, seed=42, included_fovs=None, fov_col=_FOV_ID,
                                    label_col=_CELL_LABEL, cell_col=_CELL_TYPE, *, kmeans="host"):
    """The k-means inertia of the neighbourhood matrix for every k of ``min_k .. max_k`` (both at least 2), over the
    rows of ``included_fovs`` (default: all); ``kmeans`` is passed down.  Returns
    ``spatial_analysis_utils.compute_kmeans_inertia``'s Series."""
    spatial_analysis_utils._check_kmeans(kmeans)
    data = _sweep_data(neighbor_mat, min_k, max_k, included_fovs, fov_col, label_col, cell_col)
    return spatial_analysis_utils.compute_kmeans_inertia(neighbor_mat_data=data, min_k=min_k, max_k=max_k, seed=seed,
                                                        kmeans=kmeans)


def compute_cluster_metrics_silhouette(neighbor_mat, min_k=2, max_k=10, seed=42, included_fovs=None, fov_col=_FOV_ID,
                                       label_col=_CELL_LABEL, cell_col=_CELL_TYPE, subsample=None, *,
                                       kmeans="host"):
    """The silhouette score of the k-means clusters of the neighbourhood matrix for every k of ``min_k .. max_k`` (both
    at least 2), over the rows of ``included_fovs`` (default: all); ``subsample`` rows per cluster are scored when it is
    given; ``kmeans`` is passed down.  Returns ``spatial_analysis_utils.compute_kmeans_silhouette``'s Series."""
    spatial_analysis_utils._check_kmeans(kmeans)
    data = _sweep_data(neighbor_mat, min_k, max_k, included_fovs, fov_col, label_col, cell_col)
    return spatial_analysis_utils.compute_kmeans_silhouette(neighbor_mat_data=data, min_k=min_k, max_k=max_k, seed=seed,
                                                            subsample=subsample, kmeans=kmeans)


# ---- mixing scores --------------------------------------------------------------------------------------------------
_MIXING_TYPES = ("percent", "homogeneous")


def _check_populations(target_cells, reference_cells, mixing_type=None):
    overlap = [cell for cell in target_cells if cell in reference_cells]
    if overlap:
        raise ValueError("The following cell types were included in both the target and reference populations: %s"
                         % overlap)
    if mixing_type is not None and mixing_type not in _MIXING_TYPES:
        raise ValueError('Please provide a valid mixing_type: "percent" or "homogeneous".')


def _mixing_exit(target_total, ref_total, ratio_threshold, cell_count_thresh):
    """The reference's three NaN exits, in its order: too few cells, a population absent, a ratio over the threshold."""
    if target_total + ref_total < cell_count_thresh:
        return True
    if ref_total == 0 or target_total == 0:
        return True
    return ref_total / target_total > ratio_threshold or target_total / ref_total > ratio_threshold


def _mixing_quotient(reference_target, target_target, reference_reference, mixing_type):
    """The score from the three interaction totals, divided as numpy divides float64 (0 / 0 is NaN)."""
    mixed = np.float64(reference_target)
    if mixing_type == "percent":
        return mixed / (mixed + np.float64(target_target))
    return mixed / (np.float64(target_target) + np.float64(reference_reference))


def compute_cell_ratios(neighbors_mat, target_cells, reference_cells, fov_list, bin_number=10, cell_col=_CELL_TYPE,
                        fov_col=_FOV_ID, label_col=_CELL_LABEL):
    """Per FOV of ``fov_list``, the number of target cells over the number of reference cells among the rows of the
    neighbourhood matrix ``neighbors_mat``; NaN where either population is absent.

    Returns the reference's ``ratio_data`` frame: columns ``fov`` and ``cell_ratio``.  The reference also draws two
    box plots and two histograms of the ratios; plotting stays out of this package, so ``bin_number`` (the histograms'
    bins) is accepted and unused."""
    verify_in_list(provided_column_names=[cell_col, fov_col, label_col], cell_neighbors_columns=neighbors_mat.columns)
    ratios = []
    for fov in fov_list:
        types = neighbors_mat.loc[neighbors_mat[fov_col] == fov, cell_col]
        target_total, reference_total = int(types.isin(target_cells).sum()), int(types.isin(reference_cells).sum())
        ratios.append(np.nan if target_total == 0 or reference_total == 0 else target_total / reference_total)
    return pd.DataFrame({"fov": list(fov_list), "cell_ratio": np.asarray(ratios, dtype=np.float64)})


def compute_mixing_score(fov_neighbors_mat, target_cells, reference_cells, mixing_type, ratio_threshold=5,
                         cell_count_thresh=200, cell_col=_CELL_TYPE, fov_col=_FOV_ID, label_col=_CELL_LABEL):
    """The mixing score of one FOV from its rows of the neighbourhood matrix (host code, as in the reference).

    With rt the neighbours of reference phenotypes that target cells have, tt those of target phenotypes that target
    cells have and rr those of reference phenotypes that reference cells have: ``"percent"`` is rt / (rt + tt),
    ``"homogeneous"`` rt / (tt + rr).  Returns ``(score, count)`` with count = target + reference cells; the score is
    NaN when count < ``cell_count_thresh``, when a population is absent, or when one population outnumbers the other
    by more than ``ratio_threshold`` (tested in this order).  ValueError for a phenotype in both populations and for
    an unknown ``mixing_type``.  ``fov_neighbors_mat`` is left as it is."""
    verify_in_list(provided_column_names=[cell_col, fov_col, label_col],
                   cell_neighbors_columns=fov_neighbors_mat.columns)
    _check_populations(target_cells, reference_cells, mixing_type)
    types = fov_neighbors_mat[cell_col]
    is_target, is_reference = types.isin(target_cells).to_numpy(), types.isin(reference_cells).to_numpy()
    present = set(types.unique())
    numeric = fov_neighbors_mat.drop(columns=[fov_col, label_col, cell_col])

    def interactions(rows, cells):
        # one column per listed phenotype that the FOV holds, in the list's order (a name listed twice counts twice)
        cols = [c for c in cells if c in present]
        return np.float64(sum(numeric.loc[rows, c].sum() for c in cols)) if cols else np.float64(0)
    target_total, ref_total = int(is_target.sum()), int(is_reference.sum())
    if _mixing_exit(target_total, ref_total, ratio_threshold, cell_count_thresh):
        return np.nan, target_total + ref_total
    score = _mixing_quotient(interactions(is_target, reference_cells), interactions(is_target, target_cells),
                             interactions(is_reference, reference_cells), mixing_type)
    return score, target_total + ref_total


def compute_mixing_scores(cell_table, target_cells, reference_cells, mixing_type, distlim=50, ratio_threshold=5,
                          cell_count_thresh=200, self_neighbor=False, included_fovs=None, fov_col=_FOV_ID,
                          cell_type_col=_CELL_TYPE, centroid_cols=_CENTROIDS):
    """The mixing score of every FOV of a cohort, straight from the cell table.

    Equal, value for value (NaN included), to the notebook's loop -- ``create_neighborhood_matrix(cell_table,
    distlim=distlim, self_neighbor=self_neighbor)``, then ``compute_mixing_score`` on every FOV's rows -- without the
    distance files and without the neighbourhood matrix: target is bit 0 and reference bit 1 of a cell's mask, and one
    pxsom_close_pair_counts launch gives, per FOV, the 2 x 2 table of close pairs between the two
    populations; rt, tt and rr of ``compute_mixing_score`` are its entries [0, 1], [0, 0] and [1, 1], integers below
    2^53, so the quotient is the loop's exactly.  The loop counts a population over the rows of the neighbourhood
    matrix, which has dropped the cells without any neighbour; which cells those are comes from one
    pxsom_neighbor_counts launch with a single type.  The totals and the three exits are evaluated per FOV on the host.
    A phenotype listed twice in a population counts once.

    Returns a frame with columns ``fov``, ``mixing_score`` and ``cell_count``, one row per FOV of ``included_fovs``
    (default: every FOV, in order of first appearance)."""
    _check_populations(target_cells, reference_cells, mixing_type)
    if included_fovs is None:
        included_fovs = cell_table[fov_col].unique()
    included_fovs = list(included_fovs)
    verify_in_list(fov_names=included_fovs, unique_fovs=cell_table[fov_col].unique())
    centroid_cols = centroid_columns(cell_table, centroid_cols, "compute_mixing_scores")
    types = cell_table[cell_type_col]
    if types.isna().any():
        raise ValueError("compute_mixing_scores: column %r holds missing values" % cell_type_col)

    # rows of the included FOVs, FOV by FOV in the order of included_fovs: one segment each
    fov_codes = pd.Categorical(cell_table[fov_col].to_numpy(), categories=pd.unique(np.asarray(included_fovs, dtype=object)))
    codes = np.asarray(fov_codes.codes, dtype=np.int64)
    n_fovs = len(fov_codes.categories)
    rows, seg = fov_rows_and_segments(codes, n_fovs)
    is_target, is_reference = types.isin(target_cells).to_numpy()[rows], types.isin(reference_cells).to_numpy()[rows]

    pairs = np.zeros((n_fovs, 2, 2), dtype=np.int64)
    target_total = reference_total = np.zeros(n_fovs, dtype=np.int64)
    if len(rows):
        xy = cell_table[centroid_cols].to_numpy(dtype=np.float64)[rows]
        member = is_target.astype(np.uint64) | (is_reference.astype(np.uint64) << np.uint64(1))
        pairs = spatial_analysis_utils._close_pair_counts_device(xy, member, member, seg, 2, 2, distlim,
                                                                 bool(self_neighbor))
        kept = spatial_analysis_utils._neighbor_counts_device(xy, np.zeros(len(rows), dtype=np.int64), seg, 1, distlim,
                                                              bool(self_neighbor))[:, 0] != 0
        target_total = np.bincount(codes[rows][kept & is_target], minlength=n_fovs)
        reference_total = np.bincount(codes[rows][kept & is_reference], minlength=n_fovs)

    scores, counts = [], []
    for f in range(n_fovs):
        t, r = int(target_total[f]), int(reference_total[f])
        counts.append(t + r)
        scores.append(np.nan if _mixing_exit(t, r, ratio_threshold, cell_count_thresh) else
                      _mixing_quotient(pairs[f, 0, 1], pairs[f, 0, 0], pairs[f, 1, 1], mixing_type))
    position = {fov: f for f, fov in enumerate(fov_codes.categories)}
    order = [position[fov] for fov in included_fovs]
    return pd.DataFrame({"fov": included_fovs, "mixing_score": np.asarray(scores, dtype=np.float64)[order],
                         "cell_count": np.asarray(counts, dtype=np.int64)[order]})
