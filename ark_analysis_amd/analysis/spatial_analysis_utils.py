"""Neighbour counts and k-means labels of the reference's ``ark.analysis.spatial_analysis_utils``.

``compute_neighbor_counts`` takes a FOV's centroids where the reference takes its distance matrix: the counts come from
one pxsom_neighbor_counts launch and the N x N matrix is never built.  Not mirrored: ``calc_dist_matrix``
and its ``.xr`` files (xarray is not a dependency here), the distance-feature columns
(``append_distance_features_to_dataset``; the cell-distance analysis is ``cell_neighborhood_stats``), the enrichment statistics
(``compute_close_cell_num``, ``calculate_enrichment_stats``), the k-means inertia / silhouette sweeps and everything that
plots."""
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


def generate_cluster_labels(neighbor_mat_data, cluster_num, seed=42):
    """k-means labels 1 .. ``cluster_num`` of the rows of ``neighbor_mat_data`` (scikit-learn ``KMeans`` with
    ``n_init=10`` and ``random_state=seed``, on the host).  The same data gives the same clusters on every run; which
    number a cluster gets depends on the scikit-learn build."""
    from sklearn.cluster import KMeans
    fit = KMeans(n_clusters=cluster_num, random_state=seed, n_init=10).fit(neighbor_mat_data)
    return fit.labels_ + 1
