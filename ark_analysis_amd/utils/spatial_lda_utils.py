"""The numeric helpers of the reference's ``ark.utils.spatial_lda_utils``: the argument checks of the spatial-LDA
preprocessing (``ark_analysis_amd.spLDA.processing``) and the pooled within-cluster sum of the gap statistic.

``within_cluster_sums`` is the reference's ``sum over clusters of pdist(cluster).sum() / (2 n_c)`` on the host; with
``pairs="device"`` the sums of distances come from one pxsom_silhouette call, which already forms, for
every row i, the sum S[i, c] of the Euclidean distances to the rows of every cluster c.  ``pdist(cluster).sum()`` is
half of ``sum over i in c of S[i, c]``, so the pooled sum is ``sum over c of (sum over i in c of S[i, c]) / (4 n_c)``
and the pair matrices are never built.

Not built: the plotting helpers (``plot_topics_heatmap``, ``plot_fovs_with_topics``, ``make_plot_fn``) and
``save_spatial_lda_file`` / ``read_spatial_lda_file`` -- pickles of objects of the ``spatial_lda`` library, which is not
a dependency here."""
import numpy as np

from ..host_utils import verify_in_list

# ark.settings
FOV_ID, CELL_LABEL, CELL_SIZE, CENTROID_0, CENTROID_1, CELL_TYPE = ("fov", "label", "cell_size", "centroid-0",
                                                                    "centroid-1", "cell_meta_cluster")
BASE_COLS = [FOV_ID, CELL_LABEL, CELL_SIZE, CENTROID_0, CENTROID_1, CELL_TYPE]
EDA_KEYS = ["inertia", "silhouette", "gap_stat", "gap_sds", "cell_counts", "featurization"]
FEATURIZATIONS = ["cluster", "marker", "avg_marker", "count"]

_PAIRS_CHOICES = ("host", "device")


# ---- device entry point (the CPU tests swap it for the numpy statement of the same contract) ------------------------
def _silhouette_sums_device(x: np.ndarray, labels: np.ndarray, n_clusters: int):
    """som_device.silhouette_sums on host arrays: ``x`` [n, d] float64, ``labels`` [n] in [0, n_clusters) ->
    ``(sums [n, n_clusters] float64, counts [n_clusters] int32)`` on the host."""
    import torch
    from .. import _capi, som_device
    dev = _capi.require_gpu()
    sums, counts = som_device.silhouette_sums(
        torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev),
        torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev), int(n_clusters))
    return sums[0].cpu().numpy(), counts[0].cpu().numpy()


def check_format_cell_table_args(cell_table, markers, clusters):
    """The checks of ``format_cell_table``: the table holds ``BASE_COLS``, at least one of ``markers`` and ``clusters``
    is given, neither is empty, the markers are columns and the clusters are values of the cluster column."""
    verify_in_list(required_columns=BASE_COLS, cell_table_columns=cell_table.columns.to_list())
    if markers is None and clusters is None:
        raise ValueError("Markers and clusters cannot both be None.")
    if markers is not None:
        if len(markers) == 0:
            raise ValueError("The markers list is empty.")
        verify_in_list(markers=markers, cell_table_columns=cell_table.columns.to_list())
    if clusters is not None:
        if len(clusters) == 0:
            raise ValueError("The clusters list is empty.")
        verify_in_list(clusters=clusters, cell_table_clusters=cell_table[CELL_TYPE].unique().tolist())


def check_featurize_cell_table_args(cell_table, featurization, radius, cell_index):
    """The checks of ``featurize_cell_table``: ``radius`` is an ``int`` of at least 25, ``featurization`` is one of the
    four, the formatted table was made with what the featurisation needs, and ``cell_index`` is a column of its first
    frame."""
    if not isinstance(radius, int):
        raise TypeError("radius should be of type 'int'")
    if radius < 25:
        raise ValueError("radius must not be less than 25")
    verify_in_list(featurization=[featurization], featurization_options=FEATURIZATIONS)
    if featurization in ["cluster"] and "clusters" not in cell_table:
        raise ValueError("Cannot featurize clusters, because none were used for cell table formatting")
    if featurization in ["marker", "avg_marker"] and "markers" not in cell_table:
        raise ValueError("Cannot featurize markers, because none were used for cell table formatting")
    key = list(cell_table.keys())[0]
    verify_in_list(cell_index=[cell_index], cell_table_columns=cell_table[key].columns.to_list())


def within_cluster_sums(data, labels, *, pairs="host"):
    """The pooled within-cluster sum of the gap statistic: over the clusters of ``labels``, the sum of the Euclidean
    distances (not squared) of all pairs of the cluster's rows of ``data``, divided by twice the cluster's size.

    ``pairs="host"`` is the reference, ``scipy.spatial.distance.pdist`` per cluster.  ``pairs="device"`` takes, for every
    row, the sum of its distances to the rows of its own cluster from one pxsom_silhouette call (1 <= d <= 64 columns,
    2 .. 32 clusters, the existing errors otherwise) and adds them per cluster on the host in row order: each pair is
    then counted twice, hence the division by ``4 n_c``."""
    if pairs not in _PAIRS_CHOICES:
        raise ValueError("pairs must be 'host' or 'device', got %r" % (pairs,))
    labels = np.asarray(labels)
    if pairs == "host":
        from scipy.spatial.distance import pdist
        cluster_sums = []
        for x in np.unique(labels):
            d = data[labels == x]
            cluster_sums.append(pdist(d).sum() / (2 * d.shape[0]))
        return np.sum(cluster_sums)
    uniques, codes = np.unique(labels, return_inverse=True)
    codes = codes.reshape(-1)
    sums, counts = _silhouette_sums_device(np.asarray(data, dtype=np.float64), codes, len(uniques))
    own = sums[np.arange(len(codes)), codes]
    total = np.float64(0.0)
    for c in range(len(uniques)):
        total += np.cumsum(own[codes == c])[-1] / (4.0 * counts[c])      # a cumulative sum is the fold in row order
    return total
