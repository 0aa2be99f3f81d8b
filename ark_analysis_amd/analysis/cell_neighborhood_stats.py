"""Cell-distance and neighbourhood-diversity analysis (the reference's ``ark.analysis.cell_neighborhood_stats``).

``generate_cell_distance_analysis`` gives, per cell, the mean distance to its k nearest cells of every phenotype -- for the
whole cohort in one device launch over the centroid columns of the cell table (pxsom_nearest_type_means).
The reference reads one N x N distance matrix per FOV from ``dist_mat_dir`` and sorts a slice of it per phenotype; here
neither ``dist_mat_dir`` nor a ``dist_xr`` argument is ever opened.  The result equals the reference's, bit for bit,
whenever the ``.xr`` files were written by ``calc_dist_matrix`` from the same table (what the notebook does) and labels
are unique within a FOV: the distances are then those of ``centroid_cols``.  The device route holds ``1 <= k <= 32``.

``shannon_diversity``, ``compute_neighborhood_diversity`` and ``generate_neighborhood_diversity_analysis`` are host code:
one vectorised pass in place of the reference's per-cell filter of the frame, with the reference's bits.

Not mirrored: the plots."""
import os
from functools import reduce

import numpy as np
import pandas as pd

from ..host_utils import validate_paths, verify_in_list
from ._cells import _to_device, centroid_columns, fov_rows_and_segments

# the reference's column names (ark.settings)
_FOV_ID, _CELL_LABEL, _CELL_TYPE = "fov", "label", "cell_meta_cluster"
_CENTROIDS = ("centroid-0", "centroid-1")
MAX_K = 32      # som_device.NEAREST_MAX_K


# ---- device entry point (the CPU tests swap it for the numpy statement of the same contract) ------------------------
def _nearest_type_means_device(xy: np.ndarray, types: np.ndarray, seg: np.ndarray, n_types: int, k: int) -> np.ndarray:
    """som_device.nearest_type_means on host arrays: ``xy`` [n, 2] float64, ``types`` [n] in [0, n_types), ``seg``
    [F + 1] offsets -> [n, n_types] float32 on the host."""
    from .. import som_device
    xy, types, seg = _to_device(xy, np.float64), _to_device(types, np.int32), _to_device(seg, np.int64)
    return som_device.nearest_type_means(xy, types, seg, n_types, k).cpu().numpy()


def _check_k(k) -> int:
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k must lie in 1 .. %d: the device route keeps a cell's k nearest in registers (got %d)"
                         % (MAX_K, k))
    return k


def _centroids(cell_table, centroid_cols, who):
    return cell_table[centroid_columns(cell_table, centroid_cols, who)].to_numpy(dtype=np.float64)


def _type_codes(cell_table, cell_type_col, who):
    """(codes, names): ``names`` is ``np.unique`` of the column, ``codes`` the rows' positions in it."""
    codes, names = pd.factorize(cell_table[cell_type_col].to_numpy(), sort=True)
    if (codes < 0).any():
        raise ValueError("%s: column %r holds missing values" % (who, cell_type_col))
    return codes, names


# ---- cell distances -------------------------------------------------------------------------------------------------
def calculate_mean_distance_to_all_cell_types(cell_table, dist_xr, k, cell_type_col=_CELL_TYPE,
                                              cell_label_col=_CELL_LABEL, *, centroid_cols=_CENTROIDS):
    """Per cell of ONE FOV's table, the mean float32 distance to its ``k`` nearest cells of every phenotype (cells at
    float32 distance 0, the cell itself among them, do not count; NaN when a phenotype has fewer than ``k`` others).

    ``dist_xr`` is accepted for the reference's positional order and never opened; ``cell_label_col`` likewise (the
    reference uses it to look columns up in the matrix).  Returns a float64 frame on the table's index whose columns
    are ``np.unique`` of the FOV's phenotypes.
    """
    who = "calculate_mean_distance_to_all_cell_types"
    k = _check_k(k)
    xy = _centroids(cell_table, centroid_cols, who)
    codes, names = _type_codes(cell_table, cell_type_col, who)
    columns = pd.Index(names) if len(names) else pd.Index([], dtype=object)
    if not len(cell_table):
        return pd.DataFrame(index=cell_table.index.values, columns=columns, dtype=np.float64)
    means = _nearest_type_means_device(xy, codes, np.array([0, len(cell_table)]), len(names), k)
    return pd.DataFrame(means.astype(np.float64), index=cell_table.index.values, columns=columns)


def calculate_mean_distance_to_cell_type(cell_table, dist_xr, cell_cluster, k, cell_type_col=_CELL_TYPE,
                                         cell_label_col=_CELL_LABEL, *, centroid_cols=_CENTROIDS):
    """Per cell of ONE FOV's table, the mean float32 distance to its ``k`` nearest cells of phenotype ``cell_cluster``:
    a float32 array in the table's order, or a list of NaN when the FOV holds fewer than ``k`` such cells (the
    reference's two return types).  ``dist_xr`` is never opened."""
    who = "calculate_mean_distance_to_cell_type"
    k = _check_k(k)
    xy = _centroids(cell_table, centroid_cols, who)
    member = (cell_table[cell_type_col] == cell_cluster).to_numpy()
    if member.sum() < k:
        return [np.nan] * len(cell_table)
    # two codes: the phenotype asked for and everything else
    means = _nearest_type_means_device(xy, np.where(member, 0, 1), np.array([0, len(cell_table)]), 2, k)
    return means[:, 0]


def generate_cell_distance_analysis(cell_table, dist_mat_dir, save_path, k, cell_type_col=_CELL_TYPE, fov_col=_FOV_ID,
                                    cell_label_col=_CELL_LABEL, *, centroid_cols=_CENTROIDS):
    """Per cell of the cohort, the mean distance to its ``k`` nearest cells of every phenotype of its FOV.

    Args:
        cell_table (pandas.DataFrame): the cell table: FOV, label, phenotype and the two centroid columns.
        dist_mat_dir: accepted for the reference's positional order and never opened (see the module's docstring).
        save_path: the frame is written there with ``to_csv(index=False)``.
        k (int): how many nearest cells of a phenotype to average, 1 .. 32.
        centroid_cols: the two centroid columns of ``cell_table``.

    Returns the frame: FOVs in ``np.unique`` order, each FOV's rows in table order under the table's index; ``fov_col``,
    ``cell_label_col``, ``cell_type_col``, then one float64 column per phenotype -- the union over the FOVs in order of
    first appearance over the per-FOV sorted lists, NaN where a FOV lacks the phenotype.  ONE device call covers the
    cohort.  Under a process group every rank computes the whole table: it is one launch, with nothing to exchange.
    """
    who = "generate_cell_distance_analysis"
    k = _check_k(k)
    xy = _centroids(cell_table, centroid_cols, who)
    codes, names = _type_codes(cell_table, cell_type_col, who)
    fov_codes, fov_names = pd.factorize(cell_table[fov_col].to_numpy(), sort=True)      # np.unique order
    if (fov_codes < 0).any():
        raise ValueError("%s: column %r holds missing values" % (who, fov_col))
    rows, seg = fov_rows_and_segments(fov_codes, len(fov_names))

    n_types = max(len(names), 1)
    means = np.empty((0, n_types), dtype=np.float32)
    if len(rows):
        means = _nearest_type_means_device(xy[rows], codes[rows], seg, n_types, k)

    # pd.concat's column order: first appearance over the FOVs' sorted phenotype lists
    order, seen = [], np.zeros(n_types, dtype=bool)
    for f in range(len(fov_names)):
        here = np.unique(codes[rows[seg[f]:seg[f + 1]]])
        order.extend(here[~seen[here]].tolist())
        seen[here] = True

    ordered = cell_table.iloc[rows]
    out = pd.DataFrame(means[:, order].astype(np.float64), index=ordered.index,
                       columns=pd.Index(names[order]) if order else pd.Index([], dtype=object))
    fov_values = np.empty(len(rows), dtype=object)
    fov_values[:] = [fov_names[c] for c in fov_codes[rows]]
    out.insert(0, fov_col, fov_values)
    out.insert(1, cell_label_col, ordered[cell_label_col].to_numpy())
    out.insert(2, cell_type_col, ordered[cell_type_col].to_numpy())
    out.to_csv(save_path, index=False)
    return out


# ---- diversity ------------------------------------------------------------------------------------------------------
def _row_diversity(values: np.ndarray) -> np.ndarray:
    """shannon_diversity of every row of ``values`` [n, m], with the bits of the per-row call: the positive entries of a
    row compacted to its front in order, rows grouped by how many they have, and each group reduced along axis 1 -- the
    same pairwise order numpy's sum takes over the compacted 1-d array."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    n = values.shape[0]
    out = np.zeros(n)
    if n and values.shape[1]:
        positive = values > 0
        n_pos = positive.sum(axis=1)
        front = np.argsort(~positive, axis=1, kind="stable")          # the positive columns first, in order
        packed = np.take_along_axis(values, front, axis=1)
        for m in np.unique(n_pos):
            if m == 0:
                continue
            sel = np.flatnonzero(n_pos == m)
            p = np.ascontiguousarray(packed[sel, :m])
            out[sel] = np.sum(p * np.log2(p), axis=1)
    return -out


def shannon_diversity(proportions):
    """The Shannon diversity index ``-sum(p * log2(p))`` over the positive entries of ``proportions``."""
    proportions = np.asarray(proportions)
    prop_index = proportions > 0
    return -np.sum(proportions[prop_index] * np.log2(proportions[prop_index]))


def compute_neighborhood_diversity(neighborhood_mat, cell_type_col):
    """A diversity score per cell of the frequency neighbourhood matrix (``create_neighborhood_matrix``'s second frame).

    Returns ``fov``, ``label``, ``cell_type_col`` and ``diversity_<cell_type_col>``: FOVs in ``np.unique`` order, each
    FOV's rows in the matrix's order under the matrix's index.  Where a label repeats within a FOV every such row gets
    the score of the first, as the reference's lookup by label does.
    """
    verify_in_list(cell_type_column=cell_type_col, neighbor_matrix_columns=neighborhood_mat.columns)
    values = np.array(neighborhood_mat.drop(columns=[_FOV_ID, _CELL_LABEL, cell_type_col]))
    if (values > 1).any():
        raise ValueError("Input must be frequency values.")

    fov_codes, _ = pd.factorize(neighborhood_mat[_FOV_ID].to_numpy(), sort=True)
    rows = np.argsort(fov_codes, kind="stable")
    ordered = neighborhood_mat.iloc[rows]
    scores = _row_diversity(values[rows])
    # the first row of each (FOV, label)
    cell = ordered.groupby([_FOV_ID, _CELL_LABEL], sort=False).ngroup().to_numpy()
    _, first = np.unique(cell, return_index=True)
    scores = scores[first[cell]]
    return pd.DataFrame({_FOV_ID: ordered[_FOV_ID].to_numpy(dtype=object), _CELL_LABEL: ordered[_CELL_LABEL],
                         cell_type_col: ordered[cell_type_col], f"diversity_{cell_type_col}": scores},
                        index=ordered.index)


def generate_neighborhood_diversity_analysis(neighbors_mat_dir, pixel_radius, cell_type_columns):
    """The diversity scores of every cell cluster level of ``cell_type_columns``, read from
    ``neighborhood_freqs-<col>_radius<pixel_radius>.csv`` under ``neighbors_mat_dir`` and merged on ``fov`` and ``label``."""
    freqs_mat_paths = [os.path.join(neighbors_mat_dir, f"neighborhood_freqs-{cell_type_col}_radius{pixel_radius}.csv")
                       for cell_type_col in cell_type_columns]
    validate_paths(freqs_mat_paths)
    diversity_data = [compute_neighborhood_diversity(pd.read_csv(path), cell_type_col)
                      for cell_type_col, path in zip(cell_type_columns, freqs_mat_paths)]
    return reduce(lambda left, right: pd.merge(left, right, on=[_FOV_ID, _CELL_LABEL]), diversity_data)
