"""What the cell-geometry functions of this package share: a cohort's rows FOV by FOV, the centroid columns of a cell
table, a host array's way to the device.  Imports neither torch nor the library before a device is asked for."""
import numpy as np


def fov_rows_and_segments(codes, n_fovs):
    """From an integer FOV code per table row (-1: not wanted): the wanted rows FOV by FOV, each FOV's in table order,
    and ``seg`` [n_fovs + 1] int64 with FOV f at ``rows[seg[f]:seg[f + 1]]`` (empty for a FOV without rows)."""
    codes = np.asarray(codes)
    rows = np.flatnonzero(codes >= 0)
    rows = rows[np.argsort(codes[rows], kind="stable")]
    seg = np.concatenate([[0], np.cumsum(np.bincount(codes[rows], minlength=n_fovs))]).astype(np.int64)
    return rows, seg


def centroid_columns(table, centroid_cols, who, table_name="cell_table"):
    """The names of the two centroid columns of ``table``, checked; ``who`` and ``table_name`` word the error."""
    missing = [c for c in centroid_cols if c not in table.columns]
    if len(centroid_cols) != 2 or missing:
        raise ValueError("%s needs two centroid columns in %s; missing: %s (pass centroid_cols=... if they are named "
                         "differently)" % (who, table_name, missing or list(centroid_cols)))
    return list(centroid_cols)


def _to_device(array, dtype):
    """``array`` as a contiguous HBM tensor of ``dtype`` on the current device; RuntimeError without one."""
    import torch
    from .. import _capi
    return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype)).to(_capi.require_gpu())
