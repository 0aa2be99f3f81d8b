#!/usr/bin/env python
"""Generates tests/golden/g18_neighborhood.npz: the neighbourhood matrices of the REFERENCE's
ark.analysis.spatial_analysis_utils.calc_dist_matrix + ark.analysis.neighborhood_analysis.create_neighborhood_matrix, and
the three tables of generate_cluster_matrix_results, imported from /root/reference/src with tests/golden/_shims, as
make_golden_cell_table.py does.

xarray, statsmodels, seaborn and tqdm's notebook front end are absent from this image.  The stand-ins below are installed
into sys.modules from this generator (the files under _shims stay as they are); each is a restatement, so parity with
xarray itself is unpinned:
  - xarray.DataArray(data, coords=[...]) with the default dims dim_0 / dim_1, .values, .coords, .loc[list, list] (label
    lookup per axis, the first match), to_netcdf / xarray.load_dataarray (a round trip through one .npz file: values,
    dims and coords come back as written, the float32 matrix bit for bit);
  - statsmodels.stats.multitest.multipletests, seaborn: imported only, never called here;
  - tqdm.notebook.tqdm: a context manager with set_postfix / update that prints nothing.

The cohort: four FOVs in one table.
  A  60 cells, rational centroids (sum / count), labels unsorted and not starting at 1, two pairs of coincident cells
  B  a 20 x 20 integer grid of pitch 10: 3 376 ordered pairs lie at exactly 50 and must not count at distlim 50; one
     phenotype is absent from it
  C  40 cells on a 40 000 wide field: most have no neighbour within 50 (the 5 % warning)
  D  50 cells, float centroids
The cases vary the FOVs in the table, included_fovs, distlim (int 50, float 37.5), self_neighbor and the column names.
The k-means labels the reference produced on this machine are stored; the tests inject them (k-means labels are not
compared across machines).

    python tests/golden/make_golden_neighborhood.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed file.
"""
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(0, "/root/reference/src")

OUT_DIR = os.environ.get("PXSOM_GOLDEN_OUT", HERE)


# ---- xarray -------------------------------------------------------------------------------------------------------
class _Loc:
    def __init__(self, owner):
        self._o = owner

    def __getitem__(self, key):
        key = key if isinstance(key, tuple) else (key,)
        pos = []
        for d, k in zip(self._o.dims, key):
            first = {}
            for p, v in enumerate(self._o.coords[d].tolist()):
                first.setdefault(v, p)
            pos.append([first[v] for v in np.asarray(k).tolist()])
        return DataArray(self._o.values[np.ix_(*pos)],
                         coords=[self._o.coords[d][p] for d, p in zip(self._o.dims, pos)], dims=self._o.dims)


class DataArray:
    def __init__(self, data, coords=None, dims=None):
        self.values = np.asarray(data)
        self.dims = tuple(dims) if dims is not None else tuple("dim_%d" % i for i in range(self.values.ndim))
        self.coords = {d: np.asarray(c) for d, c in zip(self.dims, coords)}

    @property
    def loc(self):
        return _Loc(self)

    def to_netcdf(self, path, format=None):
        with open(path, "wb") as f:
            np.savez(f, values=self.values, dims=np.array(self.dims), **{"coord_" + d: c for d, c in self.coords.items()})


def load_dataarray(path):
    with np.load(path, allow_pickle=False) as z:
        dims = [str(d) for d in z["dims"]]
        return DataArray(z["values"], coords=[z["coord_" + d] for d in dims], dims=dims)


class _Progress:
    def __init__(self, *args, **kwargs):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def set_postfix(self, **kwargs):
        pass

    def update(self, n=1):
        pass


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_module("xarray", DataArray=DataArray, load_dataarray=load_dataarray)
_module("seaborn")
_module("statsmodels")
_module("statsmodels.stats")
_module("statsmodels.stats.multitest", multipletests=None)
_module("tqdm.notebook", tqdm=_Progress)

from ark.analysis import neighborhood_analysis as ref_na  # noqa: E402
from ark.analysis import spatial_analysis_utils as ref_sau  # noqa: E402

PHENOTYPES = ["tumor", "CD4T", "CD8T", "stroma", "B cell"]
CHANNELS = ["chanA", "chanB", "chanC"]
COLUMNS = ["cell_size"] + CHANNELS + ["label", "fov", "centroid-0", "centroid-1", "cell_meta_cluster"]
RENAMED = {"fov": "sample", "label": "cell_id", "cell_meta_cluster": "pheno", "centroid-0": "cy", "centroid-1": "cx"}
TIE_PAIRS = 3376      # ordered pairs of the 20 x 20 pitch-10 grid at distance exactly 50


# ---- the cohort ---------------------------------------------------------------------------------------------------
def _fov(rs, name, xy, labels, phenotypes):
    n = len(xy)
    df = pd.DataFrame({"cell_size": rs.randint(20, 200, n)})
    for ch in CHANNELS:
        df[ch] = rs.gamma(0.7, 2.0, n)
    df["label"] = labels
    df["fov"] = name
    df["centroid-0"], df["centroid-1"] = xy[:, 0], xy[:, 1]
    df["cell_meta_cluster"] = rs.choice(phenotypes, n)
    return df[COLUMNS]


def cohort(rs):
    xy_a = np.stack([rs.randint(0, 12000, 60) / rs.randint(20, 80, 60), rs.randint(0, 12000, 60) / rs.randint(20, 80, 60)], 1)
    xy_a[17], xy_a[41] = xy_a[5], xy_a[40]        # coincident cells
    a = _fov(rs, "fovA", xy_a, rs.permutation(np.arange(7, 7 + 3 * 60, 3)), PHENOTYPES)
    gy, gx = np.mgrid[0:20, 0:20]
    xy_b = np.stack([gy.ravel(), gx.ravel()], 1) * 10
    b = _fov(rs, "fovB", xy_b, np.arange(1, 401), PHENOTYPES[:2] + PHENOTYPES[3:])
    c = _fov(rs, "fovC", rs.uniform(0, 40000, (40, 2)), rs.permutation(40) + 100, PHENOTYPES)
    d = _fov(rs, "fovD", rs.uniform(0, 300, (50, 2)), rs.permutation(50) + 2, PHENOTYPES)
    d32 = np.sqrt(((xy_b[:, None, :] - xy_b[None, :, :]) ** 2).sum(-1).astype(np.float64)).astype(np.float32)
    assert int((d32 == 50).sum()) == TIE_PAIRS, int((d32 == 50).sum())
    return pd.concat([a, b, c, d], ignore_index=True)


CASES = [
    # (FOVs of the table, included_fovs, distlim, self_neighbor, renamed columns and a shuffled index)
    (["fovA", "fovB", "fovD"], None, 50, False, False),
    (["fovA", "fovB", "fovD"], None, 37.5, True, False),
    (["fovA", "fovB", "fovC", "fovD"], None, 50, False, False),
    (["fovA", "fovB", "fovC", "fovD"], ["fovD", "fovA"], 50, True, False),
    (["fovB", "fovD", "fovA"], None, 37.5, False, True),
]
CLUSTER_CASE, CLUSTER_NUM, CLUSTER_SEED, CLUSTER_EXCLUDED = 0, 3, 42, ["chanB"]


def case_table(master, spec, rs_seed):
    fovs, _, _, _, renamed = spec
    table = pd.concat([master[master["fov"] == f] for f in fovs], ignore_index=True)
    if renamed:
        table = table.rename(columns=RENAMED)
        table.index = np.random.RandomState(rs_seed).permutation(len(table)) + 1000
    return table


def store_frame(out, prefix, df):
    out[prefix + "columns"] = np.array([str(c) for c in df.columns])
    out[prefix + "dtypes"] = np.array([str(t) for t in df.dtypes])
    for i, col in enumerate(df.columns):
        v = df[col].to_numpy()
        out[prefix + "col%d" % i] = v.astype(str) if v.dtype == object else v
    idx = np.asarray(df.index)
    out[prefix + "index"] = idx.astype(str) if idx.dtype == object else idx.astype(np.int64)


def run_case(i, spec, master, out):
    fovs, included, distlim, self_neighbor, renamed = spec
    table = case_table(master, spec, i)
    names = {k: RENAMED[k] if renamed else k for k in RENAMED}
    with tempfile.TemporaryDirectory() as td:
        ref_sau.calc_dist_matrix(table, td, fov_id=names["fov"], label_id=names["label"],
                                 centroid_ids=(names["centroid-0"], names["centroid-1"]))
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter("always")
            counts, freqs = ref_na.create_neighborhood_matrix(
                table, td, included_fovs=included, distlim=distlim, self_neighbor=self_neighbor, fov_col=names["fov"],
                cell_label_col=names["label"], cell_type_col=names["cell_meta_cluster"])
    p = "c%d_" % i
    out[p + "fovs"] = np.array(fovs)
    out[p + "included"] = np.array(included if included is not None else [], dtype=str)
    out[p + "included_none"] = np.array(included is None)
    out[p + "distlim"] = np.array(distlim)          # int64 for 50, float64 for 37.5: the tests pass a Python scalar
    out[p + "self_neighbor"] = np.array(self_neighbor)
    out[p + "renamed"] = np.array(renamed)
    out[p + "warnings"] = np.array([str(w.message) for w in wl if issubclass(w.category, UserWarning)], dtype=str)
    store_frame(out, p + "counts_", counts)
    store_frame(out, p + "freqs_", freqs)
    return table, counts


def main():
    rs = np.random.RandomState(18)
    master = cohort(rs)
    out = {"n_cases": np.array(len(CASES)), "tie_pairs": np.array(TIE_PAIRS)}
    store_frame(out, "master_", master)
    kept = {}
    for i, spec in enumerate(CASES):
        kept[i] = run_case(i, spec, master, out)

    table, counts = kept[CLUSTER_CASE]
    labels = []
    real = ref_sau.generate_cluster_labels

    def recording(*args, **kwargs):
        labels.append(real(*args, **kwargs))
        return labels[-1]
    ref_sau.generate_cluster_labels = recording
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # the reference assigns into a slice (SettingWithCopyWarning)
        frames = ref_na.generate_cluster_matrix_results(table, counts, CLUSTER_NUM, seed=CLUSTER_SEED,
                                                        excluded_channels=CLUSTER_EXCLUDED)
    ref_sau.generate_cluster_labels = real
    out["k_case"], out["k_num"], out["k_seed"] = np.array(CLUSTER_CASE), np.array(CLUSTER_NUM), np.array(CLUSTER_SEED)
    out["k_excluded"] = np.array(CLUSTER_EXCLUDED)
    out["k_labels"] = np.asarray(labels[0])        # int32, as scikit-learn returns them
    for tag, df in zip(("cells", "per_type", "means"), frames):
        store_frame(out, "k_%s_" % tag, df)

    path = os.path.join(OUT_DIR, "g18_neighborhood.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, ROOT), len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
