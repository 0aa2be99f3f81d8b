#!/usr/bin/env python
"""Generates tests/golden/g19_cell_distances.npz: the frames of the REFERENCE's
ark.analysis.cell_neighborhood_stats.generate_cell_distance_analysis, compute_neighborhood_diversity and
generate_neighborhood_diversity_analysis, over the matrices of ark.analysis.spatial_analysis_utils.calc_dist_matrix and the
frequency tables of ark.analysis.neighborhood_analysis.create_neighborhood_matrix, imported from /root/reference/src with
tests/golden/_shims, as make_golden_neighborhood.py does.

xarray, statsmodels, seaborn and tqdm's notebook front end are absent from this image.  The stand-ins below are installed
into sys.modules from this generator (the files under _shims stay as they are); each is a restatement, so parity with
xarray itself is unpinned:
  - xarray.DataArray(data, coords=[...]) with the default dims dim_0 / dim_1, .values, .coords, .shape, len(),
    .loc[list, list] (label lookup per axis, the first match) and .loc[:, boolean mask], .dim_1.isin(labels) (a boolean
    mask over the second axis' coordinate), ``> scalar`` (a boolean DataArray), .where(condition) (NaN where it is False,
    the dtype kept), to_netcdf / xarray.load_dataarray (a round trip through one .npz file: the float32 matrix comes back
    bit for bit);
  - statsmodels.stats.multitest.multipletests, seaborn: imported only, never called here;
  - tqdm.notebook.tqdm / tqdm.auto.tqdm: a context manager with set_postfix / update that prints nothing.

The cohort: four FOVs in one table, each cell with two phenotype columns (cell_meta_cluster: 5 names, cell_cluster: 9).
  A  60 cells, rational centroids (sum / count), labels unsorted and not starting at 1, two pairs of coincident cells
  B  a 15 x 15 integer grid of pitch 3: distances 3, 6, 9 ... and the 3-4-5 multiples, every one tied many times over;
     one phenotype is absent from it
  C  64 cells whose phenotypes have 4, 5, 8, 13 and 34 members: at k = 5, 8 and 13 one phenotype has exactly k cells (a
     cell of it has k - 1 others: NaN for its own phenotype) and another fewer than k (NaN for every cell)
  D  50 cells, float centroids
The cases vary k over 1, 5, 8 and 13 (8 and 13 take numpy's eight-accumulator order), the order of the FOVs in the table
and the column names (one case has renamed columns and a shuffled index).  The diversity frames come from the
frequency tables of both phenotype columns at radius 50.

    python tests/golden/make_golden_cell_distances.py      (needs /root/reference; never runs on the GPU box)
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
class _Coord:
    def __init__(self, values):
        self.values = np.asarray(values)

    def isin(self, labels):
        return np.isin(self.values, np.asarray(labels))


class _Loc:
    def __init__(self, owner):
        self._o = owner

    def __getitem__(self, key):
        key = key if isinstance(key, tuple) else (key,)
        pos = []
        for d, k in zip(self._o.dims, key):
            n = len(self._o.coords[d])
            if isinstance(k, slice):
                assert k == slice(None)
                pos.append(np.arange(n))
            elif np.asarray(k).dtype == bool:
                pos.append(np.flatnonzero(np.asarray(k)))
            else:
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

    @property
    def shape(self):
        return self.values.shape

    def __len__(self):
        return len(self.values)

    def __getattr__(self, name):
        if name.startswith("dim_") and name in self.__dict__.get("coords", {}):
            return _Coord(self.coords[name])
        raise AttributeError(name)

    def __gt__(self, other):
        return DataArray(self.values > other, coords=[self.coords[d] for d in self.dims], dims=self.dims)

    def where(self, cond):
        nan = self.values.dtype.type(np.nan)
        return DataArray(np.where(cond.values, self.values, nan), coords=[self.coords[d] for d in self.dims],
                         dims=self.dims)

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
_module("tqdm.auto", tqdm=_Progress)

from ark.analysis import cell_neighborhood_stats as ref_cns  # noqa: E402
from ark.analysis import neighborhood_analysis as ref_na  # noqa: E402
from ark.analysis import spatial_analysis_utils as ref_sau  # noqa: E402

PHENOTYPES = ["tumor", "CD4T", "CD8T", "stroma", "B cell"]
FINE = ["t1", "t2", "t3", "cd4a", "cd4b", "cd8", "fibro", "endo", "b"]
COLUMNS = ["cell_size", "label", "fov", "centroid-0", "centroid-1", "cell_meta_cluster", "cell_cluster"]
RENAMED = {"fov": "sample", "label": "cell_id", "cell_meta_cluster": "pheno", "centroid-0": "cy", "centroid-1": "cx"}
C_MEMBERS = [4, 5, 8, 13, 34]       # fovC's cells per phenotype, in PHENOTYPES order
RADIUS = 50


# ---- the cohort ---------------------------------------------------------------------------------------------------
def _fov(rs, name, xy, labels, phenotypes):
    n = len(xy)
    df = pd.DataFrame({"cell_size": rs.randint(20, 200, n)})
    df["label"] = labels
    df["fov"] = name
    df["centroid-0"], df["centroid-1"] = xy[:, 0], xy[:, 1]
    df["cell_meta_cluster"] = phenotypes
    df["cell_cluster"] = rs.choice(FINE, n)
    return df[COLUMNS]


def cohort(rs):
    xy_a = np.stack([rs.randint(0, 12000, 60) / rs.randint(20, 80, 60), rs.randint(0, 12000, 60) / rs.randint(20, 80, 60)], 1)
    xy_a[17], xy_a[41] = xy_a[5], xy_a[40]        # coincident cells
    a = _fov(rs, "fovA", xy_a, rs.permutation(np.arange(7, 7 + 3 * 60, 3)), rs.choice(PHENOTYPES, 60))
    gy, gx = np.mgrid[0:15, 0:15]
    xy_b = np.stack([gy.ravel(), gx.ravel()], 1) * 3
    b = _fov(rs, "fovB", xy_b, np.arange(1, 226), rs.choice(PHENOTYPES[:2] + PHENOTYPES[3:], 225))
    pheno_c = rs.permutation(np.repeat(PHENOTYPES, C_MEMBERS))
    c = _fov(rs, "fovC", rs.uniform(0, 400, (64, 2)), rs.permutation(64) + 100, pheno_c)
    d = _fov(rs, "fovD", rs.uniform(0, 300, (50, 2)), rs.permutation(50) + 2, rs.choice(PHENOTYPES, 50))
    return pd.concat([a, b, c, d], ignore_index=True)


CASES = [
    # (FOVs of the table, k, renamed columns and a shuffled index)
    (["fovA", "fovB", "fovC", "fovD"], 1, False),
    (["fovA", "fovB", "fovC", "fovD"], 5, False),
    (["fovD", "fovC", "fovB", "fovA"], 8, False),
    (["fovC", "fovA", "fovB", "fovD"], 13, False),
    (["fovB", "fovD", "fovA"], 5, True),
]
DIVERSITY_FOVS, DIVERSITY_COLUMNS = ["fovA", "fovB", "fovD"], ["cell_meta_cluster", "cell_cluster"]


def case_table(master, spec, rs_seed):
    fovs, _, renamed = spec
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
    fovs, k, renamed = spec
    table = case_table(master, spec, i)
    names = {key: RENAMED[key] if renamed else key for key in RENAMED}
    with tempfile.TemporaryDirectory() as td:
        ref_sau.calc_dist_matrix(table, td, fov_id=names["fov"], label_id=names["label"],
                                 centroid_ids=(names["centroid-0"], names["centroid-1"]))
        save_path = os.path.join(td, "cell_dists.csv")
        dists = ref_cns.generate_cell_distance_analysis(table, td, save_path, k, cell_type_col=names["cell_meta_cluster"],
                                                        fov_col=names["fov"], cell_label_col=names["label"])
        saved = pd.read_csv(save_path)
    p = "c%d_" % i
    out[p + "fovs"] = np.array(fovs)
    out[p + "k"] = np.array(k)
    out[p + "renamed"] = np.array(renamed)
    store_frame(out, p + "dists_", dists)
    store_frame(out, p + "saved_", saved)


def run_diversity(master, out):
    table = pd.concat([master[master["fov"] == f] for f in DIVERSITY_FOVS], ignore_index=True)
    with tempfile.TemporaryDirectory() as td:
        ref_sau.calc_dist_matrix(table, td)
        for col in DIVERSITY_COLUMNS:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _, freqs = ref_na.create_neighborhood_matrix(table, td, distlim=RADIUS, cell_type_col=col)
            freqs.to_csv(os.path.join(td, "neighborhood_freqs-%s_radius%d.csv" % (col, RADIUS)), index=False)
            store_frame(out, "d_freqs_%s_" % col, freqs)
            store_frame(out, "d_single_%s_" % col, ref_cns.compute_neighborhood_diversity(freqs, col))
        merged = ref_cns.generate_neighborhood_diversity_analysis(td, RADIUS, DIVERSITY_COLUMNS)
    out["d_columns"] = np.array(DIVERSITY_COLUMNS)
    out["d_radius"] = np.array(RADIUS)
    store_frame(out, "d_merged_", merged)


def main():
    rs = np.random.RandomState(19)
    master = cohort(rs)
    out = {"n_cases": np.array(len(CASES)), "c_members": np.array(C_MEMBERS)}
    store_frame(out, "master_", master)
    for i, spec in enumerate(CASES):
        run_case(i, spec, master, out)
    run_diversity(master, out)
    path = os.path.join(OUT_DIR, "g19_cell_distances.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, ROOT), len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
