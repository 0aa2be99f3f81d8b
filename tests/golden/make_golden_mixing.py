#!/usr/bin/env python
"""Generates tests/golden/g23_mixing.npz: the close-pair tables of the REFERENCE's
ark.analysis.spatial_analysis_utils.compute_close_cell_num and the mixing scores and cell ratios of
ark.analysis.neighborhood_analysis.compute_mixing_score / compute_cell_ratios over its own calc_dist_matrix and
create_neighborhood_matrix, imported from /root/reference/src with tests/golden/_shims, as make_golden_neighborhood.py does.

The stand-ins of that generator are installed into sys.modules here too (each a restatement, so parity with xarray itself
is unpinned), with what these functions need on top: xarray.DataArray takes a dict for ``coords``
(compute_close_cell_num passes ``dist_mat.coords``), seaborn has ``set``, and matplotlib runs on the Agg backend
(compute_cell_ratios draws four figures, which are closed unseen).

The cohort: five FOVs in one table, four marker channels, five phenotypes with numeric ids.
  A   60 cells, rational centroids (sum / count), labels unsorted and not starting at 1, two pairs of coincident cells;
      under cell_count_thresh in every mixing case
  B   a 15 x 15 integer grid of pitch 10: pairs at exactly 50 must not count at dist_lim 50; phenotype CD8T is absent
  C   200 cells, four tumor cells in five: over ratio_threshold
  D   300 cells on a 1200 wide field: a fifth of them have no neighbour within 50 and leave the neighbourhood matrix, so
      the populations of the mixing score are counted without them
  E   270 cells inside a disc of radius 15, all positive for chanA: every pair is within 37.5, the true chanA x chanA
      count is 270 * 269 = 72 630 and the reference's uint16 entry must be 72 630 - 65 536 = 7 094 (asserted here)
The close-pair cases vary FOV, analysis type (channel, cluster) and dist_lim (int 50, float 37.5); the mixing cases vary
the populations, mixing type, distlim, self_neighbor and the two thresholds.

    python tests/golden/make_golden_mixing.py      (needs /root/reference; never runs on the GPU box)
    PXSOM_GOLDEN_OUT=<dir> ... writes to <dir> instead, to compare a regeneration with the committed file.
"""
import os
import sys
import tempfile
import types
import warnings

import matplotlib

matplotlib.use("Agg")

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

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
        if isinstance(coords, dict):
            dims = tuple(coords) if dims is None else dims
            coords = [coords[d] for d in dims]
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
_module("seaborn", set=lambda *args, **kwargs: None)
_module("statsmodels")
_module("statsmodels.stats")
_module("statsmodels.stats.multitest", multipletests=None)
_module("tqdm.notebook", tqdm=_Progress)

import matplotlib.pyplot as plt  # noqa: E402

from ark.analysis import neighborhood_analysis as ref_na  # noqa: E402
from ark.analysis import spatial_analysis_utils as ref_sau  # noqa: E402

PHENOTYPES = ["tumor", "CD4T", "CD8T", "stroma", "B cell"]
PHENOTYPE_IDS = {name: i + 1 for i, name in enumerate(PHENOTYPES)}
CHANNELS = ["chanA", "chanB", "chanC", "chanD"]
THRESHOLDS = [0.5, 1.0, 0.2, 2.0]
COLUMNS = ["cell_size"] + CHANNELS + ["label", "fov", "centroid-0", "centroid-1", "cell_meta_cluster",
                                      "cell_meta_cluster_id"]
FOVS = ["fovA", "fovB", "fovC", "fovD", "fovE"]
WRAP_FOV, WRAP_CELLS = "fovE", 270

# (FOV, analysis type, dist_lim)
CLOSE_CASES = [("fovA", "channel", 50), ("fovA", "cluster", 37.5), ("fovB", "channel", 50), ("fovB", "cluster", 50),
               ("fovB", "channel", 37.5), ("fovC", "cluster", 50), ("fovC", "channel", 37.5), ("fovD", "channel", 50),
               ("fovD", "cluster", 37.5), ("fovE", "channel", 37.5), ("fovE", "cluster", 50), ("fovE", "channel", 50)]
# (target, reference, mixing type, distlim, self_neighbor, ratio_threshold, cell_count_thresh)
MIXING_CASES = [
    (["CD4T", "CD8T"], ["tumor"], "homogeneous", 50, False, 5, 100),
    (["CD4T", "CD8T"], ["tumor"], "percent", 37.5, True, 5, 100),
    (["tumor"], ["stroma", "B cell"], "percent", 50, True, 5, 150),
    (["CD8T"], ["CD4T"], "homogeneous", 37.5, False, 2, 20),
]


# ---- the cohort ---------------------------------------------------------------------------------------------------
def _fov(rs, name, xy, labels, phenotypes, p=None):
    n = len(xy)
    df = pd.DataFrame({"cell_size": rs.randint(20, 200, n)})
    for ch in CHANNELS:
        df[ch] = np.round(rs.gamma(0.7, 2.0, n) * 16) / 16        # sixteenths: the file stays small
    df["label"] = labels
    df["fov"] = name
    df["centroid-0"], df["centroid-1"] = xy[:, 0], xy[:, 1]
    df["cell_meta_cluster"] = rs.choice(phenotypes, n, p=p)
    df["cell_meta_cluster_id"] = df["cell_meta_cluster"].map(PHENOTYPE_IDS).astype(np.int64)
    return df[COLUMNS]


def cohort(rs):
    xy_a = np.stack([rs.randint(0, 12000, 60) / rs.randint(20, 80, 60), rs.randint(0, 12000, 60) / rs.randint(20, 80, 60)], 1)
    xy_a[17], xy_a[41] = xy_a[5], xy_a[40]        # coincident cells
    a = _fov(rs, "fovA", xy_a, rs.permutation(np.arange(7, 7 + 3 * 60, 3)), PHENOTYPES)
    gy, gx = np.mgrid[0:15, 0:15]
    xy_b = np.stack([gy.ravel(), gx.ravel()], 1) * 10
    b = _fov(rs, "fovB", xy_b, np.arange(1, 226), PHENOTYPES[:2] + PHENOTYPES[3:])
    c = _fov(rs, "fovC", rs.uniform(0, 400, (200, 2)), rs.permutation(200) + 100, PHENOTYPES[:4], p=[0.8, 0.05, 0.05, 0.1])
    d = _fov(rs, "fovD", rs.uniform(0, 1200, (300, 2)), rs.permutation(300) + 2, PHENOTYPES)
    radius, angle = 15 * np.sqrt(rs.uniform(0, 1, WRAP_CELLS)), rs.uniform(0, 2 * np.pi, WRAP_CELLS)
    e = _fov(rs, "fovE", np.stack([500 + radius * np.cos(angle), 500 + radius * np.sin(angle)], 1),
             rs.permutation(WRAP_CELLS) + 1, PHENOTYPES)
    e["chanA"] = e["chanA"] + 5.0                 # every cell of the disc is positive for chanA
    d32 = np.sqrt(((xy_b[:, None, :] - xy_b[None, :, :]) ** 2).sum(-1).astype(np.float64)).astype(np.float32)
    assert int((d32 == 50).sum()) > 1000, int((d32 == 50).sum())
    return pd.concat([a, b, c, d, e], ignore_index=True)


def store_frame(out, prefix, df):
    out[prefix + "columns"] = np.array([str(c) for c in df.columns])
    out[prefix + "dtypes"] = np.array([str(t) for t in df.dtypes])
    for i, col in enumerate(df.columns):
        v = df[col].to_numpy()
        out[prefix + "col%d" % i] = v.astype(str) if v.dtype == object else v
    idx = np.asarray(df.index)
    out[prefix + "index"] = idx.astype(str) if idx.dtype == object else idx.astype(np.int64)


def run_close_case(i, spec, master, dist_mats, out):
    fov, analysis, dist_lim = spec
    rows = master[master["fov"] == fov]
    if analysis == "channel":
        close_num, mark1_num, poslabels = ref_sau.compute_close_cell_num(
            dist_mats[fov], dist_lim, "channel", current_fov_data=rows, current_fov_channel_data=rows[CHANNELS],
            thresh_vec=np.array(THRESHOLDS))
    else:
        close_num, mark1_num, poslabels = ref_sau.compute_close_cell_num(
            dist_mats[fov], dist_lim, "cluster", current_fov_data=rows,
            cluster_ids=np.array([PHENOTYPE_IDS[p] for p in PHENOTYPES]), cell_type_col="cell_meta_cluster_id")
    assert close_num.dtype == np.uint16 and [len(p) for p in poslabels] == list(mark1_num)
    p = "k%d_" % i
    out[p + "fov"], out[p + "analysis"], out[p + "dist_lim"] = np.array(fov), np.array(analysis), np.array(dist_lim)
    out[p + "close_num"] = close_num
    out[p + "mark1_num"] = np.asarray(mark1_num, dtype=np.int64)
    out[p + "poslabels"] = np.concatenate([np.asarray(s.values, dtype=np.int64) for s in poslabels])
    out[p + "posindex"] = np.concatenate([np.asarray(s.index, dtype=np.int64) for s in poslabels])
    return close_num


def run_mixing_case(i, spec, master, out):
    target, reference, mixing_type, distlim, self_neighbor, ratio_threshold, cell_count_thresh = spec
    with tempfile.TemporaryDirectory() as td:
        ref_sau.calc_dist_matrix(master, td)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            neighbors, _ = ref_na.create_neighborhood_matrix(master, td, distlim=distlim, self_neighbor=self_neighbor)
    scores, counts = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # 0 / 0 in the reference's quotient
        for fov in FOVS:
            score, count = ref_na.compute_mixing_score(neighbors[neighbors["fov"] == fov], target, reference, mixing_type,
                                                       ratio_threshold=ratio_threshold,
                                                       cell_count_thresh=cell_count_thresh)
            scores.append(score)
            counts.append(count)
    ratios = ref_na.compute_cell_ratios(neighbors, target, reference, FOVS)
    plt.close("all")
    p = "m%d_" % i
    out[p + "target"], out[p + "reference"] = np.array(target), np.array(reference)
    out[p + "mixing_type"], out[p + "distlim"] = np.array(mixing_type), np.array(distlim)
    out[p + "self_neighbor"] = np.array(self_neighbor)
    out[p + "ratio_threshold"], out[p + "cell_count_thresh"] = np.array(ratio_threshold), np.array(cell_count_thresh)
    out[p + "scores"] = np.asarray(scores, dtype=np.float64)
    out[p + "counts"] = np.asarray(counts, dtype=np.int64)
    store_frame(out, p + "ratios_", ratios)
    return np.asarray(scores, dtype=np.float64), np.asarray(counts), len(neighbors)


def main():
    rs = np.random.RandomState(23)
    master = cohort(rs)
    out = {"n_close": np.array(len(CLOSE_CASES)), "n_mixing": np.array(len(MIXING_CASES)), "fovs": np.array(FOVS),
           "channels": np.array(CHANNELS), "thresholds": np.array(THRESHOLDS), "phenotypes": np.array(PHENOTYPES),
           "phenotype_ids": np.array([PHENOTYPE_IDS[p] for p in PHENOTYPES], dtype=np.int64)}
    store_frame(out, "master_", master)

    dist_mats = {}
    with tempfile.TemporaryDirectory() as td:
        ref_sau.calc_dist_matrix(master, td)
        for fov in FOVS:
            dist_mats[fov] = load_dataarray(os.path.join(td, fov + "_dist_mat.xr"))
    wrapped = 0
    for i, spec in enumerate(CLOSE_CASES):
        close_num = run_close_case(i, spec, master, dist_mats, out)
        if spec[0] == WRAP_FOV and spec[1] == "channel":
            true = WRAP_CELLS * (WRAP_CELLS - 1)
            assert true > 65535 and int(close_num[0, 0]) == true % 65536 == true - 65536, (int(close_num[0, 0]), true)
            wrapped += 1
    assert wrapped == 2
    out["wrap_true_count"] = np.array(WRAP_CELLS * (WRAP_CELLS - 1))

    seen_nan, seen_score, dropped = 0, 0, False
    for i, spec in enumerate(MIXING_CASES):
        scores, counts, kept = run_mixing_case(i, spec, master, out)
        seen_nan += int(np.isnan(scores).sum())
        seen_score += int(np.isfinite(scores).sum())
        dropped |= kept < len(master)
    assert seen_nan >= 4 and seen_score >= 6 and dropped, (seen_nan, seen_score, dropped)

    path = os.path.join(OUT_DIR, "g23_mixing.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, ROOT), len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
