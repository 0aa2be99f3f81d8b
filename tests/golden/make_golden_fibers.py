#!/usr/bin/env python
"""Generates tests/golden/g26_fibers.npz: the alignment scores, densities and FOV / tile summaries of the REFERENCE's
ark.segmentation.fiber_segmentation (calculate_fiber_alignment, calculate_density, generate_tile_stats through
generate_summary_stats), imported from /root/reference/src with tests/golden/_shims.

The reference module imports names it never calls on these paths -- skimage's exposure, filters, measure, morphology and
segmentation functions, tqdm, and ark.utils.plot_utils, which pulls in xarray and the plotting stack.  Stand-ins for
them go into sys.modules here, as make_golden_mixing.py does; ``_shims`` stays as it is.  What the recorded functions do
call is real: numpy, pandas, scipy's cdist, and skimage.io.imread (the Pillow shim) for the label files.

Alignment cases: one table of eight FOVs with 0, 1, 3, 9, 10, 33, 70 and 300 qualifying fibres (major / minor >= 2), the
rows of all FOVs shuffled together, rational centroids (integer / integer), labels unsorted with gaps; every FOV also
holds fibres that do not qualify (ratio 1.5, and 0 / 0, which numpy's comparison drops) and, from three qualifying
fibres on, one with minor_axis_length 0 (x / 0 = inf, kept).  The table runs with k = 1, 2, 4, 8, 9 and 32; the
reference test's own four-fibre table runs with the same k.  The reference orders neighbours by an unstable argsort of
cdist's row, which is well defined only without ties: this generator ASSERTS that the k + 2 smallest distances of every
row differ by more than 1e-9 relative.

Summary cases: (cohort, tile_length, min_fiber_num) over a small cohort (32 x 32 and 16 x 16 label planes, tile 8) and a
large one (512 x 512 and 1024 x 1024, tile 512), min_fiber_num 1 and 5.  The tables of these cohorts are synthetic
(regionprops_table is skimage's and is not on this machine), their alignment scores the reference's; the label planes
hold a few rectangles and give the functions what they read of them, the side length.

    python tests/golden/make_golden_fibers.py      (needs /root/reference; never runs on the GPU box)
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


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


# imported by the reference module, never called by what is recorded here
_module("skimage.exposure", equalize_adapthist=None)
_module("skimage.filters", frangi=None, sobel=None, threshold_multiotsu=None)
_module("skimage.measure", regionprops_table=None)
_module("skimage.morphology", remove_small_objects=None)
import skimage.segmentation  # noqa: E402  (the shim package)

if not hasattr(skimage.segmentation, "watershed"):
    skimage.segmentation.watershed = None
_module("tqdm.auto", tqdm=None)
_module("ark.utils.plot_utils", set_minimum_color_for_colormap=None)

with warnings.catch_warnings():
    warnings.simplefilter("ignore")          # scipy.ndimage.morphology is a deprecated namespace
    from ark.segmentation import fiber_segmentation as ref_fs  # noqa: E402

from scipy.spatial.distance import cdist  # noqa: E402

from ark_analysis_amd import image_io  # noqa: E402

K_VALUES = [1, 2, 4, 8, 9, 32]
QUALIFYING = [0, 1, 3, 9, 10, 33, 70, 300]
ALIGN_COLUMNS = ["fov", "label", "centroid-0", "centroid-1", "major_axis_length", "minor_axis_length", "orientation"]
PROPERTIES = ["major_axis_length", "minor_axis_length", "orientation", "area", "eccentricity", "euler_number"]
# (cohort, tile_length, min_fiber_num)
SUMMARY_CASES = [("small", 8, 1), ("small", 8, 5), ("large", 512, 1), ("large", 512, 5)]
COHORTS = {"small": [("s1", 32, 40), ("s2", 16, 9)], "large": [("l1", 512, 60), ("l2", 1024, 200)]}


def store_frame(out, prefix, df):
    out[prefix + "columns"] = np.array([str(c) for c in df.columns])
    for i, col in enumerate(df.columns):
        v = df[col].to_numpy()
        out[prefix + "col%d" % i] = v.astype(str) if v.dtype == object else v


def rational(rs, n, top):
    """n quotients of integers in [0, top)"""
    return rs.randint(0, top * 20, n) / rs.randint(20, 80, n)


def alignment_table(rs):
    frames = []
    for f, q in enumerate(QUALIFYING):
        extra = 4 + f
        n = q + extra
        major = np.concatenate([rs.uniform(20, 60, q), rs.uniform(6, 9, extra)])
        minor = np.concatenate([major[:q] / rs.uniform(2.5, 8, q), major[q:] / 1.5])
        if q >= 3:
            minor[1] = 0.0                       # x / 0 = inf: kept
        major[q], minor[q] = 0.0, 0.0            # 0 / 0 = nan: dropped
        frames.append(pd.DataFrame({
            "fov": "fov%d" % f, "label": rs.permutation(np.arange(3, 3 + 2 * n, 2)),
            "centroid-0": rational(rs, n, 2000), "centroid-1": rational(rs, n, 2000),
            "major_axis_length": major, "minor_axis_length": minor,
            "orientation": rs.uniform(-np.pi / 2, np.pi / 2, n)}))
    table = pd.concat(frames, ignore_index=True)
    return table.iloc[rs.permutation(len(table))].reset_index(drop=True)[ALIGN_COLUMNS]


def reference_test_table():
    return pd.DataFrame({"fov": ["fov1"] * 4, "label": [1, 2, 3, 4], "orientation": [-30, -15, 15, 0],
                         "centroid-0": [0, 3, 1, 2], "centroid-1": [0, 3, 3, 2],
                         "major_axis_length": [2, 2, 2, 1.5], "minor_axis_length": [1, 1, 1, 1]})


def assert_no_ties(table, k):
    """Every row's k + 2 smallest cdist values (itself included) differ by more than 1e-9 relative."""
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = (table["major_axis_length"].values / table["minor_axis_length"].values) >= 2
    kept = table[keep]
    for fov in np.unique(kept.fov):
        rows = kept[kept.fov == fov]
        xy = np.vstack((rows["centroid-0"].values, rows["centroid-1"].values)).T
        d = np.sort(cdist(xy, xy), axis=1)[:, :k + 2]
        gap = d[:, 1:] - d[:, :-1]
        assert np.all(gap > 1e-9 * d[:, 1:]), (fov, k)


def run_alignment(table, k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # 0 / 0 and x / 0 in the reference's quotient
        got = ref_fs.calculate_fiber_alignment(table, k=k)
    assert list(got.columns) == list(table.columns) + ["alignment_score"] and len(got) == len(table)
    assert (got["fov"].values == table["fov"].values).all() and (got["label"].values == table["label"].values).all()
    return np.asarray(got["alignment_score"].values, dtype=np.float64)


def summary_cohort(rs, spec):
    """The synthetic object table of a cohort (alignment by the reference, k = 4) and its label planes."""
    frames, planes = [], {}
    for fov, side, n in spec:
        major = rs.uniform(8, 40, n)
        frames.append(pd.DataFrame({
            "fov": fov, "label": rs.permutation(np.arange(1, n + 1)),
            "centroid-0": rational(rs, n, side), "centroid-1": rational(rs, n, side),
            "major_axis_length": major, "minor_axis_length": major / rs.uniform(1.2, 6, n),
            "orientation": rs.uniform(-np.pi / 2, np.pi / 2, n), "area": rs.randint(15, 400, n),
            "eccentricity": rs.uniform(0.3, 1, n), "euler_number": rs.randint(-2, 2, n)}))
        plane = np.zeros((side, side), dtype=np.int32)
        for lab in range(1, 6):
            r, c = rs.randint(0, side - 6, 2)
            plane[r:r + rs.randint(1, 6), c:c + rs.randint(1, 6)] = lab
        planes[fov] = plane
    table = pd.concat(frames, ignore_index=True)
    assert_no_ties(table, 4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ref_fs.calculate_fiber_alignment(table, k=4), planes


def run_summary(table, planes, tile_length, min_fiber_num):
    with tempfile.TemporaryDirectory() as td:
        for fov, plane in planes.items():
            image_io.write_image(os.path.join(td, fov + "_fiber_labels.tiff"), plane)
        os.makedirs(os.path.join(td, "tile_stats_%d" % tile_length))      # the reference expects it to exist
        fov_stats, tile_stats = ref_fs.generate_summary_stats(table, td, tile_length=tile_length,
                                                              min_fiber_num=min_fiber_num, save_tiles=False)
        written = sorted(os.path.relpath(os.path.join(d, f), td) for d, _, files in os.walk(td) for f in files
                         if f.endswith(".csv"))
    return fov_stats, tile_stats, written


def main():
    rs = np.random.RandomState(26)
    out = {"k_values": np.array(K_VALUES), "qualifying": np.array(QUALIFYING), "n_summary": np.array(len(SUMMARY_CASES))}

    table = alignment_table(rs)
    assert_no_ties(table, max(K_VALUES))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = table["major_axis_length"].values / table["minor_axis_length"].values
    assert np.isinf(ratio).sum() == 6 and np.isnan(ratio).sum() == len(QUALIFYING)
    assert [int(((table.fov == "fov%d" % f) & (ratio >= 2)).sum()) for f in range(len(QUALIFYING))] == QUALIFYING
    store_frame(out, "a_", table)
    small = reference_test_table()
    assert_no_ties(small, max(K_VALUES))
    store_frame(out, "t_", small)
    for k in K_VALUES:
        scores = run_alignment(table, k)
        assert int(np.isfinite(scores).sum()) == sum(QUALIFYING)
        out["a_scores_k%d" % k] = scores
        out["t_scores_k%d" % k] = run_alignment(small, k)
    only = table[(table.fov == "fov1").values & (ratio >= 2)].index[0]
    assert out["a_scores_k4"][only] == 0.0        # a FOV's only fibre: no neighbour, score 0

    cohorts = {name: summary_cohort(rs, spec) for name, spec in COHORTS.items()}
    for name, (tab, planes) in cohorts.items():
        store_frame(out, "c_%s_" % name, tab)
        out["c_%s_fovs" % name] = np.array(list(planes))
        for fov, plane in planes.items():
            out["c_%s_plane_%s" % (name, fov)] = plane
        dens = [ref_fs.calculate_density(tab[tab.fov == fov], planes[fov].shape[0] ** 2) for fov in planes]
        out["c_%s_density" % name] = np.asarray(dens, dtype=np.float64)
    seen_nan = 0
    for i, (name, tile_length, min_fiber_num) in enumerate(SUMMARY_CASES):
        tab, planes = cohorts[name]
        fov_stats, tile_stats, written = run_summary(tab, planes, tile_length, min_fiber_num)
        p = "s%d_" % i
        out[p + "cohort"], out[p + "tile_length"], out[p + "min_fiber_num"] = \
            np.array(name), np.array(tile_length), np.array(min_fiber_num)
        store_frame(out, p + "fov_", fov_stats)
        store_frame(out, p + "tile_", tile_stats)
        out[p + "written"] = np.array(written)
        seen_nan += int(np.isnan(tile_stats["avg_alignment_score"].to_numpy(dtype=np.float64)).sum())
    assert seen_nan > 0

    path = os.path.join(OUT_DIR, "g26_fibers.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, ROOT), len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
