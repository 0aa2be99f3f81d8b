"""The numpy / pandas statement of pxsom_neighborhood_sums and of the four spatial-LDA featurisations,
written from the statement of what spatial_lda's featurize_samples is taken to do -- not from any library's code.

neighborhood_sums: per row, the mask over its FOV's rows is ``np.sqrt(dx * dx + dy * dy) < radius`` (``<=`` when
closed); the count is the mask's sum and the sums are the last row of the cumulative sum of a row of +0.0 followed by
``feats[mask]`` -- a cumulative sum is the sequential fold in row order, which ``np.add.reduce`` (pairwise) is not, and
the fold starts from +0.0 as include/pxsom.h states it: members that are all -0.0 sum to +0.0.

featurize: one pandas sub-frame per anchor cell, as the featurisations are worded: cells per cluster value, cells with a
marker above 0.5, the mean marker expression, the number of cells."""
import numpy as np
import pandas as pd


def _mask(pts, i, radius, closed):
    dx = pts[:, 0] - pts[i, 0]
    dy = pts[:, 1] - pts[i, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.sqrt(dx * dx + dy * dy)
        return dist <= radius if closed else dist < radius


def neighborhood_sums(xy, feats, seg, radius, closed=False):
    """``(sums [n, p] float64, counts [n] int32)``; ``feats`` None gives p = 0.  A row no FOV holds keeps 0."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    feats = np.zeros((n, 0)) if feats is None else np.asarray(feats, dtype=np.float64)
    sums = np.zeros((n, feats.shape[1]), dtype=np.float64)
    counts = np.zeros(n, dtype=np.int32)
    radius = np.float64(radius)
    for a, b in zip(seg[:-1], seg[1:]):
        a, b = int(a), int(b)
        pts, rows = xy[a:b], feats[a:b]
        for i in range(b - a):
            mask = _mask(pts, i, radius, closed)
            counts[a + i] = mask.sum()
            if mask.any() and rows.shape[1]:
                with np.errstate(invalid="ignore"):
                    sums[a + i] = np.concatenate([np.zeros((1, rows.shape[1])), rows[mask]]).cumsum(axis=0)[-1]
    return sums, counts


def host_stand_in(radius_test="lt"):
    """The signature of ark_analysis_amd.spLDA.processing._neighborhood_sums_device."""
    def entry(xy, feats, seg, radius):
        return neighborhood_sums(xy, feats, seg, radius, closed=radius_test == "le")
    return entry


def silhouette_sums_stand_in(x, labels, n_clusters):
    """The signature of ark_analysis_amd.utils.spatial_lda_utils._silhouette_sums_device: S[i, c] = the sum of the
    Euclidean distances from row i to the rows of cluster c, and the cluster sizes."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    dist = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    sums = np.stack([dist[:, labels == c].sum(axis=1) for c in range(n_clusters)], axis=1)
    return sums, np.bincount(labels, minlength=n_clusters).astype(np.int32)


# ---- what the g27 fixture's generator and its test share: the inputs and the calls that must raise --------------------
GOLDEN_MARKERS = ["CD4", "CD8", "CD45"]
GOLDEN_CLUSTER_SUBSET = ["tumour", "b_cell"]
FORMAT_CASES = {"markers": dict(markers=GOLDEN_MARKERS, clusters=None),
                "clusters": dict(markers=None, clusters=["tumour", "b_cell", "t_cell", "stroma"]),
                "both": dict(markers=GOLDEN_MARKERS, clusters=GOLDEN_CLUSTER_SUBSET)}


def golden_cell_table():
    """A cell table of three FOVs (names out of sorted order, rows interleaved) with the columns the spatial-LDA
    formatting needs, three markers, and two columns it has to drop."""
    rs = np.random.RandomState(27)
    n = 90
    table = pd.DataFrame({
        "cell_size": rs.randint(20, 400, n), "CD4": rs.uniform(0, 1, n), "CD8": rs.uniform(0, 1, n),
        "CD45": rs.uniform(0, 1, n), "unused_marker": rs.uniform(0, 1, n), "label": np.arange(1, n + 1),
        "centroid-0": rs.uniform(0, 400, n), "centroid-1": rs.uniform(0, 400, n),
        "cell_meta_cluster": rs.choice(["tumour", "b_cell", "t_cell", "stroma"], n),
        "fov": rs.choice(["fov8", "fov12", "fov3"], n), "area_extra": rs.uniform(5, 50, n)})
    return table


def golden_error_cases(spu, table, formatted):
    """``[(name, call)]``: every way the two argument checkers of a ``spatial_lda_utils`` module ``spu`` raise."""
    no_clusters = {k: v for k, v in formatted.items() if k != "clusters"}
    no_markers = {k: v for k, v in formatted.items() if k != "markers"}
    fmt, feat = spu.check_format_cell_table_args, spu.check_featurize_cell_table_args
    return [
        ("format_missing_column", lambda: fmt(table.drop(columns=["cell_size"]), GOLDEN_MARKERS, None)),
        ("format_both_none", lambda: fmt(table, None, None)),
        ("format_markers_empty", lambda: fmt(table, [], None)),
        ("format_markers_unknown", lambda: fmt(table, ["CD4", "CD99"], None)),
        ("format_clusters_empty", lambda: fmt(table, None, [])),
        ("format_clusters_unknown", lambda: fmt(table, None, ["tumour", "nk_cell"])),
        ("featurize_radius_type", lambda: feat(formatted, "cluster", 50.0, "is_index")),
        ("featurize_radius_small", lambda: feat(formatted, "cluster", 24, "is_index")),
        ("featurize_unknown", lambda: feat(formatted, "clusters", 50, "is_index")),
        ("featurize_no_clusters", lambda: feat(no_clusters, "cluster", 50, "is_index")),
        ("featurize_no_markers_marker", lambda: feat(no_markers, "marker", 50, "is_index")),
        ("featurize_no_markers_avg", lambda: feat(no_markers, "avg_marker", 50, "is_index")),
        ("featurize_cell_index", lambda: feat(formatted, "count", 50, "is_anchor")),
    ]


def golden_errors(spu, table, formatted):
    """``{name: "ExceptionType: message"}`` of golden_error_cases."""
    out = {}
    for name, call in golden_error_cases(spu, table, formatted):
        try:
            call()
        except Exception as e:      # noqa: BLE001  (the type is recorded)
            out[name] = "%s: %s" % (type(e).__name__, e)
        else:
            out[name] = "no error"
    return out


def golden_within_case():
    rs = np.random.RandomState(28)
    return rs.normal(size=(60, 4)), rs.randint(0, 3, 60)


def store_frame(out, prefix, df):
    out[prefix + "columns"] = np.array([str(c) for c in df.columns])
    out[prefix + "dtypes"] = np.array([str(t) for t in df.dtypes])
    for i, col in enumerate(df.columns):
        v = df[col].to_numpy()
        out[prefix + "col%d" % i] = v.astype(str) if v.dtype == object else v


def record_formatted(out, prefix, formatted):
    """A formatted cell table into ``out``: its frames and the three bookkeeping keys (None as an empty array)."""
    out[prefix + "keys"] = np.array([str(k) for k in formatted.keys()])
    out[prefix + "fovs"] = np.asarray(formatted["fovs"]).astype(str)
    for key in ("markers", "clusters"):
        out[prefix + key + "_none"] = np.array(formatted[key] is None)
        out[prefix + key] = np.array([] if formatted[key] is None else formatted[key], dtype=str)
    for fov in formatted["fovs"]:
        store_frame(out, prefix + "%s_" % fov, formatted[fov])


def featurize(cell_table, featurization, radius, cell_index="is_index", closed=False, fold=False):
    """The per-anchor pandas loop.  ``fold``: avg_marker as the sequential fold over the neighbourhood divided by its
    size (what the kernel's sums give) instead of pandas' ``.mean()``.  Also returns the neighbourhood sizes and, for
    avg_marker, the sums of absolute values per entry (for the error bound)."""
    markers = cell_table.get("markers")
    all_clusters = None
    if featurization == "cluster":
        all_clusters = sorted(pd.concat([cell_table[f]["cluster"] for f in cell_table["fovs"]]).unique().tolist())
    rows, index, sizes, abs_sums = [], [], [], []
    for fov in list(cell_table["fovs"]):
        df = cell_table[fov]
        pts = df[["x", "y"]].to_numpy(dtype=np.float64)
        for pos in range(len(df)):
            if not bool(df[cell_index].iloc[pos]):
                continue
            hood = df[_mask(pts, pos, np.float64(radius), closed)]
            index.append((fov, pos))
            sizes.append(len(hood))
            if featurization == "cluster":
                vc = hood["cluster"].value_counts()
                rows.append([int(vc.get(c, 0)) for c in all_clusters])
            elif featurization == "marker":
                rows.append([int((hood[m] > 0.5).sum()) for m in markers])
            elif featurization == "avg_marker":
                if fold:
                    rows.append([np.cumsum(hood[m].to_numpy(dtype=np.float64))[-1] / np.float64(len(hood)) for m in markers])
                else:
                    rows.append([hood[m].mean() for m in markers])
                abs_sums.append([np.abs(hood[m].to_numpy(dtype=np.float64)).sum() for m in markers])
            else:
                rows.append([len(hood)])
    columns = {"cluster": all_clusters, "marker": markers, "avg_marker": markers, "count": ["count"]}[featurization]
    frame = pd.DataFrame(rows, index=pd.MultiIndex.from_tuples(index), columns=columns)
    return frame, np.asarray(sizes), np.asarray(abs_sums, dtype=np.float64)
