"""Numpy statement of the cell-table contract: what pxsom_cellquant computes per cell, written the way
the reference computes it (ark/segmentation/marker_quantification.py under fast_extraction=True, signal_extraction.py,
segmentation_utils.find_nuclear_label_id), and the frames generate_cell_table builds from it.

A cell is the set of pixels of one nonzero label; its coords are in raster order (regionprops' coords).  total_intensity
is ``np.sum(img[rows, cols], axis=0)`` in the image's dtype, positive_pixel ``np.sum(img[rows, cols] > t, axis=0)``,
center_weighting ``w.dot(img[rows, cols])`` with ``w = 1 - d / (max d + 1)``, d the Chebyshev distance to the centroid
``coords.mean(axis=0)``.  The nucleus of a cell is the nonzero nuclear label with the most pixels in the cell, the
smallest on a tie."""
import numpy as np
import pandas as pd

MODES = ("total_intensity", "positive_pixel", "center_weighting")


def cell_coords(seg):
    """{label: coords [n, 2] int64 in raster order} for every nonzero label, labels ascending."""
    seg = np.asarray(seg)
    flat = seg.ravel()
    order = np.argsort(flat, kind="stable")
    labels, starts = np.unique(flat[order], return_index=True)
    ends = np.append(starts[1:], flat.size)
    w = seg.shape[1]
    out = {}
    for lab, s, e in zip(labels, starts, ends):
        if lab == 0:
            continue
        px = order[s:e]
        out[int(lab)] = np.stack([px // w, px % w], axis=1).astype(np.int64)
    return out


def extract(coords, img, mode, threshold=0):
    """One cell's channel values (the reference's EXTRACTION_FUNCTION[mode]) as float64."""
    vals = img[tuple(coords.T)]
    if mode == "total_intensity":
        return np.asarray(np.sum(vals, axis=0), dtype=np.float64)
    if mode == "positive_pixel":
        return np.asarray(np.sum(vals > threshold, axis=0), dtype=np.float64)
    centroid = coords.mean(axis=0)[None, :]
    weights = np.linalg.norm(coords - centroid, ord=np.inf, axis=1)
    weights = 1 - (weights / (np.max(weights) + 1))
    return np.asarray(weights.dot(vals), dtype=np.float64)


def center_weighting_bound(coords, img):
    """The stated bound of a center_weighting value against any other summation order of the same products:
    2 * gamma(n + 1) * sum |w * v| per channel, gamma(k) = k u / (1 - k u), u = 2^-53."""
    vals = img[tuple(coords.T)].astype(np.float64)
    centroid = coords.mean(axis=0)[None, :]
    weights = np.linalg.norm(coords - centroid, ord=np.inf, axis=1)
    weights = 1 - (weights / (np.max(weights) + 1))
    k = coords.shape[0] + 1
    u = 2.0 ** -53
    return 2 * (k * u / (1 - k * u)) * (np.abs(weights)[:, None] * np.abs(vals)).sum(axis=0)


def nuclear_label_id(nuc, coords):
    """segmentation_utils.find_nuclear_label_id: None when the cell covers no nucleus."""
    ids, counts = np.unique(nuc[tuple(coords.T)], return_counts=True)
    if ids[ids != 0].size == 0:
        return None
    return ids[ids != 0][np.argmax(counts[ids != 0])]


def quantify(seg, img, mode="total_intensity", threshold=0, nuc=None):
    """The device contract of som_device.cell_quantify as host arrays: keys, count, sums [n, 2], bbox [n, 4],
    values [n, C] and, with ``nuc``, nuc_keys and nuc (index into nuc_keys, -1: none)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    cells = cell_coords(seg)
    keys = np.array(sorted(cells), dtype=np.int64)
    n, c = keys.size, img.shape[2]
    out = {"keys": keys.astype(np.int32), "count": np.zeros(n, np.int64), "sums": np.zeros((n, 2), np.int64),
           "bbox": np.zeros((n, 4), np.int32), "values": np.zeros((n, c), np.float64)}
    if nuc is not None:
        nuc = np.asarray(nuc)
        nuc_keys = np.unique(nuc)
        nuc_keys = nuc_keys[nuc_keys != 0].astype(np.int64)
        out["nuc_keys"] = nuc_keys.astype(np.int32)
        out["nuc"] = np.full(n, -1, np.int32)
    for i, lab in enumerate(keys):
        co = cells[int(lab)]
        out["count"][i] = co.shape[0]
        out["sums"][i] = co.sum(axis=0)
        out["bbox"][i] = (co[:, 0].min(), co[:, 0].max(), co[:, 1].min(), co[:, 1].max())
        out["values"][i] = extract(co, img, mode, threshold)
        if nuc is not None:
            nid = nuclear_label_id(nuc, co)
            if nid is not None:
                out["nuc"][i] = int(np.searchsorted(nuc_keys, nid))
    return out


def cell_frames(fov, seg, img, channels, mode="total_intensity", threshold=0, nuc=None, mask_type="whole_cell"):
    """(size-normalised, arcsinh) frames of one FOV and mask type, as the reference lays them out: cell_size, the
    channels, label (int32), centroid-0, centroid-1, the same with '_nuclear' (label_nuclear float64), fov, mask_type.
    Entries the reference leaves uninitialised (a cell without a nucleus, divided by size 0) are 0 here."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    cells = cell_coords(seg)
    names = ["cell_size"] + list(channels) + ["label", "centroid-0", "centroid-1"]
    c = len(channels)

    def row(co, lab):
        return np.concatenate(([co.shape[0]], extract(co, img, mode, threshold), [lab], co.mean(axis=0)))

    raw = np.zeros((len(cells), c + 4))
    for i, lab in enumerate(sorted(cells)):
        raw[i] = row(cells[lab], lab)
    blocks = [raw]
    if nuc is not None:
        nuclei = cell_coords(nuc)
        nraw = np.zeros_like(raw)
        for i, lab in enumerate(sorted(cells)):
            nid = nuclear_label_id(nuc, cells[lab])
            if nid is not None:
                nraw[i] = row(nuclei[int(nid)], nid)
        blocks.append(nraw)
    norms, asinhs = [], []
    for b in blocks:
        norm = b.copy()
        size = b[:, :1]
        norm[:, 1:1 + c] = np.divide(b[:, 1:1 + c], size, out=np.zeros_like(b[:, 1:1 + c]), where=size > 0)
        asinh = norm.copy()
        asinh[:, 1:1 + c] = np.arcsinh(norm[:, 1:1 + c] * 100)
        norms.append(norm)
        asinhs.append(asinh)
    frames = []
    for parts in (norms, asinhs):
        df = pd.DataFrame(parts[0], columns=names)
        df["label"] = df["label"].astype(np.int32)
        if nuc is not None:
            df = pd.concat((df, pd.DataFrame(parts[1], columns=[f + "_nuclear" for f in names])), axis=1)
        df["fov"] = fov
        df["mask_type"] = "whole_cell" if mask_type == "final_cells_remaining" else mask_type
        frames.append(df)
    return tuple(frames)


# ---- synthetic segmentations --------------------------------------------------------------------------------------
def voronoi_labels(h, w, n_cells, seed=0, background=0.1, dtype=np.int32, first_label=1):
    """Voronoi-like cells: every pixel takes the label of its nearest of ``n_cells`` random sites (computed on a
    coarse grid and upsampled by nearest neighbour, so it stays cheap at 2048^2); a fraction ``background`` of the
    cells is cleared to 0.  Labels first_label .. first_label + n_cells - 1, shuffled."""
    rng = np.random.default_rng(seed)
    step = max(1, int(np.sqrt(h * w / n_cells) / 4))
    gh, gw = (h + step - 1) // step, (w + step - 1) // step
    sites = np.stack([rng.uniform(0, gh, n_cells), rng.uniform(0, gw, n_cells)], axis=1)
    from scipy.spatial import cKDTree
    gy, gx = np.mgrid[0:gh, 0:gw]
    _, near = cKDTree(sites).query(np.stack([gy.ravel() + 0.5, gx.ravel() + 0.5], axis=1))
    labels = rng.permutation(n_cells).astype(np.int64) + first_label
    keep = rng.random(n_cells) >= background
    lab = np.where(keep[near], labels[near], 0).reshape(gh, gw)
    full = np.repeat(np.repeat(lab, step, axis=0), step, axis=1)[:h, :w]
    return np.ascontiguousarray(full).astype(dtype)


def fragment(seg, labels, pieces=6, seed=0):
    """Scatter each label of ``labels`` over ``pieces`` far-apart square patches (fragmented labels: bbox >> count)."""
    seg = np.array(seg)
    rng = np.random.default_rng(seed)
    h, w = seg.shape
    for lab in labels:
        for _ in range(pieces):
            r, c = int(rng.integers(0, h - 3)), int(rng.integers(0, w - 3))
            seg[r:r + 3, c:c + 3] = lab
    return seg
