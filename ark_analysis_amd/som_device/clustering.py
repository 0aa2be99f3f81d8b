"""Neighbourhood clustering: silhouette sweeps (K15) and Lloyd's k-means (K19)."""
import operator

import numpy as np
import torch

from .. import _capi


# ---- silhouette sweeps (K15) ----------------------------------------------------------------------------------------
SILHOUETTE_MAX_D = 64   # pxsom_silhouette keeps a row in registers
SILHOUETTE_MAX_K = 32


def _silhouette_call(x: torch.Tensor, labels: torch.Tensor, n_clusters):
    """The checks, the sort by label and the one pxsom_silhouette call behind :func:`silhouette_samples`,
    :func:`silhouette_scores` and :func:`silhouette_sums`: ``(samples [M, n], scores [M], single, sums [M, n, k],
    counts [M, k])``, ``single`` when ``labels`` came as ``[n]`` and k the largest of ``n_clusters``."""
    if x.dim() != 2 or x.dtype != torch.float64:
        raise ValueError("x must be an [n, d] float64 HBM tensor")
    n, d = x.shape
    if labels.dim() not in (1, 2) or labels.shape[-1] != n or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("labels must be an [n] or [M, n] int32 / int64 HBM tensor on x's device")
    single = labels.dim() == 1
    n_labelings = 1 if single else labels.shape[0]
    if n_labelings < 1:
        raise ValueError("labels must hold at least one labeling")
    ks = [operator.index(v) for v in (n_clusters if isinstance(n_clusters, (list, tuple, np.ndarray)) else [n_clusters])]
    if len(ks) == 1:
        ks = ks * n_labelings
    if len(ks) != n_labelings:
        raise ValueError("n_clusters must be one number or one per labeling: got %d for %d labelings"
                         % (len(ks), n_labelings))
    if not 1 <= d <= SILHOUETTE_MAX_D:
        raise ValueError("d must lie in 1 .. %d (the device route keeps a row in registers), got %d"
                         % (SILHOUETTE_MAX_D, d))
    if min(ks) < 2 or max(ks) > SILHOUETTE_MAX_K:
        raise ValueError("n_clusters must lie in 2 .. %d (the device route's limit), got %s" % (SILHOUETTE_MAX_K, ks))
    if n < 2:
        raise ValueError("the silhouette needs n >= 2 rows, got %d" % n)
    if not x.is_cuda:
        raise ValueError("x must be an [n, d] float64 HBM tensor")
    dev = x.device
    if labels.device != dev:
        raise ValueError("labels must be an [n] or [M, n] int32 / int64 HBM tensor on x's device")
    labels = labels.reshape(n_labelings, n)
    limit = torch.tensor(ks, dtype=labels.dtype, device=dev).unsqueeze(1)
    if not bool(((labels >= 0) & (labels < limit)).all().cpu()):
        raise ValueError("labels must lie in [0, n_clusters)")
    k = max(ks)
    x = x.contiguous()
    labels32 = labels.to(torch.int32).contiguous()
    order = torch.argsort(labels32, dim=1, stable=True).to(torch.int32).contiguous()
    counts = torch.empty((n_labelings, k), dtype=torch.int32, device=dev)
    sums = torch.empty((n_labelings, n, k), dtype=torch.float64, device=dev)
    samples = torch.empty((n_labelings, n), dtype=torch.float64, device=dev)
    scores = torch.empty((n_labelings,), dtype=torch.float64, device=dev)
    _capi.call("pxsom_silhouette", x.data_ptr(), n, d, labels32.data_ptr(), order.data_ptr(), n_labelings, k,
               counts.data_ptr(), sums.data_ptr(), samples.data_ptr(), scores.data_ptr(),
               _capi.stream_ptr())
    return samples, scores, single, sums, counts


def _silhouette(x: torch.Tensor, labels: torch.Tensor, n_clusters):
    """``(samples [M, n], scores [M], single)`` of :func:`_silhouette_call`."""
    return _silhouette_call(x, labels, n_clusters)[:3]


def silhouette_sums(x: torch.Tensor, labels: torch.Tensor, n_clusters):
    """What pxsom_silhouette forms on its way to the samples: ``(sums, counts)`` with ``sums[m, i, c]`` (``[M, n, k]``
    float64, k the largest of ``n_clusters``) the sum over the rows j of cluster c under labeling m of the Euclidean
    distance from row i to row j, and ``counts[m, c]`` (``[M, k]`` int32) the cluster sizes.  Arguments and limits as
    for :func:`silhouette_samples`; ``labels`` of shape ``[n]`` count as one labeling (M = 1).  The pooled
    within-cluster sum of the gap statistic is made of ``sums[m, i, labels[m, i]]``."""
    return _silhouette_call(x, labels, n_clusters)[3:]


def silhouette_samples(x: torch.Tensor, labels: torch.Tensor, n_clusters) -> torch.Tensor:
    """pxsom_silhouette: sklearn's ``silhouette_samples`` (Euclidean) of the rows of ``x`` ``[n, d]`` float64 under
    ``labels`` -- ``[n]`` int32 / int64 with values in ``[0, n_clusters)``, giving ``[n]`` float64, or ``[M, n]`` for M
    labelings in one call (``n_clusters`` then one number, or one per labeling), giving ``[M, n]``.  Distances in the
    direct form in binary64 (equal rows are at exactly 0), every sum in an order fixed by the input: the same call
    gives the same bits.  ``1 <= d <= 64``, ``2 <= n_clusters <= 32``, ``n >= 2``; a cluster may be empty."""
    samples, _, single = _silhouette(x, labels, n_clusters)
    return samples[0] if single else samples


def silhouette_scores(x: torch.Tensor, labels: torch.Tensor, n_clusters) -> torch.Tensor:
    """The mean of :func:`silhouette_samples` per labeling (sklearn's ``silhouette_score``), reduced on the device in a
    fixed order: ``[M]`` float64 (``[1]`` for ``labels`` of shape ``[n]``)."""
    return _silhouette(x, labels, n_clusters)[1]


# ---- Lloyd's k-means for several problems at once (K19) -------------------------------------------------------------
KMEANS_MAX_D = 64    # pxsom_kmeans_lloyd keeps a row in registers
KMEANS_MAX_K = 32
KMEANS_MAX_PROBLEMS = 4096


def _kmeans_ks(d: int, ks):
    ks = np.ascontiguousarray([operator.index(k) for k in ks], dtype=np.int32)
    if not 1 <= d <= KMEANS_MAX_D:
        raise ValueError("d must lie in 1 .. %d (the device route keeps a row in registers), got %d" % (KMEANS_MAX_D, d))
    if not 1 <= len(ks) <= KMEANS_MAX_PROBLEMS:
        raise ValueError("between 1 and %d problems per call, got %d" % (KMEANS_MAX_PROBLEMS, len(ks)))
    if ks.min() < 1 or ks.max() > KMEANS_MAX_K:
        raise ValueError("every k must lie in 1 .. %d (the device route's limit), got %s" % (KMEANS_MAX_K, ks.tolist()))
    return ks


def kmeans_group_count(d: int, ks) -> int:
    """How many groups -- passes over the rows per iteration -- pxsom_kmeans_lloyd forms for problems of these ``ks`` on
    rows of ``d`` columns (the rule and its LDS bytes: csrc/pxsom_kmeans.hip).  A host-side function."""
    ks = _kmeans_ks(d, ks)
    got = _capi.lib().pxsom_kmeans_group_count(d, len(ks), ks.ctypes.data)
    _capi.check(min(got, 0), "pxsom_kmeans_group_count")
    return got


def kmeans_lloyd(rows: torch.Tensor, inits, tol, max_iter, *, workgroups: int = 0):
    """pxsom_kmeans_lloyd: Lloyd's k-means of the finite rows ``[n, d]`` float64 (HBM) for every problem of ``inits`` -- a
    sequence of ``[k_p, d]`` float64 initial centres (numpy arrays or tensors) -- in shared passes over the rows.
    ``tol`` (the absolute bound on the summed squared centre shift) and ``max_iter`` are one number or one per problem.

    Returns ``(labels, centres, inertia, n_iter)``: ``[P, n]`` int32 on the device, a list of ``[k_p, d]`` float64
    tensors on the device, and numpy ``[P]`` float64 / int32.  The rule is DESIGN.md K19's; the same call gives the same
    bits for any ``workgroups`` (0: the default grid).  ``1 <= d <= 64``, ``1 <= k_p <= 32``, ``k_p <= n``; ``n = 0``
    returns at once."""
    if rows.dim() != 2 or rows.dtype != torch.float64:
        raise ValueError("rows must be an [n, d] float64 HBM tensor")
    n, d = rows.shape
    inits = [torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c) for c in inits]
    for c in inits:
        if c.dim() != 2 or c.shape[1] != d or c.dtype != torch.float64:
            raise ValueError("every entry of inits must be a [k, %d] float64 array, got %s %s"
                             % (d, tuple(c.shape), c.dtype))
    ks = _kmeans_ks(d, [c.shape[0] for c in inits])
    n_problems = len(ks)
    tols = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=np.float64), (n_problems,)))
    iters = np.ascontiguousarray(np.broadcast_to(np.asarray(max_iter, dtype=np.int32), (n_problems,)))
    if not (tols >= 0).all():
        raise ValueError("tol must be >= 0")
    if iters.min() < 1:
        raise ValueError("max_iter must be >= 1")
    if n > 0 and ks.max() > n:
        raise ValueError("k = %d exceeds the n = %d rows" % (ks.max(), n))
    if n >= 2 ** 31:
        raise ValueError("n must stay below 2^31, got %d" % n)
    if not rows.is_cuda:
        raise ValueError("rows must be an [n, d] float64 HBM tensor")
    dev = rows.device
    rows = rows.contiguous()
    centres = torch.cat([c.to(dev) for c in inits]).contiguous()
    labels = torch.empty((n_problems, n), dtype=torch.int32, device=dev)
    inertia = np.zeros(n_problems, dtype=np.float64)
    n_iter = np.zeros(n_problems, dtype=np.int32)
    lib = _capi.lib()
    ws_bytes = lib.pxsom_kmeans_workspace_bytes(n, d, n_problems, ks.ctypes.data)
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=dev)
    _capi.call("pxsom_kmeans_lloyd", rows.data_ptr(), n, d, n_problems, ks.ctypes.data, centres.data_ptr(), tols.ctypes.data,
               iters.ctypes.data, labels.data_ptr(), inertia.ctypes.data, n_iter.ctypes.data,
               ws.data_ptr(), ws_bytes, operator.index(workgroups), _capi.stream_ptr())
    return labels, list(torch.split(centres, ks.tolist())), inertia, n_iter
