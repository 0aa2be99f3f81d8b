"""PCA scores and exact t-SNE of a cell table (K30): the column moments and projection, the squared distances, the
perplexity search with the joint P, one descent iteration, and the host loop over it."""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _capi

TSNE_MAX_ROWS = 1 << 20            # include/pxsom.h PXSOM_TSNE_MAX_ROWS
TSNE_EXPLORATION_ITER = 250        # sklearn's _EXPLORATION_MAX_ITER
TSNE_ITER_CHECK = 50               # sklearn's _N_ITER_CHECK
TSNE_EARLY_EXAGGERATION = 12.0
TSNE_MIN_GAIN = 0.01
TSNE_MIN_GRAD_NORM = 1e-7


class TsneResult(NamedTuple):
    """``embedding`` float64 ``[n, 2]`` in HBM, ``kl_divergence`` the last error computed, ``n_iter`` the index of the last
    iteration (sklearn's ``n_iter_``)."""
    embedding: torch.Tensor
    kl_divergence: float
    n_iter: int


def _table(x: torch.Tensor, c_min: int = 1) -> Tuple[int, int, int]:
    if x.dim() != 2 or not x.is_cuda or not x.is_contiguous() or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("the table must be a contiguous float32 or float64 [rows, columns] HBM tensor")
    n, c = x.shape
    if n < 1 or n > TSNE_MAX_ROWS:
        raise ValueError("the table must have 1 .. %d rows, got %d" % (TSNE_MAX_ROWS, n))
    if c < c_min or c > _capi.MAX_CHANNELS:
        raise ValueError("the table must have %d .. %d columns, got %d" % (c_min, _capi.MAX_CHANNELS, c))
    return n, c, _capi.dtype_code(x)


def _f64(t: torch.Tensor, shape, what: str) -> torch.Tensor:
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
        raise ValueError("%s must be a contiguous float64 %s HBM tensor" % (what, list(shape)))
    return t


def tsne_workspace_bytes(n: int) -> int:
    return int(_capi.lib().pxsom_tsne_workspace_bytes(int(n)))


def _workspace(n: int, device) -> torch.Tensor:
    return torch.empty(tsne_workspace_bytes(n), dtype=torch.uint8, device=device)


def column_moments(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Column means ``[c]`` and the centred covariance over ``n - 1`` ``[c, c]`` (float64, HBM) of a contiguous float32 or
    float64 ``[n, c]`` HBM table, ``n >= 2`` and ``2 <= c <= 1024``."""
    n, c, code = _table(x, 2)
    if n < 2:
        raise ValueError("the covariance needs at least 2 rows, got %d" % n)
    mean = torch.empty(c, dtype=torch.float64, device=x.device)
    cov = torch.empty((c, c), dtype=torch.float64, device=x.device)
    _capi.call("pxsom_column_moments", x.data_ptr(), n, c, code, mean.data_ptr(), cov.data_ptr(), _capi.stream_ptr())
    return mean, cov


def project_rows(x: torch.Tensor, mean: torch.Tensor, axes: torch.Tensor) -> torch.Tensor:
    """``(x - mean) @ axes.T`` for float64 ``mean [c]`` and ``axes [2, c]`` -> float64 ``[n, 2]``, channels ascending."""
    n, c, code = _table(x)
    _f64(mean, (c,), "mean")
    _f64(axes, (2, c), "axes")
    scores = torch.empty((n, 2), dtype=torch.float64, device=x.device)
    _capi.call("pxsom_project_rows", x.data_ptr(), n, c, code, mean.data_ptr(), axes.data_ptr(), scores.data_ptr(),
               _capi.stream_ptr())
    return scores


def principal_axes(cov: np.ndarray) -> np.ndarray:
    """The two leading eigenvectors ``[2, c]`` of a symmetric host matrix, each signed so that its entry of largest
    magnitude is positive (sklearn's ``svd_flip(..., u_based_decision=False)``).  ``c x c`` work on the host."""
    vals, vecs = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    axes = np.ascontiguousarray(vecs[:, ::-1][:, :2].T)
    big = np.argmax(np.abs(axes), axis=1)
    signs = np.sign(axes[np.arange(2), big])
    signs[signs == 0] = 1.0
    return axes * signs[:, None]


def pca_scores(x: torch.Tensor) -> torch.Tensor:
    """The first two principal-component scores of the table, sklearn's ``PCA().fit_transform(x)[:, :2]``: device moments,
    the eigenvectors of the ``c x c`` covariance on the host (one read-back), device projection."""
    mean, cov = column_moments(x)
    axes = torch.from_numpy(principal_axes(cov.cpu().numpy())).to(x.device)
    return project_rows(x, mean, axes)


def pair_sqdist_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 ``[n, n]``: ``sum_t (x_it - x_jt)^2`` in binary64, t ascending, then one rounding to float32."""
    n, c, code = _table(x)
    if out is None:
        out = torch.empty((n, n), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, n) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 [n, n] HBM tensor")
    _capi.call("pxsom_pair_sqdist_f32", x.data_ptr(), n, c, code, out.data_ptr(), _capi.stream_ptr())
    return out


def tsne_affinities(d2: torch.Tensor, perplexity: float, joint: bool = True, out: Optional[torch.Tensor] = None):
    """sklearn's ``_binary_search_perplexity`` per row of the float32 ``[n, n]`` squared distances and, with ``joint``,
    the dense ``_joint_probabilities`` -> ``(P, beta, steps)``: float64 ``[n, n]``, float64 ``[n]``, int32 ``[n]``."""
    if d2.dim() != 2 or d2.shape[0] != d2.shape[1] or d2.dtype != torch.float32 or not d2.is_cuda or not d2.is_contiguous():
        raise ValueError("d2 must be a contiguous float32 [n, n] HBM tensor")
    n = d2.shape[0]
    if n < 2 or n > TSNE_MAX_ROWS:
        raise ValueError("d2 must have 2 .. %d rows, got %d" % (TSNE_MAX_ROWS, n))
    if not (np.isfinite(perplexity) and perplexity > 0):
        raise ValueError("perplexity must be positive and finite, got %r" % (perplexity,))
    if out is None:
        out = torch.empty((n, n), dtype=torch.float64, device=d2.device)
    else:
        _f64(out, (n, n), "out")
    beta = torch.empty(n, dtype=torch.float64, device=d2.device)
    steps = torch.empty(n, dtype=torch.int32, device=d2.device)
    ws = _workspace(n, d2.device)
    _capi.call("pxsom_tsne_affinities", d2.data_ptr(), n, float(perplexity), int(bool(joint)), beta.data_ptr(),
               steps.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _capi.stream_ptr())
    return out, beta, steps


def tsne_step(P: torch.Tensor, y_in: torch.Tensor, y_out: torch.Tensor, update: torch.Tensor, gains: torch.Tensor,
              exaggeration: float, momentum: float, learning_rate: float, min_gain: float = TSNE_MIN_GAIN,
              error: Optional[torch.Tensor] = None, grad: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None) -> None:
    """One launch chain of pxsom_tsne_step.  ``y_in``, ``y_out``, ``update``, ``gains`` and ``grad`` are float64 ``[n, 2]``;
    ``error`` (float64 ``[2]``: the KL divergence and the gradient norm) asks for both."""
    if P.dim() != 2 or P.shape[0] != P.shape[1]:
        raise ValueError("P must be square")
    n = P.shape[0]
    _f64(P, (n, n), "P")
    for name, t in (("y_in", y_in), ("y_out", y_out), ("update", update), ("gains", gains)):
        _f64(t, (n, 2), name)
    if grad is not None:
        _f64(grad, (n, 2), "grad")
    if error is not None:
        _f64(error, (2,), "error")
    if y_in.data_ptr() == y_out.data_ptr():
        raise ValueError("y_in and y_out must be different buffers")
    if workspace is None:
        workspace = _workspace(n, P.device)
    _capi.call("pxsom_tsne_step", P.data_ptr(), n, y_in.data_ptr(), y_out.data_ptr(), update.data_ptr(), gains.data_ptr(),
               float(exaggeration), float(momentum), float(learning_rate), float(min_gain), int(error is not None),
               error.data_ptr() if error is not None else None, grad.data_ptr() if grad is not None else None,
               workspace.data_ptr(), workspace.numel(), _capi.stream_ptr())


def tsne_learning_rate(n: int) -> float:
    """sklearn's ``learning_rate="auto"``: ``max(n / early_exaggeration / 4, 50)``."""
    return max(n / TSNE_EARLY_EXAGGERATION / 4, 50.0)


def tsne(P: torch.Tensor, init: torch.Tensor, max_iter: int = 1000, n_iter_without_progress: int = 300) -> TsneResult:
    """sklearn's ``TSNE._tsne`` as a host loop over pxsom_tsne_step: iterations 0 .. 249 with momentum 0.5 and the
    exaggeration 12 passed as a scalar (P is never rewritten), ``update`` and ``gains`` reset, then momentum 0.8 without
    exaggeration up to ``max_iter``.  The error and the gradient norm are computed, and read back, on every 50th iteration
    and on the last of each phase, and only there."""
    n = P.shape[0]
    _f64(init, (n, 2), "init")
    if max_iter < TSNE_EXPLORATION_ITER:
        raise ValueError("max_iter must be at least %d, got %d" % (TSNE_EXPLORATION_ITER, max_iter))
    lr = tsne_learning_rate(n)
    ws = _workspace(n, P.device)
    err = torch.empty(2, dtype=torch.float64, device=P.device)
    y, y_next = init.clone(), torch.empty_like(init)
    state = {"kl": float("nan")}

    def descend(y, y_next, it, end, momentum, exaggeration, window):
        update, gains = torch.zeros_like(y), torch.ones_like(y)
        best, best_it, i = np.finfo(np.float64).max, it, it
        for i in range(it, end):
            check = (i + 1) % TSNE_ITER_CHECK == 0
            want = check or i == end - 1
            tsne_step(P, y, y_next, update, gains, exaggeration, momentum, lr, TSNE_MIN_GAIN, err if want else None,
                      workspace=ws)
            y, y_next = y_next, y
            if want:
                kl, grad_norm = err.cpu().tolist()
                state["kl"] = kl
            if check:
                if kl < best:
                    best, best_it = kl, i
                elif i - best_it > window:
                    break
                if grad_norm <= TSNE_MIN_GRAD_NORM:
                    break
        return y, y_next, i

    y, y_next, it = descend(y, y_next, 0, TSNE_EXPLORATION_ITER, 0.5, TSNE_EARLY_EXAGGERATION, TSNE_EXPLORATION_ITER)
    if it < TSNE_EXPLORATION_ITER or max_iter - TSNE_EXPLORATION_ITER > 0:
        y, y_next, it = descend(y, y_next, it + 1, max_iter, 0.8, 1.0, n_iter_without_progress)
    return TsneResult(y, state["kl"], it)


def tsne_max_rows(free_bytes: int) -> int:
    """The largest n whose P (8 n^2), d2 (4 n^2) and workspace fit in ``free_bytes``."""
    lo, hi = 0, TSNE_MAX_ROWS
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if 12 * mid * mid + tsne_workspace_bytes(mid) <= free_bytes:
            lo = mid
        else:
            hi = mid - 1
    return lo


def tsne_embed(x: torch.Tensor, perplexity: float = 30.0, max_iter: int = 1000, init="pca", random_state=None) -> TsneResult:
    """Exact t-SNE of a contiguous float32 or float64 ``[n, c]`` HBM table, end to end: distances, affinities (d2 is freed
    after them), initial embedding, descent.  ``init``: ``"pca"`` (the exact covariance route, scaled to a standard
    deviation of 1e-4 on the first component), ``"random"`` or an ``[n, 2]`` array.  NotImplementedError when
    ``12 n^2`` bytes plus the workspace exceed the free device memory."""
    n, c, _ = _table(x)
    if perplexity >= n:
        raise ValueError("perplexity must be less than n_samples")
    free = torch.cuda.mem_get_info(x.device)[0]
    need = 12 * n * n + tsne_workspace_bytes(n)
    if need > free:
        raise NotImplementedError("exact t-SNE of %d rows needs %.2f GB on the device (P, d2 and the workspace) and %.2f GB are "
                                  "free: the largest table that fits has %d rows" % (n, 1e-9 * need, 1e-9 * free,
                                                                                      tsne_max_rows(free)))
    if isinstance(init, str):
        if init == "pca":
            if c < 2:
                raise ValueError("init='pca' needs at least 2 columns")
            y0 = pca_scores(x)
            y0 = y0 / torch.std(y0[:, 0], unbiased=False) * 1e-4
        elif init == "random":
            from sklearn.utils import check_random_state
            y0 = torch.from_numpy(1e-4 * check_random_state(random_state).standard_normal((n, 2))).to(x.device)
        else:
            raise ValueError("init must be 'pca', 'random' or an [n, 2] array, got %r" % (init,))
    else:
        y0 = np.ascontiguousarray(init, dtype=np.float64)
        if y0.shape != (n, 2):
            raise ValueError("init must have shape (%d, 2), got %s" % (n, y0.shape))
        y0 = torch.from_numpy(y0).to(x.device)
    d2 = pair_sqdist_f32(x)
    P, _, _ = tsne_affinities(d2, perplexity)
    del d2
    return tsne(P, y0.contiguous(), max_iter=max_iter)
