"""SOM assign and training: BMU labels, cluster statistics, the batch and the online trainer."""
import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _capi
from ._args import _check_metric, _codebook, _matrix_args


class AssignWorkspace:
    """Scratch for pxsom_assign (``metric`` 2) or pxsom_assign_metric (1, 3, 4), reusable across calls of the same
    (n_max, c, k, metric)."""

    def __init__(self, n_max: int, c: int, k: int, device, metric: int = 2):
        if metric == 2:
            self.bytes = _capi.lib().pxsom_assign_workspace_bytes(int(n_max), int(c), int(k))
        else:
            self.bytes = _capi.lib().pxsom_assign_metric_workspace_bytes(int(n_max), int(c), int(k), int(metric))
        if self.bytes == 0:
            raise _capi.PxsomError(f"unsupported assign shape n={n_max} c={c} k={k} metric={metric}")
        self.n_max, self.c, self.k, self.metric = int(n_max), int(c), int(k), int(metric)
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)

    def fits(self, n: int, c: int, k: int, metric: int = 2) -> bool:
        return c == self.c and k == self.k and n <= self.n_max and metric == self.metric


def assign(x: torch.Tensor, w: torch.Tensor, labels: Optional[torch.Tensor] = None,
           dists: Optional[torch.Tensor] = None, want_dists: bool = False,
           workspace: Optional[AssignWorkspace] = None, screen_all_lists: bool = False,
           metric: int = 2) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """BMU labels (int32, 1-based) of every row of ``x`` against codebook ``w`` [K, C] f64.  ``screen_all_lists``: every list of
    rows for the exact path takes the long-list (screened) kernel whatever its length (PXSOM_ASSIGN_SCREEN_ALL_LISTS; same labels).
    ``metric``: FlowSOM's distf -- 2 Euclidean (pxsom_assign), 1 Manhattan, 3 Chebyshev, 4 cosine (pxsom_assign_metric, which
    has no screen and so no lists: ``screen_all_lists`` is Euclidean-only and refused with another metric)."""
    metric = _check_metric(metric)
    if screen_all_lists and metric != 2:
        raise ValueError("screen_all_lists applies to the Euclidean route only (metric 2)")
    n, c, ldx, dt = _matrix_args(x)
    w = _codebook(w)
    k = w.shape[0]
    if w.shape[1] != c:
        raise ValueError(f"codebook has {w.shape[1]} channels, matrix has {c}")
    if labels is None:
        labels = torch.empty(n, dtype=torch.int32, device=x.device)
    if want_dists and dists is None:
        dists = torch.empty(n, dtype=torch.float64, device=x.device)
    if workspace is None or not workspace.fits(n, c, k, metric):
        workspace = AssignWorkspace(n, c, k, x.device, metric)
    if metric != 2:
        _capi.call("pxsom_assign_metric", x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k, labels.data_ptr(),
                   dists.data_ptr() if dists is not None else None,
                   workspace.buf.data_ptr(), workspace.bytes, metric, _capi.stream_ptr())
        assign.last_workspace = workspace
        return labels, dists
    _capi.call("pxsom_assign_ex", x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k, labels.data_ptr(),
               dists.data_ptr() if dists is not None else None,
               workspace.buf.data_ptr(), workspace.bytes, ASSIGN_SCREEN_ALL_LISTS if screen_all_lists else 0,
               _capi.stream_ptr())
    assign.last_workspace = workspace
    return labels, dists


def last_exact_rows(workspace: AssignWorkspace) -> int:
    out = ctypes.c_int64(0)
    _capi.call("pxsom_assign_last_exact_rows", workspace.buf.data_ptr() + getattr(workspace, "assign_offset", 0), _capi.stream_ptr(),
               ctypes.byref(out))
    return int(out.value)


def cluster_sums(x: torch.Tensor, labels: torch.Tensor, k: int,
                 sums: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None):
    """Adds per-label channel sums [k, C] f64 and counts [k] i64 of the rows of ``x``."""
    n, c, ldx, dt = _matrix_args(x)
    if labels.dtype != torch.int32 or labels.numel() != n or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int32 vector with one entry per row")
    if sums is None:
        sums = torch.zeros((k, c), dtype=torch.float64, device=x.device)
    if counts is None:
        counts = torch.zeros(k, dtype=torch.int64, device=x.device)
    _capi.call("pxsom_cluster_sums", x.data_ptr(), n, c, ldx, dt, labels.data_ptr(), int(k),
               sums.data_ptr(), counts.data_ptr(), _capi.stream_ptr())
    return sums, counts


TRAIN_UNFUSED = 1  # include/pxsom.h PXSOM_TRAIN_UNFUSED
ASSIGN_SCREEN_ALL_LISTS = 1  # include/pxsom.h PXSOM_ASSIGN_SCREEN_ALL_LISTS


class BatchTrainState:
    """Caller-owned state of ``pxsom_batch_train_sched``: the codebook twin buffer ``wbuf`` [2, K, C], the
    rotating statistics ``ring`` [3, K*(C+1)] (float64; ``ring[g % 3]`` is what a multi-rank job all-reduces
    after step g) and the scratch workspace for ``n`` training rows of ``dtype`` (default: the widest, so that the
    state fits any matrix) on ``schedule`` (an int: that many equal steps per pass).  ``metric``: FlowSOM's distf of the run's
    BMU search (2 Euclidean: pxsom_batch_train_sched; 1, 3, 4: pxsom_batch_train_sched_metric, whose workspace is another)."""

    def __init__(self, n: int, c: int, xdim: int, ydim: int, schedule, device, dtype=torch.float64, metric: int = 2):
        from ..schedule import resolve
        self.n, self.c, self.xdim, self.ydim = int(n), int(c), int(xdim), int(ydim)
        self.k, self.schedule, self.dtype = self.xdim * self.ydim, resolve(schedule), dtype
        self.metric = _check_metric(metric)
        self.batch_steps = self.schedule.steps
        self.edges = self.schedule.edges_array()            # host array handed to every call (kept alive here)
        sized = (self.n, self.c, self.k, _capi.dtype_code(torch.empty(0, dtype=dtype)), self.schedule.phases,
                 self.edges.ctypes.data, self.schedule.steps)
        self.ws_bytes = _capi.lib().pxsom_batch_train_sched_workspace_bytes(*sized) if self.metric == 2 else \
            _capi.lib().pxsom_batch_train_sched_metric_workspace_bytes(*sized, self.metric)
        if self.ws_bytes == 0:
            raise _capi.PxsomError(f"unsupported batch-training shape n={n} c={c} k={self.k}")
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.wbuf = torch.empty((2, self.k, self.c), dtype=torch.float64, device=device)
        self.ring = torch.zeros((3, self.k * (self.c + 1)), dtype=torch.float64, device=device)
        self.quantum = 0.0      # > 0: binary64 rows join the statistics rounded to its multiples (exact, order-free sums)

    def fits(self, n: int, c: int, xdim: int, ydim: int, schedule, dtype=None, metric: int = 2) -> bool:
        from ..schedule import resolve
        return (c == self.c and xdim == self.xdim and ydim == self.ydim and resolve(schedule) == self.schedule
                and metric == self.metric
                and n <= self.n and (dtype is None or torch.empty(0, dtype=dtype).element_size()
                                     <= torch.empty(0, dtype=self.dtype).element_size()))


def absmax(x: torch.Tensor) -> torch.Tensor:
    """max |x| over the finite entries of a matrix, as a 1-element float64 HBM tensor (0 when there is none)."""
    n, c, ldx, dt = _matrix_args(x)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    _capi.call("pxsom_absmax", x.data_ptr(), n, c, ldx, dt, out.data_ptr(), _capi.stream_ptr())
    return out


def exact_sum_quantum(value_bound: float, rows_bound: int) -> float:
    """The power of two q for which sums of at most ``rows_bound`` multiples of q below ``value_bound`` are exact in binary64
    (include/pxsom.h "Reproducible statistics"); 0 for all-zero data.  Host arithmetic, no GPU."""
    return float(_capi.lib().pxsom_exact_sum_quantum(float(value_bound), int(rows_bound)))


def batch_train_fused_route(x: torch.Tensor, xdim: int, ydim: int, schedule) -> bool:
    """Whether the steps of this matrix take the one-launch fused kernel (a multi-rank job agrees on the route before
    it starts: include/pxsom.h pxsom_batch_train_fused_route)."""
    from ..schedule import resolve
    n, c, ldx, dt = _matrix_args(x)
    return bool(_capi.lib().pxsom_batch_train_fused_route(x.data_ptr(), c, ldx, dt, int(xdim), int(ydim),
                                                          resolve(schedule).phases))


ONLINE_ROUTE_FIELDS = ("family", "width", "span", "in_place", "threads", "chunk", "lds_bytes")
ONLINE_LANES_PER_NODE, ONLINE_THREAD_PER_NODE = 0, 1


def train_online_route(c: int, xdim: int, ydim: int, dtype: int = _capi.PXSOM_F32, metric: int = 2) -> dict:
    """The launch ``train_online`` would make for rows of ``c`` channels (``dtype``: a PXSOM_F* code) on an
    ``xdim`` x ``ydim`` map under ``metric``, by the library's own planning function (include/pxsom.h
    pxsom_train_online_route): family, width (CH | CMAX), span (L | MAXT), in_place, threads, chunk, lds_bytes.  Raises the
    PxsomError the training call would raise for the shape.  Host arithmetic: no GPU needed."""
    out = np.empty(len(ONLINE_ROUTE_FIELDS), dtype=np.int32)
    _capi.call("pxsom_train_online_route", int(c), int(xdim), int(ydim), int(dtype), int(metric), out.ctypes.data)
    return dict(zip(ONLINE_ROUTE_FIELDS, (int(v) for v in out)))


def train_online_routes(shapes) -> np.ndarray:
    """``train_online_route`` for a table of shapes at once: ``shapes`` [count, 5] int32 rows (c, xdim, ydim, dtype,
    metric); returns [count, 1 + 7] int32 rows (status, then ONLINE_ROUTE_FIELDS -- all -1 where the status is not 0)."""
    shapes = np.ascontiguousarray(shapes, dtype=np.int32)
    if shapes.ndim != 2 or shapes.shape[1] != 5:
        raise ValueError("shapes must be [count, 5]: c, xdim, ydim, dtype, metric")
    out = np.empty((shapes.shape[0], 1 + len(ONLINE_ROUTE_FIELDS)), dtype=np.int32)
    _capi.call("pxsom_train_online_routes", shapes.shape[0], shapes.ctypes.data, out.ctypes.data)
    return out


def batch_train_steps(x: torch.Tensor, state: BatchTrainState, g_begin: int, g_end: int, total_steps: int,
                      alpha_range, radius_range, unfused: bool = False, comm: "RankComm" = None,
                      w0: Optional[torch.Tensor] = None) -> None:
    """Mini-batch steps [g_begin, g_end) of a batch training run of ``total_steps`` = passes x steps per pass, launched
    back to back by the library (``state.wbuf[0]`` holds W_0 before step 0; see include/pxsom.h).  ``comm``: the
    statistics of every step are sum-all-reduced over its ranks right behind the step's launch (every rank makes the
    same call).  ``w0`` (with ``g_begin == 0``): the run's first codebook where the caller holds it -- the launch that prepares the
    run copies it into ``state.wbuf[0]`` (pxsom_batch_train_sched_from: no copy launch in front of the pass).
    ``state.metric`` 1 / 3 / 4: pxsom_batch_train_sched_metric, which has no exchange inside the library -- a ``comm`` is refused
    (a multi-rank run makes one call per step and all-reduces ``state.ring[g % 3]`` in between)."""
    if state.metric != 2 and comm is not None:
        raise ValueError("no in-library exchange under metric %d: run one step per call and all-reduce the ring" % state.metric)
    n, c, ldx, dt = _matrix_args(x)
    if w0 is not None:
        w0 = _codebook(w0)
        if tuple(w0.shape) != (state.xdim * state.ydim, c):
            raise ValueError("w0 does not match the state's codebook")
    if not state.fits(n, c, state.xdim, state.ydim, state.schedule, x.dtype, state.metric):
        raise ValueError("batch-training state does not fit this matrix")
    sch = state.schedule
    if int(total_steps) % sch.steps:
        raise ValueError("total_steps must be a whole number of passes")
    if state.metric != 2:
        _capi.call(
            "pxsom_batch_train_sched_metric",
            x.data_ptr(), n, c, ldx, dt, w0.data_ptr() if (w0 is not None and int(g_begin) == 0) else None,
            state.wbuf.data_ptr(), state.ring.data_ptr(), state.xdim, state.ydim,
            sch.phases, state.edges.ctypes.data, sch.steps, int(g_begin), int(g_end), int(total_steps) // sch.steps,
            float(alpha_range[0]), float(alpha_range[1]), float(radius_range[0]), float(radius_range[1]), float(state.quantum),
            state.ws.data_ptr(), state.ws_bytes, 0, None, state.metric, _capi.stream_ptr())
        return
    _capi.call(
        "pxsom_batch_train_sched_from",
        x.data_ptr(), n, c, ldx, dt, w0.data_ptr() if (w0 is not None and int(g_begin) == 0) else None,
        state.wbuf.data_ptr(), state.ring.data_ptr(), state.xdim, state.ydim,
        sch.phases, state.edges.ctypes.data, sch.steps, int(g_begin), int(g_end), int(total_steps) // sch.steps,
        float(alpha_range[0]), float(alpha_range[1]), float(radius_range[0]), float(radius_range[1]), float(state.quantum),
        state.ws.data_ptr(), state.ws_bytes, TRAIN_UNFUSED if unfused else 0,
        comm.handle if comm is not None else None, _capi.stream_ptr())


def batch_train_finish(state: BatchTrainState, steps_done: int, total_steps: int, alpha_range, radius_range,
                       w_out: torch.Tensor) -> None:
    """Applies the last pending update of a run: ``w_out`` [K, C] receives the codebook after ``steps_done`` steps."""
    w_out = _codebook(w_out)
    sch = state.schedule
    _capi.call(
        "pxsom_batch_train_sched_finish",
        state.wbuf.data_ptr(), state.ring.data_ptr(), state.xdim, state.ydim, state.c, sch.phases,
        state.edges.ctypes.data, sch.steps, int(steps_done), int(total_steps) // sch.steps, float(alpha_range[0]),
        float(alpha_range[1]), float(radius_range[0]), float(radius_range[1]), w_out.data_ptr(), _capi.stream_ptr())


ACC_PREPARED = 1  # include/pxsom.h PXSOM_ACC_PREPARED


def batch_accumulate(x: torch.Tensor, w: torch.Tensor, labels: torch.Tensor, stats: torch.Tensor,
                     workspace: AssignWorkspace, prepared: bool = False) -> None:
    """Zero ``stats`` ([K*C sums | K counts], float64), label every row of ``x`` and accumulate.
    ``prepared``: ``batch_update_prepare`` already cleared ``stats`` (and, for shapes the accumulating filter
    does not prepare itself, readied ``workspace`` for ``w``): no memset, no prep launch."""
    n, c, ldx, dt = _matrix_args(x)
    w = _codebook(w)
    k = w.shape[0]
    if not workspace.fits(n, c, k):
        raise ValueError("assign workspace too small for this mini-batch")
    if labels.dtype != torch.int32 or labels.numel() < n:
        raise ValueError("labels scratch must be int32 with at least n entries")
    if stats.dtype != torch.float64 or stats.numel() != k * (c + 1) or not stats.is_contiguous():
        raise ValueError("stats must be a contiguous float64 vector of K*(C+1) entries")
    _capi.call("pxsom_batch_accumulate", x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k,
               labels.data_ptr(), stats.data_ptr(),
               workspace.buf.data_ptr(), workspace.bytes,
               ACC_PREPARED if prepared else 0, _capi.stream_ptr())


def batch_update_prepare(w: torch.Tensor, xdim: int, ydim: int, stats: torch.Tensor, thr: float,
                         alpha: float, workspace: Optional[AssignWorkspace],
                         stats_next: Optional[torch.Tensor] = None) -> None:
    """Batch-rule codebook update from ``stats`` ([K*C sums | K counts], all-reduced), in place on ``w``.
    ``stats_next`` -- the buffer the next accumulate fills (alternate two) -- is cleared by the same launch
    (``None``: ``stats`` itself is cleared afterwards); ``workspace`` is prepared for the new codebook where
    the shape needs that.  Next accumulate: ``prepared=True``."""
    w = _codebook(w)
    k, c = w.shape
    if k != xdim * ydim:
        raise ValueError(f"codebook has {k} nodes, grid is {xdim}x{ydim}")
    if stats.dtype != torch.float64 or stats.numel() != k * (c + 1) or not stats.is_contiguous():
        raise ValueError("stats must be a contiguous float64 vector of K*(C+1) entries")
    if stats_next is not None and (stats_next.dtype != torch.float64 or stats_next.numel() != stats.numel()
                                   or not stats_next.is_contiguous()):
        raise ValueError("stats_next must look like stats")
    _capi.call("pxsom_batch_update_prepare", w.data_ptr(), int(xdim), int(ydim), c, stats.data_ptr(),
               stats_next.data_ptr() if stats_next is not None else None,
               float(thr), float(alpha),
               workspace.buf.data_ptr() if workspace is not None else None,
               workspace.bytes if workspace is not None else 0,
               _capi.stream_ptr())


ONLINE_INT_ABS = 1  # include/pxsom.h PXSOM_ONLINE_INT_ABS


def train_online(x: torch.Tensor, w: torch.Tensor, xdim: int, ydim: int, rlen: int,
                 alpha_range, radius_range, order: torch.Tensor, int_abs: bool = False, metric: int = 2) -> torch.Tensor:
    """Exact online SOM (FlowSOM C_SOM) in place on ``w`` [xdim*ydim, C] f64.  ``int_abs``: the other reading of the
    early-stop accumulator (``flowsom.RECALLED["change_abs"]``).  ``metric``: FlowSOM's distf of the BMU search (2 Euclidean:
    pxsom_train_online_ex; 1 Manhattan, 3 Chebyshev, 4 cosine: pxsom_train_online_metric)."""
    metric = _check_metric(metric)
    n, c, ldx, dt = _matrix_args(x)
    w = _codebook(w)
    if w.shape != (xdim * ydim, c):
        raise ValueError(f"codebook shape {tuple(w.shape)} != ({xdim * ydim}, {c})")
    if order.dtype != torch.int64 or not order.is_cuda or order.numel() != n * rlen:
        raise ValueError("order must be an int64 HBM vector of n*rlen row indices")
    if metric != 2:
        _capi.call("pxsom_train_online_metric", x.data_ptr(), n, c, ldx, dt, w.data_ptr(), int(xdim), int(ydim), int(rlen),
                   float(alpha_range[0]), float(alpha_range[1]), float(radius_range[0]),
                   float(radius_range[1]), order.data_ptr(), metric,
                   ONLINE_INT_ABS if int_abs else 0, _capi.stream_ptr())
        return w
    _capi.call("pxsom_train_online_ex", x.data_ptr(), n, c, ldx, dt, w.data_ptr(), int(xdim),
               int(ydim), int(rlen), float(alpha_range[0]),
               float(alpha_range[1]), float(radius_range[0]),
               float(radius_range[1]), order.data_ptr(),
               ONLINE_INT_ABS if int_abs else 0, _capi.stream_ptr())
    return w


def batch_update(w: torch.Tensor, xdim: int, ydim: int, sums: torch.Tensor, counts: torch.Tensor,
                 thr: float, alpha: float) -> torch.Tensor:
    w = _codebook(w)
    c = w.shape[1]
    if sums.dtype != torch.float64 or counts.dtype != torch.float64:
        raise ValueError("sums and counts must be float64 (counts are exact integers)")
    _capi.call("pxsom_batch_update", w.data_ptr(), int(xdim), int(ydim), c, sums.data_ptr(),
               counts.data_ptr(), float(thr), float(alpha),
               _capi.stream_ptr())
    return w


class AssignSumsWorkspace:
    """Scratch for pxsom_assign_sums, reusable across calls of the same (n_max, c, k)."""

    def __init__(self, n_max: int, c: int, k: int, device):
        self.bytes = _capi.lib().pxsom_assign_sums_workspace_bytes(int(n_max), int(c), int(k))
        if self.bytes == 0:
            raise _capi.PxsomError(f"unsupported assign shape n={n_max} c={c} k={k}")
        self.n_max, self.c, self.k = int(n_max), int(c), int(k)
        # cleared ONCE: the library leaves the statistics region at its head zero after every successful call, and skips its own
        # clearing launch while ``clean`` says so (PXSOM_TABLES_SCRATCH_CLEAN); a failed call drops the promise
        self.buf = torch.zeros(self.bytes, dtype=torch.uint8, device=device)
        self.clean = True
        self.assign_offset = int(_capi.lib().pxsom_assign_sums_scratch_bytes(int(c), int(k)))   # where the assign workspace begins

    def fits(self, n: int, c: int, k: int) -> bool:
        return c == self.c and k == self.k and n <= self.n_max


TABLES_SCRATCH_CLEAN = 1  # include/pxsom.h PXSOM_TABLES_SCRATCH_CLEAN


def _with_scratch_flag(workspace: AssignSumsWorkspace, n: int, what: str, call) -> None:
    """``call(flags)`` with PXSOM_TABLES_SCRATCH_CLEAN while the workspace vouches for a zero statistics region.  It is
    vouched for again only after a call that ran over rows (which leaves the region zero) or cleared the region itself
    (no flag); an empty call with the flag touches nothing, and the next call clears once more; a failed call drops the
    promise."""
    flags, workspace.clean = (TABLES_SCRATCH_CLEAN if workspace.clean else 0), False
    _capi.check(call(flags), what)
    workspace.clean = n > 0 or not flags


def assign_sums(x: torch.Tensor, w: torch.Tensor, labels: Optional[torch.Tensor] = None,
                sums: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                workspace: Optional[AssignSumsWorkspace] = None):
    """BMU labels of every row AND the per-label channel sums [K, C] f64 / counts [K] i64 (added into ``sums`` /
    ``counts``), reading ``x`` once where the shape allows.  Returns ``(labels, sums, counts)``."""
    n, c, ldx, dt = _matrix_args(x)
    w = _codebook(w)
    k = w.shape[0]
    if labels is None:
        labels = torch.empty(n, dtype=torch.int32, device=x.device)
    if sums is None:
        sums = torch.zeros((k, c), dtype=torch.float64, device=x.device)
    if counts is None:
        counts = torch.zeros(k, dtype=torch.int64, device=x.device)
    if workspace is None or not workspace.fits(n, c, k):
        workspace = AssignSumsWorkspace(n, c, k, x.device)
    _with_scratch_flag(workspace, n, "pxsom_assign_sums_ex", lambda flags: _capi.lib().pxsom_assign_sums_ex(
        x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k, labels.data_ptr(), sums.data_ptr(), counts.data_ptr(),
        workspace.buf.data_ptr(), workspace.bytes, flags, _capi.stream_ptr()))
    return labels, sums, counts


class MetricStepWorkspace:
    """Scratch for pxsom_assign_sums_metric (metric 1, 3, 4): the prepared codebook of a (c, k); any row count."""

    def __init__(self, c: int, k: int, device, metric: int):
        self.bytes = _capi.lib().pxsom_metric_step_workspace_bytes(int(c), int(k), int(metric))
        if self.bytes == 0:
            raise _capi.PxsomError(f"unsupported shape c={c} k={k} metric={metric} (metric 2: assign_sums / batch_accumulate)")
        self.c, self.k, self.metric = int(c), int(k), int(metric)
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)

    def fits(self, c: int, k: int, metric: int) -> bool:
        return c == self.c and k == self.k and metric == self.metric


def assign_sums_metric(x: torch.Tensor, w: torch.Tensor, metric: int, labels: Optional[torch.Tensor] = None,
                       stats: Optional[torch.Tensor] = None, quantum: float = 0.0, window=(1, 0, 1),
                       workspace: Optional[MetricStepWorkspace] = None):
    """BMU labels under FlowSOM's distf 1 / 3 / 4 AND the batch statistics of the labelled rows in one pass over ``x``
    (pxsom_assign_sums_metric).  ``window`` = (phases, e0, e1): row i takes part iff e0 <= i % phases < e1; the labels of the
    other rows are left as they are (a new ``labels`` vector starts at zero).  ``stats`` [K*C sums | K counts] float64 is ADDED
    into (zeros if not given); ``quantum``: binary64 rows join the sums rounded to its multiples (``exact_sum_quantum``).
    Returns ``(labels, stats)``."""
    metric = _check_metric(metric)
    n, c, ldx, dt = _matrix_args(x)
    w = _codebook(w)
    k = w.shape[0]
    if w.shape[1] != c:
        raise ValueError(f"codebook has {w.shape[1]} channels, matrix has {c}")
    phases, e0, e1 = (int(v) for v in window)
    if labels is None:
        labels = torch.zeros(n, dtype=torch.int32, device=x.device)
    elif labels.dtype != torch.int32 or labels.numel() != n or not labels.is_contiguous() or not labels.is_cuda:
        raise ValueError("labels must be a contiguous int32 HBM vector with one entry per row")
    if stats is None:
        stats = torch.zeros(k * (c + 1), dtype=torch.float64, device=x.device)
    elif stats.dtype != torch.float64 or stats.numel() != k * (c + 1) or not stats.is_contiguous() or not stats.is_cuda:
        raise ValueError("stats must be a contiguous float64 HBM vector of K*(C+1) entries")
    if workspace is None or not workspace.fits(c, k, metric):
        workspace = MetricStepWorkspace(c, k, x.device, metric)
    _capi.call("pxsom_assign_sums_metric", x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k, phases, e0, e1, labels.data_ptr(),
               stats.data_ptr(), float(quantum), workspace.buf.data_ptr(), workspace.bytes, metric, _capi.stream_ptr())
    return labels, stats


def assign_means(x: torch.Tensor, w: torch.Tensor, labels: torch.Tensor, sums: torch.Tensor, counts: torch.Tensor,
                 means: Optional[torch.Tensor], workspace: AssignSumsWorkspace) -> None:
    """Labels, per-cluster sums / counts (OVERWRITTEN) and means = sums / max(count, 1) in one library call and one pass
    over ``x`` where the shape allows (pxsom_assign_means)."""
    n, c, ldx, dt = _matrix_args(x)
    w = _codebook(w)
    k = w.shape[0]
    if not workspace.fits(n, c, k):
        raise ValueError("workspace does not fit this matrix")
    _with_scratch_flag(workspace, n, "pxsom_assign_means_ex", lambda flags: _capi.lib().pxsom_assign_means_ex(
        x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k, labels.data_ptr(), sums.data_ptr(), counts.data_ptr(),
        means.data_ptr() if means is not None else None, workspace.buf.data_ptr(), workspace.bytes, flags,
        _capi.stream_ptr()))


def relabel(labels: torch.Tensor, lut: torch.Tensor, fill: int = -1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[i] = lut[labels[i]]`` (``fill`` for labels outside the table): SOM cluster -> meta cluster for labels
    that live in HBM.  int32 vectors; ``out`` may be ``labels``."""
    if labels.dtype != torch.int32 or lut.dtype != torch.int32 or not labels.is_cuda or not labels.is_contiguous():
        raise ValueError("labels and lut must be contiguous int32 HBM vectors")
    if out is None:
        out = torch.empty_like(labels)
    _capi.call("pxsom_relabel", labels.data_ptr(), labels.numel(), lut.contiguous().data_ptr(), lut.numel(), int(fill),
               out.data_ptr(), _capi.stream_ptr())
    return out


def pair_histogram(a: torch.Tensor, b: torch.Tensor, na: int, nb: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[a_i, b_i] += 1`` over two int32 HBM vectors (pairs outside [0, na) x [0, nb) are ignored);
    ``out`` [na, nb] int64 (zeros if not given)."""
    if a.dtype != torch.int32 or b.dtype != torch.int32 or a.numel() != b.numel() or not a.is_cuda:
        raise ValueError("a and b must be int32 HBM vectors of the same length")
    a, b = a.contiguous(), b.contiguous()
    if out is None:
        out = torch.zeros((int(na), int(nb)), dtype=torch.int64, device=a.device)
    _capi.call("pxsom_pair_histogram", a.data_ptr(), b.data_ptr(), a.numel(), int(na), int(nb),
               out.data_ptr(), _capi.stream_ptr())
    return out
