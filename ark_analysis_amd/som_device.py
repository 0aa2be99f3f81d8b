"""Device-level SOM operations: thin, typed wrappers over the C ABI working on torch tensors.

Tensors are only device-memory holders here (``data_ptr()`` goes across the ABI); every
function launches on torch's current HIP stream and returns without synchronising.
"""
import operator
from typing import Optional, Tuple

import numpy as np
import torch

from . import _capi


def _matrix_args(x: torch.Tensor) -> Tuple[int, int, int, int]:
    if x.dim() != 2:
        raise ValueError("pixel matrix must be 2-D [rows, channels]")
    if not x.is_cuda:
        raise ValueError("pixel matrix must live in HBM (a cuda/HIP tensor)")
    n, c = x.shape
    if n == 0:                         # an empty shard (more ranks than rows): no element, no stride to check
        return 0, c, c, _capi.dtype_code(x)
    if c > 1 and x.stride(1) != 1:     # (a single column has no second stride to speak of: torch reports anything)
        raise ValueError("pixel matrix rows must be contiguous (stride(1) == 1)")
    ldx = x.stride(0) if n > 1 else max(c, x.stride(0))
    return n, c, ldx, _capi.dtype_code(x)


def _codebook(w: torch.Tensor) -> torch.Tensor:
    if w.dtype != torch.float64 or not w.is_cuda or not w.is_contiguous() or w.dim() != 2:
        raise ValueError("codebook must be a contiguous float64 [K, C] HBM tensor")
    return w


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


def _check_metric(metric: int) -> int:
    code = None
    if not isinstance(metric, (bool, np.bool_)):
        try:
            code = operator.index(metric)
        except TypeError:
            pass
    if code not in _capi.METRICS:
        raise ValueError(f"unknown metric {metric!r}: FlowSOM distf 1 (Manhattan), 2 (Euclidean), 3 (Chebyshev) "
                         f"or 4 (cosine)")
    return code


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
        rc = _capi.lib().pxsom_assign_metric(x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k, labels.data_ptr(),
                                             dists.data_ptr() if dists is not None else None,
                                             workspace.buf.data_ptr(), workspace.bytes, metric, _capi.stream_ptr())
        _capi.check(rc, "pxsom_assign_metric")
        assign.last_workspace = workspace
        return labels, dists
    rc = _capi.lib().pxsom_assign_ex(x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k, labels.data_ptr(),
                                     dists.data_ptr() if dists is not None else None,
                                     workspace.buf.data_ptr(), workspace.bytes, ASSIGN_SCREEN_ALL_LISTS if screen_all_lists else 0,
                                     _capi.stream_ptr())
    _capi.check(rc, "pxsom_assign_ex")
    assign.last_workspace = workspace
    return labels, dists


def last_exact_rows(workspace: AssignWorkspace) -> int:
    import ctypes
    out = ctypes.c_int64(0)
    _capi.check(_capi.lib().pxsom_assign_last_exact_rows(workspace.buf.data_ptr() + getattr(workspace, "assign_offset", 0), _capi.stream_ptr(),
                                                         ctypes.byref(out)),
                "pxsom_assign_last_exact_rows")
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
    rc = _capi.lib().pxsom_cluster_sums(x.data_ptr(), n, c, ldx, dt, labels.data_ptr(), int(k),
                                        sums.data_ptr(), counts.data_ptr(), _capi.stream_ptr())
    _capi.check(rc, "pxsom_cluster_sums")
    return sums, counts


TRAIN_UNFUSED = 1  # include/pxsom.h PXSOM_TRAIN_UNFUSED
ASSIGN_SCREEN_ALL_LISTS = 1  # include/pxsom.h PXSOM_ASSIGN_SCREEN_ALL_LISTS


class BatchTrainState:
    """Caller-owned state of ``pxsom_batch_train_sched``: the codebook twin buffer ``wbuf`` [2, K, C], the
    rotating statistics ``ring`` [3, K*(C+1)] (float64; ``ring[g % 3]`` is what a multi-rank job all-reduces
    after step g) and the scratch workspace for ``n`` training rows of ``dtype`` (default: the widest, so that the
    state fits any matrix) on ``schedule`` (an int: that many equal steps per pass)."""

    def __init__(self, n: int, c: int, xdim: int, ydim: int, schedule, device, dtype=torch.float64):
        from .schedule import resolve
        self.n, self.c, self.xdim, self.ydim = int(n), int(c), int(xdim), int(ydim)
        self.k, self.schedule, self.dtype = self.xdim * self.ydim, resolve(schedule), dtype
        self.batch_steps = self.schedule.steps
        self.edges = self.schedule.edges_array()            # host array handed to every call (kept alive here)
        self.ws_bytes = _capi.lib().pxsom_batch_train_sched_workspace_bytes(
            self.n, self.c, self.k, _capi.dtype_code(torch.empty(0, dtype=dtype)), self.schedule.phases,
            self.edges.ctypes.data, self.schedule.steps)
        if self.ws_bytes == 0:
            raise _capi.PxsomError(f"unsupported batch-training shape n={n} c={c} k={self.k}")
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.wbuf = torch.empty((2, self.k, self.c), dtype=torch.float64, device=device)
        self.ring = torch.zeros((3, self.k * (self.c + 1)), dtype=torch.float64, device=device)
        self.quantum = 0.0      # > 0: binary64 rows join the statistics rounded to its multiples (exact, order-free sums)

    def fits(self, n: int, c: int, xdim: int, ydim: int, schedule, dtype=None) -> bool:
        from .schedule import resolve
        return (c == self.c and xdim == self.xdim and ydim == self.ydim and resolve(schedule) == self.schedule
                and n <= self.n and (dtype is None or torch.empty(0, dtype=dtype).element_size()
                                     <= torch.empty(0, dtype=self.dtype).element_size()))


def absmax(x: torch.Tensor) -> torch.Tensor:
    """max |x| over the finite entries of a matrix, as a 1-element float64 HBM tensor (0 when there is none)."""
    n, c, ldx, dt = _matrix_args(x)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    _capi.check(_capi.lib().pxsom_absmax(x.data_ptr(), n, c, ldx, dt, out.data_ptr(), _capi.stream_ptr()), "pxsom_absmax")
    return out


def exact_sum_quantum(value_bound: float, rows_bound: int) -> float:
    """The power of two q for which sums of at most ``rows_bound`` multiples of q below ``value_bound`` are exact in binary64
    (include/pxsom.h "Reproducible statistics"); 0 for all-zero data.  Host arithmetic, no GPU."""
    return float(_capi.lib().pxsom_exact_sum_quantum(float(value_bound), int(rows_bound)))


def batch_train_fused_route(x: torch.Tensor, xdim: int, ydim: int, schedule) -> bool:
    """Whether the steps of this matrix take the one-launch fused kernel (a multi-rank job agrees on the route before
    it starts: include/pxsom.h pxsom_batch_train_fused_route)."""
    from .schedule import resolve
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
    rc = _capi.lib().pxsom_train_online_route(int(c), int(xdim), int(ydim), int(dtype), int(metric), out.ctypes.data)
    _capi.check(rc, "pxsom_train_online_route")
    return dict(zip(ONLINE_ROUTE_FIELDS, (int(v) for v in out)))


def train_online_routes(shapes) -> np.ndarray:
    """``train_online_route`` for a table of shapes at once: ``shapes`` [count, 5] int32 rows (c, xdim, ydim, dtype,
    metric); returns [count, 1 + 7] int32 rows (status, then ONLINE_ROUTE_FIELDS -- all -1 where the status is not 0)."""
    shapes = np.ascontiguousarray(shapes, dtype=np.int32)
    if shapes.ndim != 2 or shapes.shape[1] != 5:
        raise ValueError("shapes must be [count, 5]: c, xdim, ydim, dtype, metric")
    out = np.empty((shapes.shape[0], 1 + len(ONLINE_ROUTE_FIELDS)), dtype=np.int32)
    _capi.check(_capi.lib().pxsom_train_online_routes(shapes.shape[0], shapes.ctypes.data, out.ctypes.data),
                "pxsom_train_online_routes")
    return out


def batch_train_steps(x: torch.Tensor, state: BatchTrainState, g_begin: int, g_end: int, total_steps: int,
                      alpha_range, radius_range, unfused: bool = False, comm: "RankComm" = None,
                      w0: Optional[torch.Tensor] = None) -> None:
    """Mini-batch steps [g_begin, g_end) of a batch training run of ``total_steps`` = passes x steps per pass, launched
    back to back by the library (``state.wbuf[0]`` holds W_0 before step 0; see include/pxsom.h).  ``comm``: the
    statistics of every step are sum-all-reduced over its ranks right behind the step's launch (every rank makes the
    same call).  ``w0`` (with ``g_begin == 0``): the run's first codebook where the caller holds it -- the launch that prepares the
    run copies it into ``state.wbuf[0]`` (pxsom_batch_train_sched_from: no copy launch in front of the pass)."""
    n, c, ldx, dt = _matrix_args(x)
    if w0 is not None:
        w0 = _codebook(w0)
        if tuple(w0.shape) != (state.xdim * state.ydim, c):
            raise ValueError("w0 does not match the state's codebook")
    if not state.fits(n, c, state.xdim, state.ydim, state.schedule, x.dtype):
        raise ValueError("batch-training state does not fit this matrix")
    sch = state.schedule
    if int(total_steps) % sch.steps:
        raise ValueError("total_steps must be a whole number of passes")
    rc = _capi.lib().pxsom_batch_train_sched_from(
        x.data_ptr(), n, c, ldx, dt, w0.data_ptr() if (w0 is not None and int(g_begin) == 0) else None,
        state.wbuf.data_ptr(), state.ring.data_ptr(), state.xdim, state.ydim,
        sch.phases, state.edges.ctypes.data, sch.steps, int(g_begin), int(g_end), int(total_steps) // sch.steps,
        float(alpha_range[0]), float(alpha_range[1]), float(radius_range[0]), float(radius_range[1]), float(state.quantum),
        state.ws.data_ptr(), state.ws_bytes, TRAIN_UNFUSED if unfused else 0,
        comm.handle if comm is not None else None, _capi.stream_ptr())
    _capi.check(rc, "pxsom_batch_train_sched_from")


COMM_ID_BYTES = 128  # include/pxsom.h PXSOM_COMM_ID_BYTES


def _torch_rccl_path() -> str:
    """The librccl.so this process already uses: PyTorch's own copy (binding a second RCCL next to it is
    what pxsom_comm_bind exists to avoid); empty = let the library fall back to the system one."""
    import os
    override = os.environ.get("PXSOM_RCCL_LIBRARY")     # another build of the collective library (tests: a stand-in)
    if override:
        return override
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    return path if os.path.exists(path) else ""


class RankComm:
    """RCCL communicator owned by libpxsom (pxsom_comm_*): what the in-library exchange of a multi-rank batch
    run reduces over.  ``RankComm.unique_id()`` on one rank, the 128 bytes handed to the others by the
    launcher's channel, then ``RankComm(id, nranks, rank)`` on every rank (collective) with its device current."""

    def __init__(self, uid: bytes, nranks: int, rank: int):
        import ctypes
        self.bind()
        if len(uid) != COMM_ID_BYTES:
            raise ValueError("communicator id must be %d bytes" % COMM_ID_BYTES)
        box = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        rc = _capi.lib().pxsom_comm_create(ctypes.cast(buf, ctypes.c_void_p), COMM_ID_BYTES, int(nranks), int(rank),
                                           ctypes.byref(box))
        _capi.check(rc, "pxsom_comm_create")
        self.handle = box
        self.nranks, self.rank = int(nranks), int(rank)

    @staticmethod
    def bind() -> None:
        rc = _capi.lib().pxsom_comm_bind(_torch_rccl_path().encode())
        _capi.check(rc, "pxsom_comm_bind")

    @staticmethod
    def unique_id() -> bytes:
        import ctypes
        RankComm.bind()
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        rc = _capi.lib().pxsom_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p), COMM_ID_BYTES)
        _capi.check(rc, "pxsom_comm_unique_id")
        return buf.raw

    def allreduce_sum(self, t: torch.Tensor) -> None:
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("the exchange reduces contiguous float64 buffers")
        rc = _capi.lib().pxsom_comm_allreduce_sum_f64(self.handle, t.data_ptr(), t.numel(), _capi.stream_ptr())
        _capi.check(rc, "pxsom_comm_allreduce_sum_f64")

    def close(self) -> None:
        if self.handle is not None:
            h, self.handle = self.handle, None
            _capi.check(_capi.lib().pxsom_comm_destroy(h), "pxsom_comm_destroy")


P2P_HANDLE_BYTES = 64  # include/pxsom.h PXSOM_P2P_HANDLE_BYTES


class P2PComm:
    """One-shot peer-to-peer exchange owned by libpxsom (pxsom_comm_p2p_*): every rank's block of device memory is mapped
    by the others through HIP IPC, an all-reduce is one launch per rank and gives bit-identical sums on all ranks.  Ranks
    may share a device.  Two phases, so that a launcher can agree on each before the next: the constructor allocates the
    own block (``local_handle``: 64 bytes), ``connect`` takes the handles of all ranks in rank order (``gather``: a
    callable doing both in one go, e.g. over ``torch.distributed.all_gather_object``).  Same interface as RankComm."""

    def __init__(self, nranks: int, rank: int, max_count: int, gather=None):
        import ctypes
        box = ctypes.c_void_p()
        _capi.check(_capi.lib().pxsom_comm_p2p_create(int(nranks), int(rank), int(max_count), ctypes.byref(box)),
                    "pxsom_comm_p2p_create")
        self.handle = box
        self.nranks, self.rank, self.max_count = int(nranks), int(rank), int(max_count)
        self.fused = False
        mine = ctypes.create_string_buffer(P2P_HANDLE_BYTES)
        _capi.check(_capi.lib().pxsom_comm_p2p_handle(self.handle, ctypes.cast(mine, ctypes.c_void_p), P2P_HANDLE_BYTES),
                    "pxsom_comm_p2p_handle")
        self.local_handle = mine.raw          # 64 bytes: what the other ranks need to map this rank's block
        if gather is not None:
            self.connect(gather(self.local_handle))

    def connect(self, handles) -> None:
        """Maps the blocks of all ranks (``handles``: every rank's ``local_handle``, rank order)."""
        import ctypes
        handles = list(handles)
        if len(handles) != self.nranks or any(len(h) != P2P_HANDLE_BYTES for h in handles):
            raise ValueError("one %d-byte handle per rank, in rank order" % P2P_HANDLE_BYTES)
        blob = ctypes.create_string_buffer(b"".join(handles), P2P_HANDLE_BYTES * self.nranks)
        _capi.check(_capi.lib().pxsom_comm_p2p_connect(self.handle, ctypes.cast(blob, ctypes.c_void_p),
                                                       P2P_HANDLE_BYTES * self.nranks), "pxsom_comm_p2p_connect")

    def allreduce_sum(self, t: torch.Tensor) -> None:
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("the exchange reduces contiguous float64 buffers")
        rc = _capi.lib().pxsom_comm_allreduce_sum_f64(self.handle, t.data_ptr(), t.numel(), _capi.stream_ptr())
        _capi.check(rc, "pxsom_comm_allreduce_sum_f64")

    def set_fused(self, on: bool) -> None:
        """The fused 10 x 10 training step runs the exchange inside its own launch (every rank: the same value)."""
        _capi.check(_capi.lib().pxsom_comm_p2p_set_fused(self.handle, 1 if on else 0), "pxsom_comm_p2p_set_fused")
        self.fused = bool(on)

    def error_epoch(self) -> int:
        """0, or the number of the first exchange a peer did not arrive at in time (its result was NaN)."""
        import ctypes
        out = ctypes.c_uint64(0)
        _capi.check(_capi.lib().pxsom_comm_p2p_error(self.handle, ctypes.byref(out)), "pxsom_comm_p2p_error")
        return int(out.value)

    def close(self) -> None:
        if self.handle is not None:
            h, self.handle = self.handle, None
            _capi.check(_capi.lib().pxsom_comm_destroy(h), "pxsom_comm_destroy")


def batch_train_finish(state: BatchTrainState, steps_done: int, total_steps: int, alpha_range, radius_range,
                       w_out: torch.Tensor) -> None:
    """Applies the last pending update of a run: ``w_out`` [K, C] receives the codebook after ``steps_done`` steps."""
    w_out = _codebook(w_out)
    sch = state.schedule
    rc = _capi.lib().pxsom_batch_train_sched_finish(
        state.wbuf.data_ptr(), state.ring.data_ptr(), state.xdim, state.ydim, state.c, sch.phases,
        state.edges.ctypes.data, sch.steps, int(steps_done), int(total_steps) // sch.steps, float(alpha_range[0]),
        float(alpha_range[1]), float(radius_range[0]), float(radius_range[1]), w_out.data_ptr(), _capi.stream_ptr())
    _capi.check(rc, "pxsom_batch_train_sched_finish")


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
    rc = _capi.lib().pxsom_batch_accumulate(x.data_ptr(), n, c, ldx, dt, w.data_ptr(), k,
                                            labels.data_ptr(), stats.data_ptr(),
                                            workspace.buf.data_ptr(), workspace.bytes,
                                            ACC_PREPARED if prepared else 0, _capi.stream_ptr())
    _capi.check(rc, "pxsom_batch_accumulate")


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
    rc = _capi.lib().pxsom_batch_update_prepare(w.data_ptr(), int(xdim), int(ydim), c, stats.data_ptr(),
                                                stats_next.data_ptr() if stats_next is not None else None,
                                                float(thr), float(alpha),
                                                workspace.buf.data_ptr() if workspace is not None else None,
                                                workspace.bytes if workspace is not None else 0,
                                                _capi.stream_ptr())
    _capi.check(rc, "pxsom_batch_update_prepare")


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
        rc = _capi.lib().pxsom_train_online_metric(x.data_ptr(), n, c, ldx, dt, w.data_ptr(), int(xdim), int(ydim), int(rlen),
                                                   float(alpha_range[0]), float(alpha_range[1]), float(radius_range[0]),
                                                   float(radius_range[1]), order.data_ptr(), metric,
                                                   ONLINE_INT_ABS if int_abs else 0, _capi.stream_ptr())
        _capi.check(rc, "pxsom_train_online_metric")
        return w
    rc = _capi.lib().pxsom_train_online_ex(x.data_ptr(), n, c, ldx, dt, w.data_ptr(), int(xdim),
                                           int(ydim), int(rlen), float(alpha_range[0]),
                                           float(alpha_range[1]), float(radius_range[0]),
                                           float(radius_range[1]), order.data_ptr(),
                                           ONLINE_INT_ABS if int_abs else 0, _capi.stream_ptr())
    _capi.check(rc, "pxsom_train_online")
    return w


def batch_update(w: torch.Tensor, xdim: int, ydim: int, sums: torch.Tensor, counts: torch.Tensor,
                 thr: float, alpha: float) -> torch.Tensor:
    w = _codebook(w)
    c = w.shape[1]
    if sums.dtype != torch.float64 or counts.dtype != torch.float64:
        raise ValueError("sums and counts must be float64 (counts are exact integers)")
    rc = _capi.lib().pxsom_batch_update(w.data_ptr(), int(xdim), int(ydim), c, sums.data_ptr(),
                                        counts.data_ptr(), float(thr), float(alpha),
                                        _capi.stream_ptr())
    _capi.check(rc, "pxsom_batch_update")
    return w


def gaussian_kernel1d(sigma: float, truncate: float = 4.0):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius): host numpy, as scipy builds it."""
    radius = int(truncate * float(sigma) + 0.5)
    sigma2 = sigma * sigma
    xs = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * xs ** 2)
    phi_x = phi_x / phi_x.sum()
    return np.ascontiguousarray(phi_x[::-1], dtype=np.float64), radius


def gaussian_blur_hwc(img: torch.Tensor, sigma: float, tmp: Optional[torch.Tensor] = None,
                      f32_semantics: bool = False, generic_form: bool = False) -> torch.Tensor:
    """In-place per-channel Gaussian blur of an [H, W, C] float64 HBM image (scipy semantics).
    ``f32_semantics``: the values are widened float32 and every pass is stored as float32, as scipy does
    for a float32 image."""
    if img.dtype != torch.float64 or not img.is_cuda or not img.is_contiguous() or img.dim() != 3:
        raise ValueError("image must be a contiguous float64 [H, W, C] HBM tensor")
    h, w, c = img.shape
    if tmp is None:
        tmp = torch.empty_like(img)
    weights, radius = gaussian_kernel1d(sigma)
    rc = _capi.lib().pxsom_gaussian_blur_hwc(img.data_ptr(), tmp.data_ptr(), h, w, c,
                                             weights.ctypes.data, radius,
                                             int(bool(f32_semantics)) | (2 if generic_form else 0), _capi.stream_ptr())
    _capi.check(rc, "pxsom_gaussian_blur_hwc")
    return img


def rowsum_filter_normalize(x: torch.Tensor, thresh: float, f32_semantics: bool = False):
    """(rows [m, C] f64 = x_i / rowsum_i for kept pixels, flat pixel index [m] i64), compacted in order.
    ``f32_semantics``: widened float32 values, row sum and division in binary32 (a float32 pandas frame)."""
    if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
        raise ValueError("matrix must be a contiguous float64 [N, C] HBM tensor")
    n, c = x.shape
    out = torch.empty_like(x)
    idx = torch.empty(n, dtype=torch.int64, device=x.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=x.device)
    wsb = _capi.lib().pxsom_rownorm_workspace_bytes(n)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=x.device)
    rc = _capi.lib().pxsom_rowsum_filter_normalize(x.data_ptr(), n, c, float(thresh), out.data_ptr(),
                                                   idx.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb,
                                                   int(bool(f32_semantics)), _capi.stream_ptr())
    _capi.check(rc, "pxsom_rowsum_filter_normalize")
    m = int(cnt.item())
    return out[:m], idx[:m]


def normalize_columns(x: torch.Tensor, norm: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if x.dtype != torch.float64 or norm.dtype != torch.float64:
        raise ValueError("normalize_columns works in float64 like the reference")
    n, c = x.shape
    if out is None:
        out = torch.empty((n, c), dtype=torch.float64, device=x.device)
    rc = _capi.lib().pxsom_normalize_columns(x.data_ptr(), n, c, x.stride(0) if n > 1 else c, norm.data_ptr(),
                                             out.data_ptr(), out.stride(0) if n > 1 else c, _capi.stream_ptr())
    _capi.check(rc, "pxsom_normalize_columns")
    return out


def quantile_nonzero(x: torch.Tensor, q: float, keep_mode: int = 0) -> torch.Tensor:
    """Exact type-7 quantile of the kept (non-zero / positive) values of every column -> [C] f64."""
    if x.dtype != torch.float64 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("matrix must be a float64 [N, C] HBM tensor with contiguous rows")
    n, c = x.shape
    out = torch.empty(c, dtype=torch.float64, device=x.device)
    wsb = _capi.lib().pxsom_quantile_workspace_bytes(n, c)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    rc = _capi.lib().pxsom_quantile_nonzero(x.data_ptr(), n, c, x.stride(0) if n > 1 else c, float(q),
                                            int(keep_mode), out.data_ptr(), ws.data_ptr(), wsb,
                                            _capi.stream_ptr())
    _capi.check(rc, "pxsom_quantile_nonzero")
    return out


def to_numpy(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


def pair_histogram(a: torch.Tensor, b: torch.Tensor, na: int, nb: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[a_i, b_i] += 1`` over two int32 HBM vectors (pairs outside [0, na) x [0, nb) are ignored);
    ``out`` [na, nb] int64 (zeros if not given)."""
    if a.dtype != torch.int32 or b.dtype != torch.int32 or a.numel() != b.numel() or not a.is_cuda:
        raise ValueError("a and b must be int32 HBM vectors of the same length")
    a, b = a.contiguous(), b.contiguous()
    if out is None:
        out = torch.zeros((int(na), int(nb)), dtype=torch.int64, device=a.device)
    rc = _capi.lib().pxsom_pair_histogram(a.data_ptr(), b.data_ptr(), a.numel(), int(na), int(nb),
                                          out.data_ptr(), _capi.stream_ptr())
    _capi.check(rc, "pxsom_pair_histogram")
    return out


def quantile_f32(x: torch.Tensor, q: float, keep_mode: int = 1) -> torch.Tensor:
    """``np.quantile`` of the kept values of every float32 column, in numpy's float32 arithmetic
    (keep_mode 1: > 0, 2: every non-NaN value) -> [C] float32."""
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("matrix must be a float32 [N, C] HBM tensor with contiguous rows")
    n, c = x.shape
    out = torch.empty(c, dtype=torch.float64, device=x.device)
    wsb = _capi.lib().pxsom_quantile_workspace_bytes(n, c)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    rc = _capi.lib().pxsom_quantile_f32(x.data_ptr(), n, c, x.stride(0) if n > 1 else c, float(q), int(keep_mode),
                                        out.data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr())
    _capi.check(rc, "pxsom_quantile_f32")
    return out.to(torch.float32)


def scaled_rowsum(img: torch.Tensor, norm: torch.Tensor) -> torch.Tensor:
    """``np.sum(img / norm, axis=-1)`` for [N, C] pixels and [C] divisors of one floating type (float32: numpy's
    binary32 arithmetic; float64: what numpy computes for every other image dtype), in numpy's summation
    order -> [N] of that type."""
    if img.dtype not in (torch.float32, torch.float64) or norm.dtype != img.dtype or not img.is_cuda \
            or img.dim() != 2 or img.stride(1) != 1:
        raise ValueError("img must be a float32 / float64 [N, C] HBM tensor with contiguous rows, norm [C] of the same type")
    n, c = img.shape
    out = torch.empty(n, dtype=img.dtype, device=img.device)
    fn = _capi.lib().pxsom_scaled_rowsum_f32 if img.dtype == torch.float32 else _capi.lib().pxsom_scaled_rowsum_f64
    rc = fn(img.data_ptr(), n, c, img.stride(0) if n > 1 else c, norm.contiguous().data_ptr(), out.data_ptr(),
            _capi.stream_ptr())
    _capi.check(rc, "pxsom_scaled_rowsum")
    return out


def scaled_rowsum_f32(img: torch.Tensor, norm: torch.Tensor) -> torch.Tensor:
    if img.dtype != torch.float32 or norm.dtype != torch.float32:
        raise ValueError("img must be a float32 [N, C] HBM tensor with contiguous rows, norm float32 [C]")
    return scaled_rowsum(img, norm)


MASK_BAD_LABEL, MASK_BAD_PIXEL = 1, 2   # include/pxsom.h PXSOM_MASK_*
LUT_UNMAPPED = -2 ** 31                 # PXSOM_LUT_UNMAPPED


def cluster_mask(row_index: torch.Tensor, column_index: torch.Tensor, labels: torch.Tensor, lut: torch.Tensor,
                 h: int, w: int):
    """``mask.ravel()[row_index * w + column_index] = lut[labels]`` on an int16 ``[h, w]`` image of zeros
    (last row wins for a pixel listed twice).  int64 HBM vectors, int32 LUT.  Returns ``(mask, status)``:
    status 0, or MASK_BAD_LABEL / MASK_BAD_PIXEL bits (synchronises to read it)."""
    for name, t in (("row_index", row_index), ("column_index", column_index), ("labels", labels)):
        if t.dtype != torch.int64 or not t.is_cuda or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 HBM vector")
    if not (row_index.numel() == column_index.numel() == labels.numel()):
        raise ValueError("row_index, column_index and labels must have one entry per table row")
    if lut.dtype != torch.int32 or not lut.is_cuda or not lut.is_contiguous():
        raise ValueError("lut must be a contiguous int32 HBM vector")
    dev = labels.device
    mask = torch.empty((int(h), int(w)), dtype=torch.int16, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = _capi.lib().pxsom_cluster_mask_workspace_bytes(int(h), int(w))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    rc = _capi.lib().pxsom_cluster_mask(row_index.data_ptr(), column_index.data_ptr(), labels.data_ptr(),
                                        labels.numel(), lut.data_ptr(), lut.numel(), int(h), int(w),
                                        mask.data_ptr(), status.data_ptr(), ws.data_ptr(), wsb, _capi.stream_ptr())
    _capi.check(rc, "pxsom_cluster_mask")
    return mask, int(status.item())


def relabel(labels: torch.Tensor, lut: torch.Tensor, fill: int = -1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[i] = lut[labels[i]]`` (``fill`` for labels outside the table): SOM cluster -> meta cluster for labels
    that live in HBM.  int32 vectors; ``out`` may be ``labels``."""
    if labels.dtype != torch.int32 or lut.dtype != torch.int32 or not labels.is_cuda or not labels.is_contiguous():
        raise ValueError("labels and lut must be contiguous int32 HBM vectors")
    if out is None:
        out = torch.empty_like(labels)
    rc = _capi.lib().pxsom_relabel(labels.data_ptr(), labels.numel(), lut.contiguous().data_ptr(), lut.numel(), int(fill),
                                   out.data_ptr(), _capi.stream_ptr())
    _capi.check(rc, "pxsom_relabel")
    return out


# include/pxsom.h PXSOM_SEG_*: the label dtypes of a segmentation image, and float64 (an output only)
SEG_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.uint16: 2, torch.int32: 3, torch.uint32: 4, torch.int64: 5}
SEG_F64 = 6
SEG_ERODE = {None: 0, "thick": 1, "inner": 2}
SEGMASK_FORCE_SEARCH = 1


def segmask_table(keys, values, device, float_values: bool = False):
    """Host (key -> value) arrays as the device table of :func:`segmentation_mask`: ``keys`` int32, sorted ascending and
    unique (checked here: the library relies on it), ``values`` int32, or float64 with ``float_values``."""
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float64 if float_values else np.int32)
    if keys.ndim != 1 or values.shape != keys.shape:
        raise ValueError("keys and values must be vectors of one length")
    if keys.size > 1 and not np.all(keys[1:] > keys[:-1]):
        raise ValueError("keys must be sorted ascending without duplicates")
    return (torch.from_numpy(keys).to(device), torch.from_numpy(values).to(device),
            int(keys[0]) if keys.size else 0, int(keys[-1]) if keys.size else 0)


def segmentation_mask(seg: torch.Tensor, erode: Optional[str] = None, connectivity: int = 1, background: int = 0,
                      table=None, unassigned=0, out_dtype: Optional[torch.dtype] = None, force_search: bool = False,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One pass of pxsom_segmask over a ``[H, W]`` label image in HBM (rows contiguous, any row stride): optional border
    erosion (``erode`` "thick" / "inner": skimage's find_boundaries with ``connectivity`` and ``background``; boundary
    pixels become 0), then the optional lookup ``table`` of :func:`segmask_table` (label cast to int32, ``unassigned``
    where the table has no entry), stored as ``out_dtype`` (int16, int32, float64 or the image's dtype; default: the
    image's).  ``force_search`` takes the binary-search route even where a dense LUT would fit."""
    if seg.dim() != 2 or not seg.is_cuda or seg.dtype not in SEG_DTYPES:
        raise ValueError("seg must be a 2-D uint8 / int16 / uint16 / int32 / uint32 / int64 HBM tensor")
    h, w = seg.shape
    if h == 0 or w == 0:
        raise ValueError("seg must not be empty")
    if w > 1 and seg.stride(1) != 1:
        raise ValueError("seg rows must be contiguous (stride(1) == 1)")
    if erode not in SEG_ERODE:
        raise NotImplementedError(f"erosion mode {erode!r}: only 'thick' and 'inner' are implemented")
    connectivity = max(int(connectivity), 1)        # scipy's generate_binary_structure treats < 1 as 1
    if out_dtype is None:
        out_dtype = seg.dtype
    if out_dtype != seg.dtype and out_dtype not in (torch.int16, torch.int32, torch.float64):
        raise ValueError("out_dtype must be int16, int32, float64 or the image's dtype")
    code_out = SEG_F64 if out_dtype == torch.float64 else SEG_DTYPES[out_dtype]
    out = _rows_plane(out, h, w, out_dtype, seg.device, "out")
    ld, ldo = _ld(seg), _ld(out)
    lib = _capi.lib()
    if table is None:
        keys = values = None
        n_keys, kmin, kmax = -1, 0, 0
    else:
        keys, values, kmin, kmax = table
        n_keys = keys.numel()
        if values.dtype != (torch.float64 if out_dtype == torch.float64 else torch.int32):
            raise ValueError("table values must be float64 for a float64 output, int32 otherwise")
    wsb = 0 if force_search or n_keys <= 0 else lib.pxsom_segmask_workspace_bytes(n_keys, kmin, kmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device=seg.device) if wsb else None
    rc = lib.pxsom_segmask(seg.data_ptr(), SEG_DTYPES[seg.dtype], h, w, ld, SEG_ERODE[erode], connectivity, int(background),
                           keys.data_ptr() if keys is not None else None, values.data_ptr() if values is not None else None,
                           n_keys, kmin, kmax, float(unassigned), out.data_ptr(), code_out, ldo,
                           ws.data_ptr() if ws is not None else None, wsb,
                           SEGMASK_FORCE_SEARCH if force_search else 0, _capi.stream_ptr())
    _capi.check(rc, "pxsom_segmask")
    return out


# pxsom_gaussian_blur_plane / pxsom_zero_by_seg: the plane dtypes (PXSOM_SEG_* codes, float32 = PXSOM_SEG_F32)
PLANE_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.uint16: 2, torch.int32: 3, torch.float32: 7}
BLUR_MAX_RADIUS = 64                     # kMaxRadius of csrc/pxsom_pre.hip
BLUR_SIGMA_LIMIT = 16.125                # int(4 sigma + 0.5) <= 64  <=>  sigma < 16.125


def check_blur_sigma(sigma: float) -> None:
    """NotImplementedError for a sigma whose radius the device blur does not take (sigma >= 16.125)."""
    if float(sigma) > 1e-15 and int(4.0 * float(sigma) + 0.5) > BLUR_MAX_RADIUS:
        raise NotImplementedError("gaussian blur on the device: sigma %r is beyond the radius limit "
                                  "(sigma < %g, radius <= %d)" % (sigma, BLUR_SIGMA_LIMIT, BLUR_MAX_RADIUS))


BLUR_MODES = {"reflect": 0, "nearest": 1}          # include/pxsom.h PXSOM_BLUR_REFLECT / PXSOM_BLUR_NEAREST
PLANE_MODE_DTYPES = {**PLANE_DTYPES, torch.float64: 6}


def _blur_plane(plane: torch.Tensor, sigma: float, mode: str, out, tmp, mode_entry: bool) -> torch.Tensor:
    """The body of both plane blurs; ``mode_entry``: through pxsom_gaussian_blur_plane_mode."""
    if mode not in BLUR_MODES:
        raise ValueError("mode must be 'reflect' or 'nearest', got %r" % (mode,))
    if plane.dim() != 2 or not plane.is_cuda or not plane.is_contiguous() or plane.dtype not in PLANE_MODE_DTYPES:
        raise ValueError("plane must be a contiguous 2-D uint8 / int16 / uint16 / int32 / float32 / float64 HBM tensor")
    h, w = plane.shape
    if h == 0 or w == 0:
        raise ValueError("plane must not be empty")
    check_blur_sigma(sigma)
    out = _like_plane(out, plane, "out")
    if float(sigma) <= 1e-15:
        if out.data_ptr() != plane.data_ptr():
            out.copy_(plane)
        return out
    tmp = _like_plane(tmp, plane, "tmp")
    weights, radius = gaussian_kernel1d(float(sigma))
    args = (plane.data_ptr(), out.data_ptr(), tmp.data_ptr(), h, w, PLANE_MODE_DTYPES[plane.dtype], weights.ctypes.data, radius)
    if mode_entry:
        rc = _capi.lib().pxsom_gaussian_blur_plane_mode(*args, BLUR_MODES[mode], _capi.stream_ptr())
        _capi.check(rc, "pxsom_gaussian_blur_plane_mode")
    else:
        rc = _capi.lib().pxsom_gaussian_blur_plane(*args, _capi.stream_ptr())
        _capi.check(rc, "pxsom_gaussian_blur_plane")
    return out


def gaussian_blur_plane(plane: torch.Tensor, sigma: float, out: Optional[torch.Tensor] = None,
                        tmp: Optional[torch.Tensor] = None, mode: str = "reflect") -> torch.Tensor:
    """scipy.ndimage.gaussian_filter(plane, sigma, mode=mode) of a contiguous ``[H, W]`` HBM plane in its own dtype (uint8,
    int16, uint16, int32, float32 or float64): each pass stored in that dtype, as scipy stores it.  sigma <= 1e-15 skips
    both axes (scipy's rule): the result is a copy.  ``out`` may be ``plane`` itself.  ``mode``: scipy's border, "reflect"
    (the default) or "nearest".  The default mode on the five dtypes up to float32 is pxsom_gaussian_blur_plane, route and
    bits as before the keyword existed; "nearest", and float64 planes (which this function used to refuse) under either
    mode, go to pxsom_gaussian_blur_plane_mode."""
    return _blur_plane(plane, sigma, mode, out, tmp, mode != "reflect" or plane.dtype == torch.float64)


def gaussian_blur_plane_mode(plane: torch.Tensor, sigma: float, mode: str, out: Optional[torch.Tensor] = None,
                             tmp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scipy.ndimage.gaussian_filter(plane, sigma, mode=mode) through pxsom_gaussian_blur_plane_mode: the plane blur of
    :func:`gaussian_blur_plane` with the border "reflect" or "nearest" and float64 planes beside the others."""
    return _blur_plane(plane, sigma, mode, out, tmp, True)


# ---- object masks (K16): labelling, the area passes, the foreground predicates ----------------------------------------
SELECT_FILL, SELECT_KEEP = 0, 1                      # include/pxsom.h PXSOM_SELECT_*
BIN_POSITIVE, BIN_LEVEL, BIN_LOCAL = 0, 1, 2         # PXSOM_BIN_*
CCL_TILE = 64                                        # kTile of csrc/pxsom_ccl.hip


def _binary_plane(fg: torch.Tensor, what: str) -> torch.Tensor:
    if fg.dim() != 2 or not fg.is_cuda or fg.dtype not in (torch.uint8, torch.bool):
        raise ValueError("%s must be a 2-D uint8 or bool HBM tensor" % what)
    if fg.shape[0] == 0 or fg.shape[1] == 0:
        raise ValueError("%s must not be empty" % what)
    if fg.shape[1] > 1 and fg.stride(1) != 1:
        raise ValueError("%s rows must be contiguous (stride(1) == 1)" % what)
    return fg.view(torch.uint8) if fg.dtype == torch.bool else fg


def _rows_plane(t: Optional[torch.Tensor], h: int, w: int, dtype, device, what: str) -> torch.Tensor:
    """``t``, checked to be a ``[h, w]`` HBM plane of ``dtype`` with contiguous rows (any row stride), or a new one."""
    if t is None:
        return torch.empty((h, w), dtype=dtype, device=device)
    if t.shape != (h, w) or t.dtype != dtype or not t.is_cuda or (w > 1 and t.stride(1) != 1):
        raise ValueError("%s must be a [H, W] %s HBM tensor with contiguous rows" % (what, str(dtype).replace("torch.", "")))
    return t


def _label_plane(t: Optional[torch.Tensor], h: int, w: int, device, what: str) -> torch.Tensor:
    return _rows_plane(t, h, w, torch.int32, device, what)


def _like_plane(t: Optional[torch.Tensor], plane: torch.Tensor, what: str) -> torch.Tensor:
    """``t``, checked to be a contiguous HBM tensor of the plane's shape and dtype, or a new one."""
    if t is None:
        return torch.empty_like(plane)
    if t.shape != plane.shape or t.dtype != plane.dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError("%s must be a contiguous HBM tensor of the plane's shape and dtype" % what)
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def label_components(fg: torch.Tensor, connectivity: int, invert: bool = False, out: Optional[torch.Tensor] = None,
                     capacity: Optional[int] = None):
    """``skimage.measure.label(fg != 0, connectivity=connectivity)`` of a ``[H, W]`` uint8 / bool HBM plane (rows
    contiguous, any row stride); with ``invert`` the pixels equal to 0 are the foreground.  Returns ``(labels, n, areas)``,
    all in HBM: ``labels`` int32 ``[H, W]`` (``out`` if given: rows contiguous, any row stride), background 0, components
    numbered by their first pixel in raster order; ``n`` int32 ``[1]``, the count; ``areas`` int32 ``[capacity]`` with
    ``areas[0]`` the background pixels (default capacity: every image's worst case, ``(H W + 1) // 2 + 1``)."""
    fg = _binary_plane(fg, "fg")
    h, w = fg.shape
    if connectivity not in (1, 2):
        raise ValueError("connectivity must be 1 or 2, got %r" % (connectivity,))
    labels = _label_plane(out, h, w, fg.device, "out")
    capacity = (h * w + 1) // 2 + 1 if capacity is None else int(capacity)
    n = torch.empty(1, dtype=torch.int32, device=fg.device)
    areas = torch.empty(capacity, dtype=torch.int32, device=fg.device)
    lib = _capi.lib()
    wsb = lib.pxsom_label_components_workspace_bytes(h, w)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=fg.device)
    rc = lib.pxsom_label_components(fg.data_ptr(), h, w, _ld(fg), int(connectivity), int(bool(invert)), labels.data_ptr(),
                                    _ld(labels), n.data_ptr(), areas.data_ptr(), capacity, ws.data_ptr(), wsb,
                                    _capi.stream_ptr())
    _capi.check(rc, "pxsom_label_components")
    return labels, n, areas


def components_select(labels: torch.Tensor, areas: torch.Tensor, mode: str, fg: Optional[torch.Tensor] = None,
                      area_threshold: Optional[int] = None, min_area: int = 0, max_area: Optional[int] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One pass over a label image and its area table (:func:`label_components`).
    ``mode="fill"``: ``fg | (labels != 0 & areas[labels] < area_threshold)`` as uint8, ``labels`` being those of the
    inverted ``fg`` under connectivity 1 -- ``morphology.remove_small_holes(fg, area_threshold)``.
    ``mode="keep"``: ``labels`` where ``min_area <= areas[labels] <= max_area``, else 0 (int32; not renumbered);
    ``out`` may be ``labels``."""
    if mode not in ("fill", "keep"):
        raise ValueError("mode must be 'fill' or 'keep', got %r" % (mode,))
    if labels.dim() != 2 or labels.shape[0] == 0 or labels.shape[1] == 0:
        raise ValueError("labels must be a non-empty [H, W] tensor")
    h, w = labels.shape
    labels = _label_plane(labels, h, w, labels.device, "labels")
    if areas.dtype != torch.int32 or not areas.is_cuda or areas.dim() != 1 or not areas.is_contiguous() or not areas.numel():
        raise ValueError("areas must be a contiguous int32 HBM vector")
    lim = 2 ** 62
    if mode == "fill":
        if fg is None or area_threshold is None:
            raise ValueError("mode 'fill' needs fg and area_threshold")
        fg = _binary_plane(fg, "fg")
        if fg.shape != (h, w):
            raise ValueError("fg and labels must have one shape")
        out = _rows_plane(out, h, w, torch.uint8, labels.device, "out")
        args = (SELECT_FILL, fg.data_ptr(), _ld(fg), 0, max(-lim, min(lim, int(area_threshold))))
    else:
        out = _label_plane(out, h, w, labels.device, "out")
        hi = lim if max_area is None else max(-lim, min(lim, int(np.floor(max_area))))
        args = (SELECT_KEEP, None, 0, max(-lim, min(lim, int(np.ceil(min_area)))), hi)
    rc = _capi.lib().pxsom_components_select(args[0], args[1], args[2], labels.data_ptr(), _ld(labels), areas.data_ptr(),
                                             areas.numel(), h, w, args[3], args[4], out.data_ptr(), _ld(out),
                                             _capi.stream_ptr())
    _capi.check(rc, "pxsom_components_select")
    return out


def binarize_plane(plane: torch.Tensor, mode: int = BIN_POSITIVE, level: float = 0.0,
                   local: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The uint8 foreground of a contiguous float32 / float64 ``[H, W]`` HBM plane: ``v > 0`` (BIN_POSITIVE),
    ``!(v < level) & v > 0`` (BIN_LEVEL) or ``v > local`` (BIN_LOCAL, ``local`` a plane of the same dtype and shape)."""
    if plane.dim() != 2 or not plane.is_cuda or not plane.is_contiguous() or plane.dtype not in (torch.float32, torch.float64):
        raise ValueError("plane must be a contiguous 2-D float32 / float64 HBM tensor")
    if plane.numel() == 0:
        raise ValueError("plane must not be empty")
    if mode == BIN_LOCAL:
        if local is None:
            raise ValueError("BIN_LOCAL needs the local plane")
        local = _like_plane(local, plane, "local")
    h, w = plane.shape
    out = torch.empty((h, w), dtype=torch.uint8, device=plane.device)
    rc = _capi.lib().pxsom_binarize_plane(plane.data_ptr(), PLANE_MODE_DTYPES[plane.dtype], h, w, int(mode), float(level),
                                          local.data_ptr() if mode == BIN_LOCAL else None, out.data_ptr(), w,
                                          _capi.stream_ptr())
    _capi.check(rc, "pxsom_binarize_plane")
    return out


RIDGE_MAX_RADIUS, RIDGE_MAX_SCALES = 16, 8           # kRidgeMaxRadius / kRidgeMaxScales of csrc/pxsom_ridge.hip


def ridge_sign(fg: torch.Tensor, sigmas=(1, 2, 3, 4), alpha=0.5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``skimage.filters.meijering(fg != 0, sigmas, alpha, black_ridges=False) > 0`` in skimage 0.19's statement
    (include/pxsom.h "K22"; parity with skimage itself is unpinned) of a ``[H, W]`` uint8 / bool HBM plane (rows contiguous,
    any row stride) -> uint8 ``[H, W]`` of 1 / 0 in HBM (``out`` if given: rows contiguous, any row stride, not ``fg``).
    One launch of pxsom_ridge_sign.  ``H`` and ``W`` are at least 2, as np.gradient demands; up to 8 scales, each with
    ``int(4 sigma + 0.5)`` between 1 and 16."""
    fg = _binary_plane(fg, "fg")
    h, w = fg.shape
    if h < 2 or w < 2:
        raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements "
                         "are required.")
    sigmas = list(sigmas)
    if not 1 <= len(sigmas) <= RIDGE_MAX_SCALES:
        raise ValueError("ridge_sign takes 1 to %d scales, got %d" % (RIDGE_MAX_SCALES, len(sigmas)))
    if not all(float(s) > 0 and np.isfinite(float(s)) for s in sigmas) or not np.isfinite(float(alpha)):
        raise ValueError("ridge_sign takes finite sigmas > 0 and a finite alpha, got %r and %r" % (sigmas, alpha))
    kernels = [gaussian_kernel1d(float(s)) for s in sigmas]
    for s, (_, radius) in zip(sigmas, kernels):
        if not 1 <= radius <= RIDGE_MAX_RADIUS:
            raise NotImplementedError("ridge_sign: sigma %r has radius %d outside [1, %d]" % (s, radius, RIDGE_MAX_RADIUS))
    weights = np.ascontiguousarray(np.concatenate([k for k, _ in kernels]), dtype=np.float64)
    radii = np.array([r for _, r in kernels], dtype=np.int32)
    scales = np.array([float(s ** 2) for s in sigmas], dtype=np.float64)
    out = _rows_plane(out, h, w, torch.uint8, fg.device, "out")
    rc = _capi.lib().pxsom_ridge_sign(fg.data_ptr(), h, w, _ld(fg), weights.ctypes.data, radii.ctypes.data, scales.ctypes.data,
                                      len(sigmas), float(alpha), out.data_ptr(), _ld(out), _capi.stream_ptr())
    _capi.check(rc, "pxsom_ridge_sign")
    return out


def object_mask(img: torch.Tensor, sigma, thresh, hole_size, min_area, max_area, local_block=None, ridge=None) -> torch.Tensor:
    """The device chain of ``_create_object_mask`` on a ``[H, W]`` HBM image -> int32 ``[H, W]`` labels in HBM.
    float32 / float64 images go as they are, any other dtype is cast to float64 (skimage's ``preserve_range`` rule).
      blur       ``sigma`` None: none; else ``gaussian_filter(x, sigma, mode='nearest')`` in x's dtype
      threshold  ``thresh`` None: ``blur > 0``; an int: ``p = np.percentile(blur[blur != 0], thresh)``, foreground
                 ``!(blur < p) & blur > 0``; "auto": ``blur > gaussian_filter(blur, (local_block - 1) / 6, mode='reflect')``
      holes      ``hole_size`` None: none; else background components (4-neighbourhood) of area < hole_size are filled
      ridge      ``ridge`` None: none; a ``(sigmas, alpha)`` tuple: the foreground becomes :func:`ridge_sign` of it
                 ("projection" objects)
      labels     8-neighbourhood components, kept where ``min_area <= area <= max_area`` (not renumbered)
    The percentile is the one value read back to the host: pxsom_quantile_f32 / pxsom_quantile_nonzero with their
    ``!= 0`` keep rule (bits equal numpy's for both dtypes; a NaN pixel is dropped there where numpy's result turns NaN)."""
    if img.dim() != 2 or not img.is_cuda or img.shape[0] == 0 or img.shape[1] == 0:
        raise ValueError("img must be a non-empty 2-D HBM tensor")
    x = img if img.dtype in (torch.float32, torch.float64) else img.to(torch.float64)
    x = x.contiguous()
    blur = x if sigma is None else gaussian_blur_plane(x, sigma, mode="nearest")
    if thresh is None:
        fg = binarize_plane(blur, BIN_POSITIVE)
    elif isinstance(thresh, str):
        if thresh != "auto" or local_block is None:
            raise ValueError("thresh 'auto' needs local_block; got thresh=%r local_block=%r" % (thresh, local_block))
        local = gaussian_blur_plane(blur, (float(local_block) - 1) / 6.0, mode="reflect")
        fg = binarize_plane(blur, BIN_LOCAL, local=local)
    else:
        column = blur.reshape(-1, 1)
        q = np.true_divide(thresh, 100)        # np.percentile's own division
        p = (quantile_f32 if blur.dtype == torch.float32 else quantile_nonzero)(column, float(q), keep_mode=0)
        fg = binarize_plane(blur, BIN_LEVEL, level=float(p.item()))
    if hole_size is not None:
        holes, _, hole_areas = label_components(fg, 1, invert=True)
        fg = components_select(holes, hole_areas, "fill", fg=fg, area_threshold=hole_size)
    if ridge is not None:
        fg = ridge_sign(fg, ridge[0], ridge[1])
    labels, _, areas = label_components(fg, 2)
    return components_select(labels, areas, "keep", min_area=min_area, max_area=max_area, out=labels)


# ---- merging object masks into the cell segmentation (K18) --------------------------------------------------------------
PAIR_CAPACITY_MAX = 1 << 27                          # kMaxPairCapacity of csrc/pxsom_merge.hip


def label_regions(seg: torch.Tensor, connectivity: int, out: Optional[torch.Tensor] = None,
                  capacity: Optional[int] = None):
    """``skimage.measure.label(seg, background=0, connectivity=connectivity)`` of a ``[H, W]`` integer HBM label plane
    (uint8 .. int64, rows contiguous, any row stride): regions of equal non-zero value, touching regions of different
    values kept apart.  Returns ``(labels, n, areas)`` with the conventions of :func:`label_components`; the default
    capacity is every image's worst case, ``H W + 1``."""
    h, w, ld = _label_image(seg, "seg")
    if connectivity not in (1, 2):
        raise ValueError("connectivity must be 1 or 2, got %r" % (connectivity,))
    labels = _label_plane(out, h, w, seg.device, "out")
    capacity = h * w + 1 if capacity is None else int(capacity)
    n = torch.empty(1, dtype=torch.int32, device=seg.device)
    areas = torch.empty(max(capacity, 0), dtype=torch.int32, device=seg.device)
    lib = _capi.lib()
    wsb = lib.pxsom_label_regions_workspace_bytes(h, w)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=seg.device)
    rc = lib.pxsom_label_regions(seg.data_ptr(), SEG_DTYPES[seg.dtype], h, w, ld, int(connectivity), labels.data_ptr(),
                                 _ld(labels), n.data_ptr(), areas.data_ptr(), capacity, ws.data_ptr(), wsb,
                                 _capi.stream_ptr())
    _capi.check(rc, "pxsom_label_regions")
    return labels, n, areas


def _label_pair(a: torch.Tensor, b: torch.Tensor):
    for name, t in (("a", a), ("b", b)):
        if t.dim() != 2 or not t.is_cuda or t.dtype != torch.int32 or t.shape[0] == 0 or t.shape[1] == 0 or \
                (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError("%s must be a non-empty [H, W] int32 HBM plane with contiguous rows" % name)
    if a.shape != b.shape:
        raise ValueError("a and b must have one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    return a.shape


def pair_overlaps(a: torch.Tensor, b: torch.Tensor, n_a: Optional[int] = None, n_b: Optional[int] = None) -> torch.Tensor:
    """The label pairs two ``[H, W]`` int32 HBM planes share: ``[P, 3]`` int32 in HBM, one row ``(a, b, pixels)`` per
    pair with ``1 <= a <= n_a``, ``1 <= b <= n_b`` (default: every positive label) and ``pixels > 0``, sorted by
    ``(a, b)``.  Two calls of pxsom_pair_overlaps: the first counts the runs of the image, which is read back and sizes
    the list and the table of the second."""
    h, w = _label_pair(a, b)
    top = 2 ** 31 - 1
    n_a, n_b = (top if v is None else int(v) for v in (n_a, n_b))
    if not (0 <= n_a <= top and 0 <= n_b <= top):
        raise ValueError("n_a and n_b must lie in 0 .. 2147483647")
    lib = _capi.lib()
    n = torch.empty(2, dtype=torch.int32, device=a.device)

    def call(pairs, capacity, ws, wsb):
        rc = lib.pxsom_pair_overlaps(a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), h, w, n_a, n_b, pairs, capacity,
                                     n.data_ptr(), ws, wsb, _capi.stream_ptr())
        _capi.check(rc, "pxsom_pair_overlaps")

    call(None, 0, None, 0)
    runs = int(n[1].item())
    if runs == 0:
        return torch.empty((0, 3), dtype=torch.int32, device=a.device)
    if runs > PAIR_CAPACITY_MAX:
        raise NotImplementedError("pair_overlaps: %d runs of label pairs are beyond the limit %d" % (runs, PAIR_CAPACITY_MAX))
    pairs = torch.empty((runs, 3), dtype=torch.int32, device=a.device)
    wsb = lib.pxsom_pair_overlaps_workspace_bytes(runs)
    ws = torch.empty(wsb, dtype=torch.uint8, device=a.device)
    call(pairs.data_ptr(), runs, ws.data_ptr(), wsb)
    count = int(n[0].item())
    if count < 0:
        raise RuntimeError("pair_overlaps: the planes changed between the two passes")
    return pairs[:count]


def merge_apply(a: torch.Tensor, b: torch.Tensor, winner: torch.Tensor, removed: torch.Tensor,
                merged: Optional[torch.Tensor] = None, remaining: Optional[torch.Tensor] = None):
    """One pass over two ``[H, W]`` int32 HBM planes with two int32 tables indexed by ``b``:
    ``merged = winner[b] != 0 ? winner[b] : a`` and ``remaining = removed[b] ? 0 : b`` (int32 planes, any row stride)."""
    h, w = _label_pair(a, b)
    for name, t in (("winner", winner), ("removed", removed)):
        if t.dtype != torch.int32 or not t.is_cuda or t.dim() != 1 or not t.is_contiguous() or not t.numel():
            raise ValueError("%s must be a contiguous int32 HBM vector" % name)
    if winner.numel() != removed.numel():
        raise ValueError("winner and removed must have one length")
    merged = _label_plane(merged, h, w, a.device, "merged")
    remaining = _label_plane(remaining, h, w, a.device, "remaining")
    rc = _capi.lib().pxsom_merge_apply(a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), h, w, winner.data_ptr(),
                                       removed.data_ptr(), winner.numel(), merged.data_ptr(), _ld(merged),
                                       remaining.data_ptr(), _ld(remaining), _capi.stream_ptr())
    _capi.check(rc, "pxsom_merge_apply")
    return merged, remaining


def _region_tables(labels: torch.Tensor, n: int):
    """count [n] int64, sums [n, 2] int64 (row, column) and bbox [n, 4] int32 (closed) of the labels 1 .. n, on the host."""
    if n == 0:
        return np.zeros(0, np.int64), np.zeros((0, 2), np.int64), np.zeros((0, 4), np.int32)
    h, w, ld = _label_image(labels, "labels")
    dev = labels.device
    keys = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int64, device=dev)
    sums = torch.empty((n, 2), dtype=torch.int64, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    shape = torch.empty((n, 6), dtype=torch.int64, device=dev)
    lib = _capi.lib()
    wsb = lib.pxsom_region_shape_workspace_bytes(n, 1, n, 0)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    rc = lib.pxsom_region_shape(labels.data_ptr(), SEG_DTYPES[labels.dtype], ld, h, w, keys.data_ptr(), n, 1, n,
                                shape.data_ptr(), count.data_ptr(), sums.data_ptr(), bbox.data_ptr(), ws.data_ptr(), wsb, 0,
                                _capi.stream_ptr())
    _capi.check(rc, "pxsom_region_shape")
    return count.cpu().numpy(), sums.cpu().numpy(), bbox.cpu().numpy()


def choose_merges(pairs: np.ndarray, object_bbox: np.ndarray, cell_count: np.ndarray, cell_sums: np.ndarray,
                  overlap_thresh, expansion_factor):
    """The choice of merge_masks_single on the host, in the reference's float64 statements.  ``pairs`` [P, 3] sorted by
    (object, cell); ``object_bbox`` [n_o, 4] closed (row min, row max, column min, column max); ``cell_count`` [n_c] and
    ``cell_sums`` [n_c, 2] of the cells 1 .. n_c.  Returns the int32 tables ``(winner, removed)`` of n_c + 1 entries:
    the largest object that chose the cell (0: none) and whether any did.  A cell without overlap is never chosen, so
    only the cells of the pair list are candidates; they come in ascending label within an object."""
    n_c = len(cell_count)
    winner = np.zeros(n_c + 1, dtype=np.int32)
    removed = np.zeros(n_c + 1, dtype=np.int32)
    if len(pairs) == 0:
        return winner, removed
    cells = pairs[:, 1].astype(np.int64) - 1
    area = cell_count[cells].astype(np.int64)
    centroid = cell_sums[cells].astype(np.float64) / area.astype(np.float64)[:, None]      # one division per axis
    box = object_bbox[pairs[:, 0].astype(np.int64) - 1].astype(np.int64)
    inside = ((centroid[:, 0] >= box[:, 0] - expansion_factor) & (centroid[:, 0] <= box[:, 1] + expansion_factor) &
              (centroid[:, 1] >= box[:, 2] - expansion_factor) & (centroid[:, 1] <= box[:, 3] + expansion_factor))
    overlap = pairs[:, 2].astype(np.int64)
    meets = overlap / area > overlap_thresh / 100
    best_object, best_overlap, best_cell = 0, 0, 0

    def settle():
        if best_cell:
            winner[best_cell] = best_object       # objects ascend: the last to choose a cell keeps it
            removed[best_cell] = 1

    for obj, cell, ov, ok in zip(pairs[:, 0].tolist(), pairs[:, 1].tolist(), overlap.tolist(), (inside & meets).tolist()):
        if obj != best_object:
            settle()
            best_object, best_overlap, best_cell = obj, 0, 0
        if ok and ov > best_overlap:
            best_overlap, best_cell = ov, cell
    settle()
    return winner, removed


def merge_masks(object_mask: torch.Tensor, cell_mask: torch.Tensor, overlap_thresh, expansion_factor):
    """The device chain of ``merge_masks_single`` on two ``[H, W]`` integer HBM masks of one shape -> ``(merged,
    remaining)`` int32 planes in HBM.  Both masks are relabelled (:func:`label_regions`, 8-neighbourhood); every object,
    in ascending order, takes the cell with the largest overlap among the cells whose centroid lies in the object's
    closed bounding box grown by ``expansion_factor`` and whose ``overlap / area > overlap_thresh / 100`` (both compares
    strict, the smaller label on a tie).  ``merged`` is the object labels with every chosen cell painted in its object's
    label (the largest, when several chose it); ``remaining`` the relabelled cells without the chosen ones.  One small
    read-back -- the pair list and the region tables -- serves the choice (:func:`choose_merges`)."""
    if object_mask.shape != cell_mask.shape:
        raise ValueError("Both masks must have the same shape")
    objects, n_o, _ = label_regions(object_mask, 2)
    cells, n_c, cell_areas = label_regions(cell_mask, 2)
    n_o, n_c = int(n_o.item()), int(n_c.item())
    pairs = pair_overlaps(objects, cells, n_o, n_c).cpu().numpy() if n_o and n_c else np.zeros((0, 3), np.int32)
    if len(pairs):
        _, _, object_bbox = _region_tables(objects, n_o)
        _, cell_sums, _ = _region_tables(cells, n_c)
        cell_count = cell_areas[1:n_c + 1].cpu().numpy()
    else:
        object_bbox, cell_sums, cell_count = np.zeros((n_o, 4), np.int32), np.zeros((n_c, 2), np.int64), np.ones(n_c, np.int64)
    winner, removed = choose_merges(pairs, object_bbox, cell_count, cell_sums, overlap_thresh, expansion_factor)
    dev = objects.device
    return merge_apply(objects, cells, torch.from_numpy(winner).to(dev), torch.from_numpy(removed).to(dev))


def zero_by_segmentation(img: torch.Tensor, seg: torch.Tensor, exclude: bool = True) -> torch.Tensor:
    """In place: ``img[seg > 0] = 0`` (``exclude``) or ``img[seg == 0] = 0`` for a contiguous HBM image (uint8, int16,
    uint16, int32 or float32) and a contiguous segmentation of the same shape (uint8 .. int64)."""
    if not img.is_cuda or not img.is_contiguous() or img.dtype not in PLANE_DTYPES:
        raise ValueError("img must be a contiguous uint8 / int16 / uint16 / int32 / float32 HBM tensor")
    if not seg.is_cuda or not seg.is_contiguous() or seg.dtype not in SEG_DTYPES:
        raise ValueError("seg must be a contiguous uint8 / int16 / uint16 / int32 / uint32 / int64 HBM tensor")
    if seg.shape != img.shape:
        raise ValueError("img and seg must have the same shape, got %s and %s" % (tuple(img.shape), tuple(seg.shape)))
    rc = _capi.lib().pxsom_zero_by_seg(img.data_ptr(), PLANE_DTYPES[img.dtype], seg.data_ptr(), SEG_DTYPES[seg.dtype],
                                       img.numel(), 1 if exclude else 0, _capi.stream_ptr())
    _capi.check(rc, "pxsom_zero_by_seg")
    return img


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


# pxsom_cellquant (K12): image dtypes (PXSOM_SEG_* codes) and modes
CELLQUANT_IMAGE_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.uint16: 2, torch.int32: 3, torch.float64: 6,
                          torch.float32: 7}
CELLQUANT_MODES = {"total_intensity": 0, "positive_pixel": 1, "center_weighting": 2}
CELLQUANT_FORCE_SEARCH = 1
CELLQUANT_NUC_CAPACITY = 128


def label_keys(seg: torch.Tensor) -> torch.Tensor:
    """The sorted unique nonzero labels of an HBM label image as the int32 key table of :func:`cell_quantify`.
    Labels must be positive int32 values (NotImplementedError otherwise: negative labels and labels past int32 have no
    cell-table row the reference's int32 label column could name)."""
    wide = seg if seg.dtype in (torch.int32, torch.int64) else seg.to(
        torch.int64 if seg.dtype == torch.uint32 else torch.int32)
    keys = torch.unique(wide, sorted=True)
    if keys.numel():
        lo, hi = (int(v) for v in keys[[0, -1]].cpu())
        if lo < 0 or hi > 2147483647:
            raise NotImplementedError("cell table: labels must lie in 0 .. 2147483647, got %d .. %d" % (lo, hi))
        if lo == 0:
            keys = keys[1:]
    return keys.to(torch.int32)


def _label_image(seg: torch.Tensor, what: str):
    if seg.dim() != 2 or not seg.is_cuda or seg.dtype not in SEG_DTYPES:
        raise ValueError("%s must be a 2-D uint8 / int16 / uint16 / int32 / uint32 / int64 HBM tensor" % what)
    h, w = seg.shape
    if h == 0 or w == 0:
        raise ValueError("%s must not be empty" % what)
    if w > 1 and seg.stride(1) != 1:
        raise ValueError("%s rows must be contiguous (stride(1) == 1)" % what)
    return h, w, seg.stride(0) if h > 1 else w


def _key_range(keys: torch.Tensor):
    if keys.dtype != torch.int32 or keys.dim() != 1 or not keys.is_cuda or not keys.is_contiguous():
        raise ValueError("keys must be a contiguous int32 HBM vector")
    if keys.numel() == 0:
        return 0, 0
    lo, hi = (int(v) for v in keys[[0, -1]].cpu())
    return lo, hi


def cell_quantify(seg: torch.Tensor, img: torch.Tensor, keys: Optional[torch.Tensor] = None,
                  mode: str = "total_intensity", threshold: float = 0.0, nuc: Optional[torch.Tensor] = None,
                  nuc_keys: Optional[torch.Tensor] = None, nuc_capacity: int = 0, force_search: bool = False) -> dict:
    """One pass of pxsom_cellquant: the per-cell table of a ``[H, W]`` label image (any row stride) over a contiguous
    ``[H, W, C]`` (or ``[H, W]``) HBM image.  ``keys`` (default :func:`label_keys` of ``seg``) name the cells, sorted
    ascending, unique and positive.  Returns a dict of HBM tensors: ``keys``, ``count`` [n] int64, ``sums`` [n, 2] int64
    (row, column), ``bbox`` [n, 4] int32 (row min, row max, column min, column max), ``values`` [n, C] float64 (``mode``
    total_intensity / positive_pixel with ``threshold``, compared in binary64 / center_weighting), and with a nuclear
    label image ``nuc``: ``nuc`` [n] int32, the index in ``nuc_keys`` (default :func:`label_keys` of ``nuc``, also
    returned as ``nuc_keys``) of the nucleus with the most pixels in the cell, the smaller on a tie, -1 for none.
    ``nuc_capacity`` bounds the per-cell overlap table (0: 128); ``force_search`` takes the binary-search route for
    both key tables."""
    h, w, ld = _label_image(seg, "seg")
    if img.dim() == 2:
        img = img.unsqueeze(-1)
    if img.dim() != 3 or tuple(img.shape[:2]) != (h, w) or not img.is_cuda or not img.is_contiguous() or \
            img.dtype not in CELLQUANT_IMAGE_DTYPES:
        raise ValueError("img must be a contiguous [H, W, C] uint8 / int16 / uint16 / int32 / float32 / float64 HBM "
                         "tensor of the segmentation's height and width")
    c = img.shape[2]
    if c == 0:
        raise ValueError("img must have at least one channel")
    if mode not in CELLQUANT_MODES:
        raise ValueError("mode must be one of %s" % sorted(CELLQUANT_MODES))
    if keys is None:
        keys = label_keys(seg)
    kmin, kmax = _key_range(keys)
    n = keys.numel()
    if n and kmin <= 0:
        raise ValueError("keys must be positive")
    dev = seg.device
    out = {"keys": keys,
           "count": torch.empty(n, dtype=torch.int64, device=dev),
           "sums": torch.empty((n, 2), dtype=torch.int64, device=dev),
           "bbox": torch.empty((n, 4), dtype=torch.int32, device=dev),
           "values": torch.empty((n, c), dtype=torch.float64, device=dev)}
    n_nuc, nmin, nmax, ldn, nuc_code = -1, 0, 0, w, 0
    if nuc is not None:
        if tuple(nuc.shape) != (h, w):
            raise ValueError("nuc must have the segmentation's shape")
        _, _, ldn = _label_image(nuc, "nuc")
        nuc_code = SEG_DTYPES[nuc.dtype]
        if nuc_keys is None:
            nuc_keys = label_keys(nuc)
        nmin, nmax = _key_range(nuc_keys)
        n_nuc = nuc_keys.numel()
        if n_nuc and nmin <= 0:
            raise ValueError("nuc_keys must be positive")
        out["nuc_keys"] = nuc_keys
        out["nuc"] = torch.empty(n, dtype=torch.int32, device=dev)
    if not 0 <= int(nuc_capacity) <= CELLQUANT_NUC_CAPACITY:
        raise ValueError("nuc_capacity must lie in 0 .. %d" % CELLQUANT_NUC_CAPACITY)
    flags = CELLQUANT_FORCE_SEARCH if force_search else 0
    img_code, mode_code = CELLQUANT_IMAGE_DTYPES[img.dtype], CELLQUANT_MODES[mode]
    lib = _capi.lib()
    wsb = lib.pxsom_cellquant_workspace_bytes(h, w, c, img_code, mode_code, n, kmin, kmax, n_nuc, nmin, nmax, flags)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib.pxsom_cellquant(seg.data_ptr(), SEG_DTYPES[seg.dtype], ld, nuc.data_ptr() if nuc is not None else None,
                             nuc_code, ldn, h, w, img.data_ptr(), img_code, c, keys.data_ptr() if n else None, n, kmin,
                             kmax, nuc_keys.data_ptr() if nuc is not None and n_nuc > 0 else None, n_nuc, nmin, nmax,
                             mode_code, float(threshold), int(nuc_capacity), out["count"].data_ptr(),
                             out["sums"].data_ptr(), out["bbox"].data_ptr(), out["values"].data_ptr(),
                             out["nuc"].data_ptr() if nuc is not None else None, ws.data_ptr(), wsb, flags,
                             _capi.stream_ptr())
    _capi.check(rc, "pxsom_cellquant")
    return out


# pxsom_region_shape / pxsom_region_hull (K17)
REGION_FORCE_SEARCH = 1
REGION_MAX_SIDE = 64           # the device route of the hull: bounding boxes up to 64 x 64
CONCAVITY_DEFAULTS = {"small_concavity_minimum": 10, "max_compactness": 60, "large_concavity_minimum": 150}


def region_props(seg: torch.Tensor, keys: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                 sums: Optional[torch.Tensor] = None, bbox: Optional[torch.Tensor] = None,
                 small_concavity_minimum: float = 10, max_compactness: float = 60,
                 large_concavity_minimum: float = 150, force_search: bool = False) -> dict:
    """The raw integers of the morphology regionprops of a ``[H, W]`` HBM label image (any row stride), one row per key
    (default :func:`label_keys` of ``seg``): a dict of HBM tensors ``keys``, ``count`` [n] int64, ``sums`` [n, 2] int64,
    ``bbox`` [n, 4] int32 (taken from the arguments when :func:`cell_quantify` already produced all three, computed in
    the same pass otherwise), ``shape`` [n, 6] int64 (sum r^2, sum c^2, sum r c, and the border pixels of perimeter
    weight 1, sqrt 2 and (1 + sqrt 2) / 2), ``hull`` [n, 4] int64 (convex area, convex row sum, convex column sum,
    concavities) and ``left_out`` [n] int32: 1 for a cell whose bounding box is past 64 x 64, whose ``hull`` row is 0 and
    is the host route's to fill (regionprops_extraction.host_hull)."""
    h, w, ld = _label_image(seg, "seg")
    if keys is None:
        keys = label_keys(seg)
    kmin, kmax = _key_range(keys)
    n = keys.numel()
    if n and kmin <= 0:
        raise ValueError("keys must be positive")
    given = [t is not None for t in (count, sums, bbox)]
    if any(given) and not all(given):
        raise ValueError("count, sums and bbox go together (all three from cell_quantify, or none)")
    dev = seg.device
    have = all(given)
    if have:
        ok = (count.dtype == torch.int64 and tuple(count.shape) == (n,) and sums.dtype == torch.int64 and
              tuple(sums.shape) == (n, 2) and bbox.dtype == torch.int32 and tuple(bbox.shape) == (n, 4))
        if not ok or not all(t.is_cuda and t.is_contiguous() for t in (count, sums, bbox)):
            raise ValueError("count [n] int64, sums [n, 2] int64 and bbox [n, 4] int32 must be contiguous HBM tensors")
    else:
        count = torch.empty(n, dtype=torch.int64, device=dev)
        sums = torch.empty((n, 2), dtype=torch.int64, device=dev)
        bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    for name, v in (("small_concavity_minimum", small_concavity_minimum), ("max_compactness", max_compactness),
                    ("large_concavity_minimum", large_concavity_minimum)):
        if float(v) != float(v):
            raise ValueError("%s must not be NaN" % name)
    out = {"keys": keys, "count": count, "sums": sums, "bbox": bbox,
           "shape": torch.empty((n, 6), dtype=torch.int64, device=dev),
           "hull": torch.empty((n, 4), dtype=torch.int64, device=dev),
           "left_out": torch.empty(n, dtype=torch.int32, device=dev)}
    flags = REGION_FORCE_SEARCH if force_search else 0
    lib = _capi.lib()
    wsb = lib.pxsom_region_shape_workspace_bytes(n, kmin, kmax, flags)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    code = SEG_DTYPES[seg.dtype]
    rc = lib.pxsom_region_shape(seg.data_ptr(), code, ld, h, w, keys.data_ptr() if n else None, n, kmin, kmax,
                                out["shape"].data_ptr(), None if have else count.data_ptr(),
                                None if have else sums.data_ptr(), None if have else bbox.data_ptr(), ws.data_ptr(),
                                wsb, flags, _capi.stream_ptr())
    _capi.check(rc, "pxsom_region_shape")
    rc = lib.pxsom_region_hull(seg.data_ptr(), code, ld, h, w, keys.data_ptr() if n else None, n, count.data_ptr(),
                               bbox.data_ptr(), float(small_concavity_minimum), float(max_compactness),
                               float(large_concavity_minimum), out["hull"].data_ptr(), out["left_out"].data_ptr(),
                               _capi.stream_ptr())
    _capi.check(rc, "pxsom_region_hull")
    return out


# pxsom_nuclear_overlaps / pxsom_split_apply (K21)
NUCSPLIT_FORCE_SEARCH = 1


def _split_planes(cell: torch.Tensor, nuc: torch.Tensor, cell_keys, nuc_keys):
    """The shared arguments of the two K21 entries: shape, strides, dtype codes, the key tables and their ranges."""
    h, w, ldc = _label_image(cell, "cell")
    if tuple(nuc.shape) != (h, w):
        raise ValueError("cell and nuc must have one shape, got %s and %s" % (tuple(cell.shape), tuple(nuc.shape)))
    _, _, ldn = _label_image(nuc, "nuc")
    if nuc.device != cell.device:
        raise ValueError("cell and nuc must be on one device")
    if cell_keys is None:
        cell_keys = label_keys(cell)
    if nuc_keys is None:
        nuc_keys = label_keys(nuc)
    (cmin, cmax), (nmin, nmax) = _key_range(cell_keys), _key_range(nuc_keys)
    if (cell_keys.numel() and cmin <= 0) or (nuc_keys.numel() and nmin <= 0):
        raise ValueError("cell_keys and nuc_keys must be positive")
    return h, w, ldc, ldn, cell_keys, nuc_keys, (cell_keys.numel(), cmin, cmax), (nuc_keys.numel(), nmin, nmax)


def nuclear_overlaps(cell: torch.Tensor, nuc: torch.Tensor, cell_keys: Optional[torch.Tensor] = None,
                     nuc_keys: Optional[torch.Tensor] = None, force_search: bool = False, capacity: Optional[int] = None):
    """One streaming pass of pxsom_nuclear_overlaps over two ``[H, W]`` HBM label planes (uint8 .. int64 each, any row
    stride).  ``cell_keys`` / ``nuc_keys`` (default :func:`label_keys` of each plane) name the cells and the nuclei,
    sorted ascending, unique and positive.  Returns HBM tensors ``(keys, nuc_keys, best, inside, area)``: per cell the
    index in ``nuc_keys`` of the nucleus with the most pixels inside it (the smaller label on a tie, -1: none) and that
    count, both int32 ``[n_cells]``; per nucleus its pixels in the whole plane, int64 ``[n_nuc]``.  Two calls: the first
    counts the runs of the image, which is read back and sizes the pair table of the second (``capacity`` overrides the
    size: a table too small gives RuntimeError and writes nothing)."""
    h, w, ldc, ldn, cell_keys, nuc_keys, ck, nk = _split_planes(cell, nuc, cell_keys, nuc_keys)
    dev = cell.device
    flags = NUCSPLIT_FORCE_SEARCH if force_search else 0
    lib = _capi.lib()
    n = torch.empty(2, dtype=torch.int32, device=dev)
    best = torch.empty((max(ck[0], 1), 2), dtype=torch.int32, device=dev)
    area = torch.empty(max(nk[0], 1), dtype=torch.int64, device=dev)

    def call(area_ptr, best_ptr, cap, ws, wsb):
        rc = lib.pxsom_nuclear_overlaps(cell.data_ptr(), SEG_DTYPES[cell.dtype], ldc, nuc.data_ptr(), SEG_DTYPES[nuc.dtype],
                                        ldn, h, w, cell_keys.data_ptr() if ck[0] else None, *ck,
                                        nuc_keys.data_ptr() if nk[0] else None, *nk, area_ptr, best_ptr, cap, n.data_ptr(),
                                        ws, wsb, flags, _capi.stream_ptr())
        _capi.check(rc, "pxsom_nuclear_overlaps")

    if capacity is None:
        call(None, None, 0, None, 0)
        capacity = max(int(n[1].item()), 1)
    capacity = int(capacity)
    if not 1 <= capacity <= PAIR_CAPACITY_MAX:
        raise NotImplementedError("nuclear_overlaps: %d runs of label pairs are beyond the limit %d" % (capacity, PAIR_CAPACITY_MAX))
    wsb = lib.pxsom_nuclear_overlaps_workspace_bytes(capacity, *ck, *nk, flags)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    call(area.data_ptr(), best.data_ptr(), capacity, ws.data_ptr(), wsb)
    if int(n[0].item()) < 0:
        raise RuntimeError("nuclear_overlaps: %d runs of label pairs do not fit the capacity %d" % (int(n[1].item()), capacity))
    best = best[:ck[0]]
    return cell_keys, nuc_keys, best[:, 0], best[:, 1], area[:nk[0]]


def choose_splits(keys, nuc_keys, best, inside, area, cell_ids, min_size=15, small=5, first_new=None, dtype=None):
    """The choice of split_large_nuclei on the host over the tables of :func:`nuclear_overlaps` (host arrays).  Every
    entry of ``cell_ids``, in the caller's order and duplicates included, whose cell has a nucleus with
    ``area - inside > min_size`` takes the next new label (from ``first_new``, default ``max(nuc_keys) + 1``); a cell
    named twice keeps its last number, the earlier one stays without pixels.  The sizes after the split come from the
    tables -- a new label has ``inside`` pixels, a split nucleus keeps ``area`` minus the ``inside`` of the distinct cells
    that split it -- and every label below ``small`` pixels becomes 0 (``remove_small_objects`` on an integer plane: no
    connected components).  Returns ``(chosen, cell_value, nuc_value, n_splits)``, the three tables of
    :func:`split_nuclei_apply`: ``chosen`` int32 [n_cells], ``cell_value`` int64 [n_cells] (-1: the cell splits nothing),
    ``nuc_value`` int64 [n_nuc].  IndexError names a ``cell_ids`` entry that is no key; with the plane's numpy ``dtype``
    given, ValueError names it when the last new label does not fit it (the reference's numpy scalar wraps there)."""
    keys = np.asarray(keys, dtype=np.int64)
    nuc_keys = np.asarray(nuc_keys, dtype=np.int64)
    best = np.asarray(best, dtype=np.int64)
    inside = np.asarray(inside, dtype=np.int64)
    area = np.asarray(area, dtype=np.int64)
    ids = np.asarray(cell_ids).reshape(-1)
    if ids.size and ids.dtype.kind not in "iu":
        raise TypeError("cell_ids must be integers, got %s" % ids.dtype)
    ids = ids.astype(np.int64)
    seq = np.searchsorted(keys, ids)
    miss = keys[np.minimum(seq, keys.size - 1)] != ids if keys.size else np.ones(ids.size, dtype=bool)
    if miss.any():
        raise IndexError("split_large_nuclei: cell id %d is no label of the cell segmentation" % int(ids[miss][0]))
    if first_new is None:
        first_new = (int(nuc_keys[-1]) if nuc_keys.size else 0) + 1
    has = best >= 0
    outside = np.zeros(keys.size, dtype=np.int64)
    outside[has] = area[best[has]] - inside[has]
    splits = has & (outside > min_size)                            # per cell: would it split its nucleus?
    flag = splits[seq]
    number = int(first_new) - 1 + np.cumsum(flag)                  # per entry of cell_ids
    n_splits = int(flag.sum())
    if dtype is not None and n_splits and int(first_new) - 1 + n_splits > np.iinfo(dtype).max:
        raise ValueError("split_large_nuclei: %d new labels from %d on do not fit the nuclear plane's dtype %s"
                         % (n_splits, int(first_new), np.dtype(dtype)))
    cell_value = np.full(keys.size, -1, dtype=np.int64)
    np.maximum.at(cell_value, seq[flag], number[flag])             # the numbers ascend: the last entry of a cell wins
    done = cell_value >= 0
    remaining = area.copy()
    np.subtract.at(remaining, best[done], inside[done])
    nuc_value = np.where(remaining < small, 0, nuc_keys)
    cell_value[done & (inside < small)] = 0
    return best.astype(np.int32), cell_value, nuc_value.astype(np.int64), n_splits


def split_nuclei_apply(cell: torch.Tensor, nuc: torch.Tensor, cell_keys: torch.Tensor, nuc_keys: torch.Tensor,
                       chosen: torch.Tensor, cell_value: torch.Tensor, nuc_value: torch.Tensor,
                       out: Optional[torch.Tensor] = None, force_search: bool = False) -> torch.Tensor:
    """The write pass of pxsom_split_apply: ``out`` (the nuclear plane's dtype, any row stride, default a new plane) takes
    ``cell_value[c]`` where the pixel's cell ``c`` chose the pixel's nucleus (``chosen[c]``) and ``cell_value[c] >= 0``,
    else ``nuc_value[j]`` of its nucleus ``j``; a nuclear label outside ``nuc_keys`` is copied through."""
    h, w, ldc, ldn, cell_keys, nuc_keys, ck, nk = _split_planes(cell, nuc, cell_keys, nuc_keys)
    dev = cell.device
    for name, t, dtype, n in (("chosen", chosen, torch.int32, ck[0]), ("cell_value", cell_value, torch.int64, ck[0]),
                              ("nuc_value", nuc_value, torch.int64, nk[0])):
        if t.dtype != dtype or not t.is_cuda or t.dim() != 1 or not t.is_contiguous() or t.numel() != n:
            raise ValueError("%s must be a contiguous %s HBM vector of %d entries" % (name, str(dtype).replace("torch.", ""), n))
    out = _rows_plane(out, h, w, nuc.dtype, dev, "out")
    flags = NUCSPLIT_FORCE_SEARCH if force_search else 0
    lib = _capi.lib()
    wsb = lib.pxsom_split_apply_workspace_bytes(*ck, *nk, flags)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    rc = lib.pxsom_split_apply(cell.data_ptr(), SEG_DTYPES[cell.dtype], ldc, nuc.data_ptr(), SEG_DTYPES[nuc.dtype], ldn, h, w,
                               cell_keys.data_ptr() if ck[0] else None, *ck, nuc_keys.data_ptr() if nk[0] else None, *nk,
                               chosen.data_ptr() if ck[0] else None, cell_value.data_ptr() if ck[0] else None,
                               nuc_value.data_ptr() if nk[0] else None, out.data_ptr(), _ld(out), ws.data_ptr(), wsb, flags,
                               _capi.stream_ptr())
    _capi.check(rc, "pxsom_split_apply")
    return out


def split_large_nuclei(cell: torch.Tensor, nuc: torch.Tensor, cell_ids=None, min_size=15, small=5,
                       out: Optional[torch.Tensor] = None, force_search: bool = False) -> torch.Tensor:
    """The device chain of ``segmentation_utils.split_large_nuclei`` on two ``[H, W]`` HBM label planes -> the modified
    nuclear plane in HBM, in the nuclear plane's dtype.  For every id of ``cell_ids`` (default: every cell label
    ascending), in that order: the nucleus with the most pixels inside the cell (the smallest label on a tie) is
    renumbered inside the cell when more than ``min_size`` of its pixels lie outside it; then every label below ``small``
    pixels is removed.  Only the per-cell and per-nucleus tables are read back for the choice (:func:`choose_splits`);
    the planes stay in HBM.  ValueError when the new labels do not fit the nuclear plane's dtype (the reference's numpy
    scalar wraps there), raised before the write pass."""
    keys, nuc_keys, best, inside, area = nuclear_overlaps(cell, nuc, force_search=force_search)
    keys_h = keys.cpu().numpy()
    if cell_ids is None:
        cell_ids = keys_h
    chosen, cell_value, nuc_value, _ = choose_splits(keys_h, nuc_keys.cpu().numpy(), best.cpu().numpy(), inside.cpu().numpy(),
                                                     area.cpu().numpy(), cell_ids, min_size, small,
                                                     dtype=np.dtype(str(nuc.dtype).replace("torch.", "")))
    dev = cell.device
    return split_nuclei_apply(cell, nuc, keys, nuc_keys, torch.from_numpy(chosen).to(dev), torch.from_numpy(cell_value).to(dev),
                              torch.from_numpy(nuc_value).to(dev), out=out, force_search=force_search)


# ---- neighbourhood matrix (K13) -------------------------------------------------------------------------------------
def _smallest_double(pred):
    """The smallest double s in [0, +inf] with ``pred(s)`` for a monotone pred (False, ..., False, True, ..., True),
    as its bit pattern; None when pred(+inf) is False.  Non-negative doubles order as their bit patterns do."""
    def at(bits):
        return bool(pred(np.array(bits, dtype=np.uint64).view(np.float64)[()]))
    lo, hi = 0, 0x7FF0000000000000
    if not at(hi):
        return None
    if at(lo):
        return lo
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if at(mid):
            hi = mid
        else:
            lo = mid
    return hi


def neighbor_thresholds(distlim) -> Tuple[float, float]:
    """``(s_lim, s_zero)`` for pxsom_neighbor_counts: with ``d = float32(sqrt(s))`` the entry of the reference's distance
    matrix for a squared distance s, ``d < distlim`` is ``s < s_lim`` and ``d == 0`` is ``s <= s_zero``, exactly --
    sqrt and the cast to float32 are correctly rounded and monotone, so each test flips at one double, found here by
    bisection over the bit patterns.  ``distlim`` compares in the dtype numpy compares a float32 array with it in
    (``np.result_type(np.float32, distlim)``: a Python scalar in float32, an ``np.float64`` in float64)."""
    lim = np.result_type(np.float32, distlim).type(distlim)

    def d32(s):
        with np.errstate(over="ignore"):
            return np.float32(np.sqrt(s))
    at_lim = _smallest_double(lambda s: d32(s) >= lim)
    above_zero = _smallest_double(lambda s: d32(s) > 0)
    as_double = lambda bits: float(np.array(bits, dtype=np.uint64).view(np.float64)[()])  # noqa: E731
    # a NaN distlim is below nothing: s < 0 never holds
    return (0.0 if at_lim is None else as_double(at_lim)), as_double(above_zero - 1)


def _cell_args(xy: torch.Tensor, seg: torch.Tensor, check_rows):
    """The ``xy`` / ``seg`` checks of the cell-geometry calls, with the caller's checks of its per-row vectors
    (``check_rows(n, device)``) in their place between the two: ``(n, device, seg made contiguous, n_fovs)``."""
    if xy.dim() != 2 or xy.shape[1] != 2 or xy.dtype != torch.float64 or not xy.is_cuda:
        raise ValueError("xy must be an [n, 2] float64 HBM tensor")
    check_rows(xy.shape[0], xy.device)
    if seg.dim() != 1 or seg.numel() < 1 or seg.dtype != torch.int64 or seg.device != xy.device:
        raise ValueError("seg must be an [F + 1] int64 HBM vector on xy's device")
    return xy.shape[0], xy.device, seg.contiguous(), seg.numel() - 1


def _check_offsets(seg: torch.Tensor, n: int, *more) -> list:
    """ValueError unless ``seg`` is right.  A call's one read-back: it returns the values of the 0-d bools ``more``."""
    ok = torch.stack([seg[0] == 0, seg[-1] == n, (seg[1:] >= seg[:-1]).all(), *more]).cpu()
    if not bool(ok[:3].all()):
        raise ValueError("seg must be non-decreasing offsets from 0 to n")
    return ok[3:].tolist()


def _cells_sorted_by_type(xy: torch.Tensor, types: torch.Tensor, seg: torch.Tensor, n_types: int):
    """The arguments :func:`neighbor_counts` and :func:`nearest_type_means` share, checked (one read-back), and the cells
    as their kernels want them: sorted by type inside each FOV.  Returns ``(xy_s, types_s, seg, order, n_fovs)``; sorted
    row r is the caller's row ``order[r]``.  With no cells the first two and ``order`` are None."""
    def check_types(n, dev):
        if types.dim() != 1 or types.shape[0] != n or types.dtype not in (torch.int32, torch.int64) or types.device != dev:
            raise ValueError("types must be an [n] int32 / int64 HBM vector on xy's device")
    n, dev, seg, n_fovs = _cell_args(xy, seg, check_types)
    if n_types < 1:
        raise ValueError("n_types must be at least 1")
    if not _check_offsets(seg, n, ((types >= 0) & (types < n_types)).all())[0]:
        raise ValueError("types must lie in [0, n_types)")
    if n == 0:
        return None, None, seg, None, n_fovs
    rows = torch.arange(n, device=dev)
    fov = torch.searchsorted(seg[1:], rows, right=True)
    order = torch.argsort(fov * n_types + types.to(torch.int64), stable=True)
    return xy[order].contiguous(), types[order].to(torch.int32).contiguous(), seg, order, n_fovs


def neighbor_counts(xy: torch.Tensor, types: torch.Tensor, seg: torch.Tensor, n_types: int, distlim,
                    self_neighbor: bool = False) -> torch.Tensor:
    """pxsom_neighbor_counts: ``counts[i, t]`` (``[n, n_types]`` int32, HBM) = how many cells j of cell i's FOV with
    ``types[j] == t`` have ``float32(dist(i, j)) < distlim`` (and ``!= 0`` unless ``self_neighbor``), dist the binary64
    Euclidean distance of the centroids ``xy`` [n, 2] -- the reference's compute_neighbor_counts over calc_dist_matrix's
    matrix, which is never built.  ``types`` [n] int32 / int64 in [0, n_types); ``seg`` [F + 1] int64 offsets (FOV f is
    rows seg[f] .. seg[f + 1], seg[0] = 0, seg[F] = n, empty FOVs allowed).  Rows come in and go out in the caller's
    order: the sort by type inside each FOV that the kernel wants is done here."""
    n_types = operator.index(n_types)
    xy_s, types_s, seg, order, n_fovs = _cells_sorted_by_type(xy, types, seg, n_types)
    s_lim, s_zero = neighbor_thresholds(distlim)
    n = xy.shape[0]
    counts = torch.empty((n, n_types), dtype=torch.int32, device=xy.device)
    if n == 0:
        return counts
    sorted_counts = torch.empty_like(counts)
    rc = _capi.lib().pxsom_neighbor_counts(xy_s.data_ptr(), types_s.data_ptr(), seg.data_ptr(), n_fovs, n, n_types,
                                           s_lim, s_zero, 1 if self_neighbor else 0, sorted_counts.data_ptr(),
                                           _capi.stream_ptr())
    _capi.check(rc, "pxsom_neighbor_counts")
    counts[order] = sorted_counts
    return counts


CLOSE_PAIR_MAX_SETS = 64    # pxsom_close_pair_counts: a set is a bit of a 64-bit membership mask


def close_pair_counts(xy: torch.Tensor, member_q: torch.Tensor, member_c: torch.Tensor, seg: torch.Tensor,
                      n_sets_q: int, n_sets_c: int, distlim, self_neighbor: bool = False) -> torch.Tensor:
    """pxsom_close_pair_counts: ``out[f, s, t]`` (``[F, n_sets_q, n_sets_c]`` int64, HBM) = the number of ordered pairs
    (a, b) of cells of FOV f with bit s of ``member_q[a]`` and bit t of ``member_c[b]`` set and
    ``float32(dist(a, b)) < distlim`` (and ``!= 0`` unless ``self_neighbor``: without it a cell pairs neither with itself
    nor with a cell on its own centroid) -- the pair test of :func:`neighbor_counts`, the N x N matrix never built.
    ``member_q`` / ``member_c`` are ``[n]`` int64 tensors holding the uint64 masks (bit 63 is the sign bit; they may be
    the same tensor); bits at or above the set counts are ignored.  ``1 <= n_sets <= 64``: callers with more sets go
    through blocks of 64 rows x 64 columns.  ``seg`` as for :func:`neighbor_counts`; the rows need no order inside a
    FOV.  The entry clears the output itself."""
    n_sets_q, n_sets_c = operator.index(n_sets_q), operator.index(n_sets_c)
    def check_members(n, dev):
        for name, m in (("member_q", member_q), ("member_c", member_c)):
            if m.dim() != 1 or m.shape[0] != n or m.dtype != torch.int64 or m.device != dev:
                raise ValueError("%s must be an [n] int64 HBM vector (the bits of a uint64 mask) on xy's device" % name)
    n, dev, seg, n_fovs = _cell_args(xy, seg, check_members)
    if not (1 <= n_sets_q <= CLOSE_PAIR_MAX_SETS and 1 <= n_sets_c <= CLOSE_PAIR_MAX_SETS):
        raise ValueError("n_sets_q and n_sets_c must lie in 1 .. %d, got %d and %d"
                         % (CLOSE_PAIR_MAX_SETS, n_sets_q, n_sets_c))
    _check_offsets(seg, n)
    s_lim, s_zero = neighbor_thresholds(distlim)
    out = torch.empty((n_fovs, n_sets_q, n_sets_c), dtype=torch.int64, device=dev)
    if n_fovs == 0:
        return out
    xy, same = xy.contiguous(), member_c is member_q
    member_q = member_q.contiguous()
    member_c = member_q if same else member_c.contiguous()
    rc = _capi.lib().pxsom_close_pair_counts(xy.data_ptr(), member_q.data_ptr(), member_c.data_ptr(), seg.data_ptr(),
                                             n_fovs, n, n_sets_q, n_sets_c, s_lim, s_zero, 1 if self_neighbor else 0,
                                             out.data_ptr(), _capi.stream_ptr())
    _capi.check(rc, "pxsom_close_pair_counts")
    return out


# ---- cell-distance analysis (K14) -----------------------------------------------------------------------------------
NEAREST_MAX_K = 32      # pxsom_nearest_type_means keeps the k smallest squared distances in registers
_S_ZERO = None


def _nearest_s_zero() -> float:
    """neighbor_thresholds' s_zero (it does not depend on distlim), bisected once per process."""
    global _S_ZERO
    if _S_ZERO is None:
        _S_ZERO = neighbor_thresholds(1)[1]
    return _S_ZERO


def nearest_type_means(xy: torch.Tensor, types: torch.Tensor, seg: torch.Tensor, n_types: int, k: int) -> torch.Tensor:
    """pxsom_nearest_type_means: ``means[i, t]`` (``[n, n_types]`` float32, HBM) = the mean of the k smallest non-zero
    float32 distances from cell i to the cells j of its FOV with ``types[j] == t``, NaN when fewer than k are non-zero
    -- the reference's calculate_mean_distance_to_cell_type over calc_dist_matrix's matrix, which is never built, bit for
    bit (float32 sum in numpy's pairwise order).  Arguments as for :func:`neighbor_counts`; ``1 <= k <= 32``.  Rows come
    in and go out in the caller's order: the sort by type inside each FOV that the kernel wants is done here."""
    k = operator.index(k)
    if not 1 <= k <= NEAREST_MAX_K:
        raise ValueError("k must lie in 1 .. %d (the device route keeps the k nearest in registers), got %d"
                         % (NEAREST_MAX_K, k))
    n_types = operator.index(n_types)
    xy_s, types_s, seg, order, n_fovs = _cells_sorted_by_type(xy, types, seg, n_types)
    s_zero = _nearest_s_zero()
    n = xy.shape[0]
    means = torch.empty((n, n_types), dtype=torch.float32, device=xy.device)
    if n == 0:
        return means
    sorted_means = torch.empty_like(means)
    rc = _capi.lib().pxsom_nearest_type_means(xy_s.data_ptr(), types_s.data_ptr(), seg.data_ptr(), n_fovs, n, n_types, k,
                                              s_zero, sorted_means.data_ptr(), _capi.stream_ptr())
    _capi.check(rc, "pxsom_nearest_type_means")
    means[order] = sorted_means
    return means


# ---- silhouette sweeps (K15) ----------------------------------------------------------------------------------------
SILHOUETTE_MAX_D = 64   # pxsom_silhouette keeps a row in registers
SILHOUETTE_MAX_K = 32


def _silhouette(x: torch.Tensor, labels: torch.Tensor, n_clusters):
    """The checks, the sort by label and the one pxsom_silhouette call behind :func:`silhouette_samples` and
    :func:`silhouette_scores`: ``(samples [M, n], scores [M], single)``, ``single`` when ``labels`` came as ``[n]``."""
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
    rc = _capi.lib().pxsom_silhouette(x.data_ptr(), n, d, labels32.data_ptr(), order.data_ptr(), n_labelings, k,
                                      counts.data_ptr(), sums.data_ptr(), samples.data_ptr(), scores.data_ptr(),
                                      _capi.stream_ptr())
    _capi.check(rc, "pxsom_silhouette")
    return samples, scores, single


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
    rc = lib.pxsom_kmeans_lloyd(rows.data_ptr(), n, d, n_problems, ks.ctypes.data, centres.data_ptr(), tols.ctypes.data,
                                iters.ctypes.data, labels.data_ptr(), inertia.ctypes.data, n_iter.ctypes.data,
                                ws.data_ptr(), ws_bytes, operator.index(workgroups), _capi.stream_ptr())
    _capi.check(rc, "pxsom_kmeans_lloyd")
    return labels, list(torch.split(centres, ks.tolist())), inertia, n_iter
