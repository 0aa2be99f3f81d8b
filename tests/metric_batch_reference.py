"""The batch rule under FlowSOM's other distances (distf 1, 3, 4), composed from the statements of record (TEST
INFRASTRUCTURE; the product never imports this module).

The loop is tests/oracle_backend.OracleKernels' with ``metric_reference.map_data_to_nodes(w, rows, distf)`` in place of the
Euclidean search: ``rows_of_step`` deals the rows, ``oracle_binding.quantize`` rounds them to the run's quantum,
``oracle_binding.cluster_sums`` (orc_cluster_sums; label-0 rows add nothing) gives the statistics, ``batch_schedule`` the
position on the online schedule and ``oracle_binding.batch_update`` (orc_batch_update) the new codebook.
"""
import numpy as np
import torch

from tests import metric_reference as mr
from tests import oracle_binding as ob


def step_stats(w, x, distf, quantum=0.0):
    """(labels, [k*c sums | k counts] float64) of the rows ``x`` against the codebook ``w``."""
    w = np.asarray(w, dtype=np.float64)
    xn = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, w.shape[1])
    lab, _ = mr.map_data_to_nodes(w, xn, distf)
    with np.errstate(all="ignore"):
        s, cnt = ob.cluster_sums(ob.quantize(xn, quantum), lab, w.shape[0])
    return lab, np.concatenate([s.reshape(-1), cnt.astype(np.float64)])


class MetricOracleKernels:
    """Same interface as ark_analysis_amd.distributed.HipKernels(metric=distf), on host memory."""

    def __init__(self, metric):
        self.metric = int(metric)

    def absmax(self, x):
        a = np.abs(x.numpy())
        a = a[np.isfinite(a)]
        return float(a.max()) if a.size else 0.0

    def begin(self, x, w, xdim, ydim, schedule, quantum=0.0):
        from ark_analysis_amd.schedule import resolve
        self.xdim, self.ydim, self.sch, self.quantum = xdim, ydim, resolve(schedule), float(quantum)
        k, c = w.shape
        self.w = [w.clone(), w.clone()]
        self.rings = [torch.zeros(k * (c + 1), dtype=torch.float64) for _ in range(3)]

    def ring(self, g):
        return self.rings[g % 3]

    def _update(self, w, g, total, alpha_range, radius_range):
        from ark_analysis_amd.distributed import batch_schedule
        k, c = w.shape
        passes = total // self.sch.steps
        thr, alpha = batch_schedule(self.sch.position(g), passes * self.sch.phases, alpha_range, radius_range)
        st = self.rings[g % 3]
        with np.errstate(all="ignore"):
            return torch.from_numpy(ob.batch_update(w.numpy(), self.xdim, self.ydim, st[: k * c].view(k, c).numpy(),
                                                    st[k * c:].numpy().astype(np.int64), thr, alpha))

    def steps(self, x, g0, g1, total, alpha_range, radius_range):
        for g in range(g0, g1):
            if g > 0:
                self.w[g % 2] = self._update(self.w[(g - 1) % 2], g - 1, total, alpha_range, radius_range)
            w = self.w[g % 2]
            rows = self.sch.rows_of_step(x.shape[0], g)
            _, st = step_stats(w.numpy(), x.numpy()[rows], self.metric, self.quantum)
            self.rings[g % 3].copy_(torch.from_numpy(st))

    def finish(self, steps_done, total, alpha_range, radius_range, w):
        g = steps_done - 1
        w.copy_(self._update(self.w[g % 2], g, total, alpha_range, radius_range))


def som_batch(shards, w0, xdim, ydim, passes, schedule, alpha_range, radius_range, distf, quantum=0.0):
    """The codebook after ``passes`` passes of the rule over ``shards`` (a list of row matrices, one per rank: each rank deals
    ITS rows into the schedule's phases; the statistics of a step are summed over the ranks) from ``w0``."""
    from ark_analysis_amd.schedule import resolve
    sch = resolve(schedule)
    kerns = [MetricOracleKernels(distf) for _ in shards]
    xs = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64)) for s in shards]
    w0 = torch.from_numpy(np.ascontiguousarray(w0, dtype=np.float64))
    for kern, x in zip(kerns, xs):
        kern.begin(x, w0, xdim, ydim, sch, quantum=quantum)
    total = passes * sch.steps
    for g in range(total):
        for kern, x in zip(kerns, xs):
            kern.steps(x, g, g + 1, total, alpha_range, radius_range)
        both = sum(kern.ring(g) for kern in kerns)
        for kern in kerns:
            kern.ring(g).copy_(both)
    out = w0.clone()
    kerns[0].finish(total, total, alpha_range, radius_range, out)
    return out.numpy()


def run_quantum(shards, schedule):
    """The quantum BatchSOMTrainer._sum_quantum picks for a job whose ranks hold ``shards``."""
    from ark_analysis_amd import _capi
    from ark_analysis_amd.schedule import resolve
    sch = resolve(schedule)
    a = np.abs(np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1) for s in shards]))
    a = a[np.isfinite(a)]
    vmax = float(a.max()) if a.size else 0.0
    n_total, world = sum(len(s) for s in shards), len(shards)
    widest = max(b - a for a, b in zip(sch.edges, sch.edges[1:]))
    return float(_capi.lib().pxsom_exact_sum_quantum(vmax, (n_total // sch.phases + world) * max(widest, 1)))


def test_rows(n, c, seed, dtype=np.float64):
    """The issue's inputs: gamma-distributed rows with 40 % of the entries zeroed."""
    rng = np.random.RandomState(seed)
    x = rng.gamma(2.0, 1.0, size=(n, c))
    x[rng.random_sample((n, c)) < 0.4] = 0.0
    return x.astype(dtype)


test_rows.__test__ = False


def install(patch):
    """The stand-ins of tests/oracle_backend.install, plus metric-aware ones for the entry points that take a ``distf``."""
    from ark_analysis_amd import flowsom
    from tests import oracle_backend
    oracle_backend.install(patch)
    euclid_map = flowsom.map_data_to_nodes

    def map_data_to_nodes(nodes, newdata, distf=2):
        if distf == 2:
            return euclid_map(nodes, newdata)
        return mr.map_data_to_nodes(np.asarray(nodes, dtype=np.float64), np.asarray(newdata, dtype=np.float64), distf)

    patch(flowsom, "map_data_to_nodes", map_data_to_nodes)
    patch(flowsom, "_batch_backend_metric", lambda distf: (torch.device("cpu"), MetricOracleKernels(distf)))
