"""The fused 10 x 10 training step (pxsom_batch_step.hip): its duplicate-node mask by bucket tables -- and the linear scan
behind them, forced by PXSOM_TRAIN_SMALL_DUP_TABLES -- and its steps of 1, 2, 3 and 5 rounds of rows per workgroup,
against orc_som_batch_sched: the run's codebook bit for bit, every step's statistics against cluster_sums of the
oracle's labels for the codebook the step searched with.

What the mask tests can see: the labels do not depend on the mask (rows of two equal nodes that are NOT masked are listed and
settled exactly, to the first of them), so a mask that misses a duplicate is not observable through the API -- only slower.
A mask that hides a node which is no duplicate (one_ulp, random) changes labels and fails here; and the table path is held
against the linear scan, which PXSOM_TRAIN_SMALL_DUP_TABLES forces, step by step.  The rounds cases and the binary64 case
are regression cover of the row loop around the changed phase.

Rows are multiples of 2^-12 (binary16 rows: whatever that rounds to): sums of a million such values are exact in binary64,
so the statistics do not depend on the order of the atomic additions and bit equality is well defined.  `-m gpu` only."""
import numpy as np
import pytest
import torch

from ark_analysis_amd import _capi
from ark_analysis_amd import som_device as sd
from ark_analysis_amd import synth
from ark_analysis_amd.flowsom import default_radius_range
from ark_analysis_amd.schedule import BatchSchedule, resolve

pytestmark = pytest.mark.gpu

XD = YD = 10
K, C = 100, 22
ALPHA = (0.05, 0.01)
SMALL_DUP_TABLES = 4     # include/pxsom.h PXSOM_TRAIN_SMALL_DUP_TABLES
ROWS_PER_ROUND = 512     # per workgroup of the four-tile kernel; one workgroup per CU


def _steps(x, state, g_begin, g_end, total, rr, flags):
    """sd.batch_train_steps with the call's flags word handed through."""
    n, c, ldx, dt = sd._matrix_args(x)
    sch = state.schedule
    rc = _capi.lib().pxsom_batch_train_sched_from(
        x.data_ptr(), n, c, ldx, dt, None, state.wbuf.data_ptr(), state.ring.data_ptr(), state.xdim, state.ydim,
        sch.phases, state.edges.ctypes.data, sch.steps, int(g_begin), int(g_end), int(total) // sch.steps,
        float(ALPHA[0]), float(ALPHA[1]), float(rr[0]), float(rr[1]), float(state.quantum),
        state.ws.data_ptr(), state.ws_bytes, int(flags), None, _capi.stream_ptr())
    _capi.check(rc, "pxsom_batch_train_sched_from")


def _train(xd, w0, sch, passes, rr, flags=0, quantum=0.0, trace_steps=None):
    """Step by step: [(W_g, statistics of step g)] for the steps in trace_steps (None: all), and the run's codebook."""
    n, c = xd.shape
    st = sd.BatchTrainState(n, c, XD, YD, sch, xd.device, dtype=xd.dtype)
    st.quantum = quantum
    st.wbuf[0].copy_(torch.from_numpy(w0))
    total = passes * st.schedule.steps
    trace = {}
    for g in range(total):
        _steps(xd, st, g, g + 1, total, rr, flags)
        if trace_steps is None or g in trace_steps:
            trace[g] = (st.wbuf[g % 2].cpu().numpy().copy(), st.ring[g % 3].cpu().numpy().copy())
    w = torch.empty((K, c), dtype=torch.float64, device=xd.device)
    sd.batch_train_finish(st, total, total, ALPHA, rr, w)
    return trace, w.cpu().numpy()


def _check(oracle, x64, w0, sch, passes, rr, trace, w_final, quantum=0.0):
    n, c = x64.shape
    want = oracle.som_batch_sched(x64, w0, XD, YD, passes, ALPHA, rr, sch.phases, sch.edges, quantum)
    assert np.array_equal(w_final, want), "the run's codebook differs from the oracle's"
    xq = oracle.quantize(x64, quantum) if quantum > 0.0 else x64
    for g, (w_g, ring) in trace.items():
        idx = sch.rows_of_step(n, g)
        lab, _ = oracle.map_data_to_nodes(w_g, x64[idx]) if len(idx) else (np.empty(0, np.int32), None)
        s, cnt = oracle.cluster_sums(xq[idx].reshape(-1, c), lab, K)
        assert np.array_equal(ring[K * c:], cnt.astype(np.float64)), f"counts of step {g}"
        assert np.array_equal(ring[: K * c].reshape(K, c), s), f"sums of step {g}"


def _data(n, seed, dtype=np.float32, c=C):
    x = synth.make_fov_numpy(max(n, 4 * K), c, seed=seed, dtype=np.float64)[:n]
    return np.ascontiguousarray((np.round(x * 4096.0) / 4096.0).astype(dtype))


def _rows_codebook(x, seed):
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray(x[rs.choice(x.shape[0], size=K, replace=False)].astype(np.float64))


# ---- the duplicate mask -----------------------------------------------------------------------------------------------
def _w0_random(w):
    return w


def _pair(i, j):
    def make(w):
        w[j] = w[i]
        return w
    return make


def _w0_triple(w):
    w[50] = w[12]
    w[70] = w[12]
    return w


def _w0_all_equal(w):
    w[:] = w[0]
    return w


def _w0_one_ulp(w):   # not duplicates: one channel of the copy is the next binary64 number
    w[37] = w[3]
    w[37, 5] = np.nextafter(w[3, 5], np.inf)
    w[99] = w[98]
    w[99, 21] = np.nextafter(w[98, 21], -np.inf)
    return w


def _w0_pairs_and_triple(w):
    return _w0_triple(_pair(3, 37)(w))


WIDE = (12.0, 1.0)       # the first radius covers the whole grid: every window is the grid, every node the same mean
KINDS = {
    # name: (W0 maker, rows, radius range (None: the default), schedules)
    "random": (_w0_random, 3000, None, ("default", 4, 7)),
    "pair_0_99": (_pair(0, 99), 3000, None, ("default", 4)),
    "pair_3_37": (_pair(3, 37), 2500, None, ("default", 7)),
    "pair_98_99": (_pair(98, 99), 3000, None, ("default", 4)),
    "triple": (_w0_triple, 4000, None, ("default", 7)),
    "all_equal": (_w0_all_equal, 3000, None, ("default", 4)),
    "one_ulp": (_w0_one_ulp, 3000, None, ("default", 4)),
    "whole_grid_windows": (_w0_random, 2000, WIDE, ("default", 4, 7)),
    # 50 rows per step for 100 nodes under 3 x 3 windows: nodes whose window holds no row stay (gain < 0), duplicates with them
    "starved": (_w0_pairs_and_triple, 2000, (1.6, 1.1), (40,)),
}


@pytest.mark.parametrize("kind,schedule", [(k, s) for k, v in KINDS.items() for s in v[3]])
def test_duplicate_mask_matches_the_oracle_with_and_without_the_scan(gpu, oracle, kind, schedule):
    make, n, rr, _ = KINDS[kind]
    rr = rr or default_radius_range(XD, YD)
    sch = BatchSchedule.two_phase() if schedule == "default" else resolve(schedule)
    x = _data(n, seed=71)
    w0 = make(_rows_codebook(x, seed=8))
    xd = torch.from_numpy(x).to(gpu)
    x64 = x.astype(np.float64)
    runs = [_train(xd, w0, sch, 1, rr, flags) for flags in (0, SMALL_DUP_TABLES)]
    for g in runs[0][0]:
        assert np.array_equal(runs[0][0][g][0], runs[1][0][g][0]), f"codebook of step {g}: tables and scan differ"
        assert np.array_equal(runs[0][0][g][1], runs[1][0][g][1]), f"statistics of step {g}: tables and scan differ"
    assert np.array_equal(runs[0][1], runs[1][1])
    for trace, w in runs:
        _check(oracle, x64, w0, sch, 1, rr, trace, w)


def test_forty_random_codebooks_through_the_scan(gpu, oracle):
    """4 buckets per table: every node but the first few finds an earlier node in both of its buckets and scans."""
    n, sch, rr = 2000, resolve(4), default_radius_range(XD, YD)
    x = _data(n, seed=72)
    xd = torch.from_numpy(x).to(gpu)
    x64 = x.astype(np.float64)
    for seed in range(40):
        rs = np.random.RandomState(1000 + seed)
        w0 = _rows_codebook(x, seed=100 + seed)
        for _ in range(seed % 4):                       # none to three copies of an earlier or later node
            i, j = rs.choice(K, size=2, replace=False)
            w0[j] = w0[i]
        trace, w = _train(xd, w0, sch, 1, rr, SMALL_DUP_TABLES)
        _, w_tables = _train(xd, w0, sch, 1, rr, 0, trace_steps=())
        assert np.array_equal(w, w_tables), f"seed {seed}: tables and scan differ"
        _check(oracle, x64, w0, sch, 1, rr, trace, w)


# ---- rounds -----------------------------------------------------------------------------------------------------------
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rounds(rows):
    return -(-rows // (ROWS_PER_ROUND * _cus()))


TWO_EQUAL = BatchSchedule(2, [0, 1, 2])
SEVEN_OF_EIGHT = BatchSchedule(8, [0, 7, 8])     # step 0: 7 consecutive rows out of every 8 -- the scheduled group_w > 1 view


def _first_step_rows(rounds, blocks_past, rows_past):
    """Rows of a step of `rounds` rounds: (rounds - 1) full ones, then `blocks_past` blocks and `rows_past` rows more."""
    return ROWS_PER_ROUND * ((rounds - 1) * _cus() + blocks_past) + rows_past


@pytest.mark.parametrize("name,rounds,blocks_past,rows_past,sch,dtype,padded", [
    ("one_round", 1, -2, 37, TWO_EQUAL, np.float32, False),          # (0 full rounds + CUs - 2 blocks + 37 rows)
    # an odd number of blocks on an even number of workgroups: the last workgroup has no second round; last block partly empty
    ("two_rounds_last_wg_idle", 2, 3, -100, TWO_EQUAL, np.float32, False),
    ("two_rounds_f16", 2, 7, 5, TWO_EQUAL, np.float16, False),
    ("three_rounds_padded_view", 3, 11, 9, TWO_EQUAL, np.float32, True),      # ldx > c
    ("five_rounds_grouped_view", 5, 5, 77, SEVEN_OF_EIGHT, np.float32, False),
])
def test_rounds_match_the_oracle(gpu, oracle, name, rounds, blocks_past, rows_past, sch, dtype, padded):
    cus = _cus()
    rows0 = _first_step_rows(rounds, blocks_past if rounds > 1 else cus + blocks_past, rows_past)
    width = sch.edges[1] - sch.edges[0]
    n = (rows0 // width) * sch.phases + rows0 % width
    assert len(sch.rows_of_step(n, 0)) == rows0 and _rounds(rows0) == rounds and rows0 > 256 * cus
    x = _data(n, seed=73, dtype=dtype)
    w0 = _rows_codebook(x[: 50_000], seed=9)
    w0[91] = w0[17]                                      # a duplicate node
    xd = torch.from_numpy(x).to(gpu)
    if padded:
        wide = torch.zeros((n, C + 4), dtype=xd.dtype, device=gpu)
        wide[:, :C] = xd
        xd = wide[:, :C]
    rr = default_radius_range(XD, YD)
    trace, w = _train(xd, w0, sch, 1, rr)
    _check(oracle, x.astype(np.float64), w0, sch, 1, rr, trace, w)


def test_binary64_rows_take_many_rounds_of_one_tile(gpu, oracle):
    """binary64 rows keep one tile per wave: a step of more than three rounds of 128 rows per workgroup, statistics exact
    through the run's quantum."""
    cus = _cus()
    rows0 = 128 * (3 * cus + 5) + 19
    n = 2 * rows0
    x = _data(n, seed=74, dtype=np.float64)
    w0 = _rows_codebook(x[: 50_000], seed=10)
    w0[91] = w0[17]
    quantum = sd.exact_sum_quantum(float(np.abs(x).max()), n)
    assert quantum > 0.0
    xd = torch.from_numpy(x).to(gpu)
    rr = default_radius_range(XD, YD)
    trace, w = _train(xd, w0, TWO_EQUAL, 1, rr, quantum=quantum)
    _check(oracle, x, w0, TWO_EQUAL, 1, rr, trace, w, quantum=quantum)
