"""Full-size parity: every row of every BASELINE shape against the CPU oracle, and batch training step by step at full size.
`-m gpu` only.

(a) All-rows audit.  ``sd.assign`` labels and distances of EVERY row equal ``orc_map_data_to_nodes``'s bit for bit, on the
    shapes bench.py runs and on the codebooks that make the fp16-MFMA filter list most: trained, data rows (distance-0
    matches), node pairs 1e-2 apart, and W_1 of a pass (nodes pulled nearly together).  No sampling: the oracle labels all
    rows on the host (tests/full_size_reference.py: chunked, threaded).  On cfg2 and the sparse MIBI-like matrix the
    long-list kernel (``screen_all_lists``) and the one-pass mean table (``assign_means``) are audited too; on cfg4 / cfg5 the
    mean table's two-kernel route.
(b) Training at full size, step by step on the GPU's own trajectory: every step's statistics against the oracle's sums of
    the oracle's BMUs for the step's rows, every update equals ``orc_batch_update``, and where the sums are exact one
    ``BatchSOMTrainer.train`` call gives the same bits -- on the route bench.py takes for that shape.
(c) The statistics region of a mean-table workspace is really zero when the wrapper says so (an empty call after a failed
    one used to re-arm PXSOM_TABLES_SCRATCH_CLEAN over a dirty region).

Each audit case prints its row count, ``last_exact_rows`` and wall time (run with ``-s`` to see them).
"""
import math
import time

import numpy as np
import pytest
import torch

from ark_analysis_amd import som_device as sd
from ark_analysis_amd import synth
from ark_analysis_amd.distributed import BatchSOMTrainer, batch_schedule
from tests import full_size_reference as fr

pytestmark = pytest.mark.gpu

MPX = 1024 * 1024


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _assert_rows_equal(got: np.ndarray, want: np.ndarray, what: str, tag: str, ler: int) -> None:
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{tag}: {what} of {bad.size} of {got.size} rows differ from the oracle; first row {bad[0]}: "
                           f"{got[bad[0]]} != {want[bad[0]]}; last_exact_rows {ler}")


def fixed_point_tolerance(w: torch.Tensor, n: int, counts: np.ndarray, ref_means: np.ndarray):
    """Per-mean bound |mean_device - mean_binary64| of the one-pass table (include/pxsom.h, pxsom_assign_sums ACCURACY CONTRACT).

    - The filter scales by 2^e, e the integer with |W|max * 2^e in [128, 256): with |W|max = m * 2^E, m in [0.5, 1)
      (frexp), e = 8 - E.
    - Inside a workgroup every value enters the table rounded to a multiple of 2^-s, s = 46 + e - max(11, ceil(log2 r)),
      r the rows the workgroup meets.  r <= n, and s falls as r grows: s = 46 + e - max(11, ceil(log2 n)) is a lower
      bound, 2^-s an upper bound on the unit.
    - One rounding per value: at most 2^-(s+1) each; a sum of cnt values is off by at most cnt * 2^-(s+1), its mean by at
      most 2^-(s+1) -- whatever cnt.  Values the format does not hold and listed rows are added in binary64 instead.
    - Allowance for binary64 rounding: the reference's own recursive sums (chunked, in order), the device's binary64 flushes
      of workgroup partials and bypassing rows, and the division: (2 cnt + 4) * 2^-53 * |mean| (the audited rows are
      non-negative, so sum |x| = |sum x|).

    Returns (per-mean tolerance [K, C], the fixed-point term 2^-(s+1))."""
    wmax = float(w.abs().max())
    _, big_e = math.frexp(wmax)
    e = 8 - big_e
    assert 128.0 <= wmax * 2.0 ** e < 256.0
    s = 46 + e - max(11, math.ceil(math.log2(n)))
    fixed = 2.0 ** -(s + 1)
    allowance = (2.0 * counts[:, None] + 4.0) * 2.0 ** -53 * np.abs(ref_means)
    return fixed + allowance, fixed


def _audit(tag: str, x: torch.Tensor, w: torch.Tensor, screen: bool = False, means: str = None) -> np.ndarray:
    """Labels and distances of every row of ``x`` against the oracle; ``screen``: the long-list kernel too; ``means``:
    "fixed" (the one-pass table's contract) or "exact" (two-kernel route: binary64 sums within a few ulp of the exact sums)
    for ``assign_means``.  Returns the labels."""
    t0 = time.time()
    n, c = x.shape
    k = w.shape[0]
    labels, dists = sd.assign(x, w, want_dists=True)
    ler = sd.last_exact_rows(sd.assign.last_workspace)
    res = fr.oracle_labels(w, x, with_sums=means == "fixed")
    want_l, want_d = res[0], res[1]
    lab = labels.cpu().numpy()
    _assert_rows_equal(lab, want_l, "labels", tag, ler)
    _assert_rows_equal(dists.cpu().numpy().view(np.int64), want_d.view(np.int64), "distance bits", tag, ler)
    del dists
    if screen:
        l2, _ = sd.assign(x, w, screen_all_lists=True)
        _assert_rows_equal(l2.cpu().numpy(), want_l, "screen_all_lists labels", tag, sd.last_exact_rows(sd.assign.last_workspace))
        del l2
    if means is not None:
        ws = sd.AssignSumsWorkspace(n, c, k, x.device)
        lm = torch.empty(n, dtype=torch.int32, device=x.device)
        sums = torch.empty((k, c), dtype=torch.float64, device=x.device)
        cnt = torch.empty(k, dtype=torch.int64, device=x.device)
        mns = torch.empty((k, c), dtype=torch.float64, device=x.device)
        sd.assign_means(x, w, lm, sums, cnt, mns, ws)
        assert torch.equal(lm, labels), f"{tag}: assign_means labels differ from assign's"
        counts = cnt.cpu().numpy()
        np.testing.assert_array_equal(counts, np.bincount(lab - 1, minlength=k), err_msg=f"{tag}: assign_means counts")
        got_s, got_m = sums.cpu().numpy(), mns.cpu().numpy()
        # means = sums / max(count, 1): one binary64 division, the same on the host
        np.testing.assert_array_equal(got_m, got_s / np.maximum(counts, 1)[:, None], err_msg=f"{tag}: means != sums / counts")
        assert np.all(got_s[counts == 0] == 0.0), f"{tag}: sums of empty clusters"
        used = counts > 0
        if means == "fixed":
            assert float(x.min()) >= 0.0
            ref_s, ref_c = res[2], res[3]
            np.testing.assert_array_equal(ref_c, counts)
            ref_m = ref_s / np.maximum(ref_c, 1)[:, None]
            tol, fixed = fixed_point_tolerance(w, n, counts, ref_m)
            assert fixed <= 1e-8 * float(w.abs().max()), f"{tag}: bound {fixed:.3g} no tighter than the old 1e-6 relative"
            err = np.abs(got_m - ref_m)
            worst = np.unravel_index(np.argmax(np.where(used[:, None], err / tol, 0.0)), err.shape)
            assert np.all(err[used] <= tol[used]), (f"{tag}: mean [{worst[0]}, {worst[1]}] off by {err[worst]:.3g} > {tol[worst]:.3g} "
                                                    f"(fixed-point term {fixed:.3g})")
        else:
            exact = fr.exact_cluster_sums(x, labels, k).cpu().numpy()
            ulps = np.abs(got_s - exact) / np.spacing(np.abs(exact))
            assert np.all(got_s[exact == 0] == 0.0) and float(ulps[exact != 0].max(initial=0.0)) <= 4.0, \
                f"{tag}: sums {float(ulps[exact != 0].max(initial=0.0)):.1f} ulp from the exact sums"
        del lm, ws
    print(f"\nAUDIT {tag}: {n} rows, last_exact_rows {ler} ({ler / max(n, 1):.4%}), {time.time() - t0:.1f} s")
    return lab


# ---- (a) all-rows audit ---------------------------------------------------------------------------------------------------

def test_all_rows_cfg2(gpu):
    """cfg2: 10 x 1024^2 x 22 f32 (bench.py's rows), K = 100: trained, data rows, node pairs 1e-2 apart, collapsed W_1; the
    long-list kernel and the one-pass mean table on each."""
    x = fr.fov_rows(10, MPX, 22, 1000, gpu)
    sub = x[::10].contiguous()
    w = fr.trained_codebook(sub, 10, 10)
    books = {"trained": w, "data rows": fr.data_row_codebook(x, 100), "pairs 1e-2 apart": fr.near_pair_codebook(w),
             "collapsed W_1": fr.collapsed_codebook(sub, 10, 10)}
    del sub
    for name, wb in books.items():
        _audit(f"cfg2 / {name}", x, wb, screen=True, means="fixed")


def test_all_rows_cfg3_share(gpu):
    """cfg3's per-GPU share: 25 x 1024^2 x 22 f32 (26.2 M rows), the codebook trained on its 10 % subset."""
    x = fr.fov_rows(25, MPX, 22, 1000, gpu)
    w = fr.trained_codebook(x[::10].contiguous(), 10, 10)
    _audit("cfg3 share / trained", x, w)


def test_all_rows_cfg4(gpu):
    """cfg4: 10^6 x 100 f32 Poisson cells (quantised values, duplicate rows, exact ties), trained on all rows, and data rows;
    the mean table's two-kernel route."""
    x = fr.cell_rows(1_000_000, 100, 2000, gpu)
    for name, wb in (("trained", fr.trained_codebook(x, 10, 10)), ("data rows", fr.data_row_codebook(x, 100))):
        _audit(f"cfg4 / {name}", x, wb, means="exact")


def test_all_rows_cfg5(gpu):
    """cfg5: 4 x 2048^2 x 40 f16 (16.8 M rows), K = 400: trained on the 10 % subset, and node pairs 1e-2 apart."""
    x = fr.fov_rows(4, 4 * MPX, 40, 1000, gpu, dtype=torch.float16)
    w = fr.trained_codebook(x[::10].contiguous(), 20, 20)
    for name, wb in (("trained", w), ("pairs 1e-2 apart", fr.near_pair_codebook(w))):
        _audit(f"cfg5 / {name}", x, wb, means="exact")


def test_all_rows_mibi_like(gpu):
    """10.5 M sparse MIBI-like rows x 22 f32 (1-3 non-zero channels, mostly exact duplicates), K = 100: trained on the 10 %
    subset, and data rows; the long-list kernel and the one-pass mean table on each."""
    x = fr.mibi_rows(10 * MPX, 22, 77, gpu)
    w = fr.trained_codebook(x[::10].contiguous(), 10, 10)
    for name, wb in (("trained", w), ("data rows", fr.data_row_codebook(x, 100))):
        _audit(f"MIBI-like / {name}", x, wb, screen=True, means="fixed")


# ---- (b) training step by step at full size -------------------------------------------------------------------------------

def _cfg3_subset(dev):
    x = fr.fov_rows(25, MPX, 22, 1000, dev)
    sub = x[::10].contiguous()
    del x
    return sub


@pytest.mark.parametrize("case", ["cfg3 subset", "cfg4", "cfg5 subset"])
def test_training_step_by_step_at_full_size(gpu, oracle, case):
    """One pass of the trainer's own schedule, one ``batch_train_steps`` call per step: for every step g, the GPU's W_g labels
    the step's rows on the host (oracle); the counts in ``ring[g % 3]`` equal the oracle's, and W_{g+1} equals
    ``orc_batch_update`` of W_g and the GPU's statistics of step g (each step checked on the GPU's own trajectory).
    Routes, as bench.py takes them: cfg3's 10 % subset the fused 10 x 10 step; cfg4 (all rows, c = 100) the wide one-launch
    and windowed steps; cfg5's subset (20 x 20, f16) the generic route on row views.

    Sums: binary64 additions of the rows in whatever order the workgroups deliver them.  Where every partial sum of a step
    fits 53 bits (``fr.sum_bits`` of the step's rows: cfg4's counts, cfg5's binary16 values) they are exact, so they equal
    ``orc_cluster_sums`` bit for bit, and one ``BatchSOMTrainer.train`` call from W_0 gives the step-by-step codebook bit
    for bit.  The synthetic binary32 FOVs need more (values down to 1e-9 next to sums of 1e3): a sum may then round
    differently from the oracle's sequential one, and each such sum must lie within the recursive-summation bound
    (m - 1) 2^-53 sum |x| of the correctly rounded exact sum (math.fsum), as the oracle's own does; the run-to-run
    comparison has no bit-level contract there."""
    t0 = time.time()
    if case == "cfg3 subset":
        x, grid, fused = _cfg3_subset(gpu), 10, True
    elif case == "cfg4":
        x, grid, fused = fr.cell_rows(1_000_000, 100, 2000, gpu), 10, False
    else:
        full = fr.fov_rows(4, 4 * MPX, 40, 1000, gpu, dtype=torch.float16)
        x, grid, fused = full[::10].contiguous(), 20, False
        del full
    n, c = x.shape
    xdim = ydim = grid
    k = xdim * ydim
    tr = BatchSOMTrainer(xdim, ydim, c, gpu)
    sch = tr.schedule
    assert sd.batch_train_fused_route(x, xdim, ydim, sch) == fused
    total = tr.batch_steps
    a_r, r_r = tr.alpha_range, tr.radius_range
    w0 = fr.first_codebook(x, k)
    st = sd.BatchTrainState(n, c, xdim, ydim, sch, gpu, dtype=x.dtype)
    st.wbuf[0].copy_(w0)
    x_host = x.cpu()
    w_prev = s_prev = cnt_prev = None
    inexact, all_exact, bits = 0, True, 0.0
    for g in range(total):
        sd.batch_train_steps(x, st, g, g + 1, total, a_r, r_r)
        w_g = st.wbuf[g % 2].cpu().numpy()
        if g > 0:
            thr, alpha = batch_schedule(sch.position(g - 1), sch.phases, a_r, r_r)
            np.testing.assert_allclose(w_g, oracle.batch_update(w_prev, xdim, ydim, s_prev, cnt_prev, thr, alpha), rtol=1e-12, atol=0,
                                       err_msg=f"{case}: codebook after step {g - 1}")
        rows_t = x_host[torch.from_numpy(sch.rows_of_step(n, g))]
        bits = max(bits, fr.sum_bits(rows_t))
        exact = fr.sum_bits(rows_t) <= 53
        all_exact &= exact
        rows = rows_t.to(torch.float64).numpy()
        lab, _ = fr.oracle_labels(w_g, torch.from_numpy(rows))
        s, cnt = oracle.cluster_sums(rows, lab, k)
        ring = st.ring[g % 3].cpu().numpy()
        np.testing.assert_array_equal(ring[k * c:], cnt.astype(np.float64), err_msg=f"{case}: counts of step {g}")
        got = ring[: k * c].reshape(k, c)
        if exact:
            np.testing.assert_array_equal(got, s, err_msg=f"{case}: sums of step {g} ({len(lab)} rows)")
        for b, j in np.argwhere(got != s):
            vals = rows[lab == b + 1, j]
            want = math.fsum(vals.tolist())
            bound = (vals.size - 1) * 2.0 ** -53 * float(np.abs(vals).sum())
            assert abs(got[b, j] - want) <= bound and abs(s[b, j] - want) <= bound, \
                f"{case}: sum [{b}, {j}] of step {g}: {got[b, j]!r} vs exact {want!r} (oracle {s[b, j]!r}, bound {bound:.3g})"
            inexact += 1
        w_prev, s_prev, cnt_prev = w_g, got.copy(), cnt
    wa = torch.empty((k, c), dtype=torch.float64, device=gpu)
    sd.batch_train_finish(st, total, total, a_r, r_r, wa)
    thr, alpha = batch_schedule(sch.position(total - 1), sch.phases, a_r, r_r)
    np.testing.assert_allclose(wa.cpu().numpy(), oracle.batch_update(w_prev, xdim, ydim, s_prev, cnt_prev, thr, alpha), rtol=1e-12,
                               atol=0, err_msg=f"{case}: last update")
    assert all_exact or case == "cfg3 subset", f"{case}: the sums of a step need {bits:.1f} bits"
    if all_exact:
        w = w0.clone()
        tr.train(x, w, num_passes=1)
        assert tr.schedule == sch
        assert torch.equal(w, wa), f"{case}: one train() call differs from the step-by-step run"
    print(f"\nTRAIN {case}: {n} rows x {c}, {total} steps, sums of up to {bits:.1f} bits, {inexact} sums rounded unlike the "
          f"oracle's, {time.time() - t0:.1f} s")


# ---- (c) the scratch-clean promise ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["assign_sums", "assign_means"])
def test_empty_call_after_a_failed_one_leaves_the_tables_right(gpu, entry):
    """A workspace in the state a failed call leaves (statistics region dirty, ``clean`` False), then an empty call, then a real
    one: the tables equal those of a fresh workspace.  The empty call must clear the region, or must not vouch for it."""
    n, c, k = 300_000, 22, 100
    x = synth.make_fov_torch(n, c, seed=1000, device=gpu)
    w = fr.data_row_codebook(x, k)

    def run(ws, rows):
        if entry == "assign_sums":
            return sd.assign_sums(rows, w, workspace=ws)
        lab = torch.empty(rows.shape[0], dtype=torch.int32, device=gpu)
        sums = torch.empty((k, c), dtype=torch.float64, device=gpu)
        cnt = torch.empty(k, dtype=torch.int64, device=gpu)
        sd.assign_means(rows, w, lab, sums, cnt, torch.empty((k, c), dtype=torch.float64, device=gpu), ws)
        return lab, sums, cnt

    l0, s0, c0 = run(sd.AssignSumsWorkspace(n, c, k, gpu), x)
    ws = sd.AssignSumsWorkspace(n, c, k, gpu)
    stats_end = ws.assign_offset - 256                  # [statistics | 256 bytes: ticket word] [assign workspace]
    ws.buf[:stats_end].view(torch.float64).fill_(1.0)
    ws.clean = False
    run(ws, x[:0])
    l1, s1, c1 = run(ws, x)
    assert torch.equal(l1, l0)
    assert torch.equal(c1, c0), f"counts off by {int((c1 - c0).abs().max())}: the dirty region was taken for clean"
    np.testing.assert_allclose(s1.cpu().numpy(), s0.cpu().numpy(), rtol=1e-13, atol=0)
    assert float(ws.buf[:stats_end].view(torch.float64).abs().max()) == 0.0, "statistics region left dirty"
