"""Randomised parity sweep of the six entries of K30 (csrc/pxsom_embed.hip: pxsom_pair_sqdist_f32, pxsom_column_moments,
pxsom_project_rows, pxsom_tsne_affinities, pxsom_tsne_step) against the numpy statement of tests/tsne_reference.py, by route class: case i of a generator takes
class i % R of a fixed tuple and draws the rest, so a default run (max(12, R) cases) visits every class.  Every output
-- d2, mean, cov, scores, P, beta, steps, y_out, update, gains, grad, error and the workspaces -- is a slice at a drawn element offset of a sentinel buffer whose rest must still hold the
sentinel afterwards; the entries are called as their som_device wrappers call them, through _capi, since the wrappers
allocate their outputs or their workspace.  ``PXSOM_FUZZ_CASES`` / ``PXSOM_FUZZ_SEED`` as in test_gpu_fuzz_preprocessing.py.  The generators
are device-free (tests/test_fuzz_generators.py checks them on CPU)."""
import numpy as np
import pytest

from tests import tsne_reference as ts
from tests.test_gpu_fuzz_images import _bytes_equal, _guard_intact, _sentinel, _view1d
from tests.test_gpu_fuzz_preprocessing import PXSOM_OK, SEED, case_count

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
kDistTile, kDistChunk, kMomentRows, kThreads = 16, 32, 256, 256      # pxsom_embed.hip

# ---- pxsom_pair_sqdist_f32 -------------------------------------------------------------------------------------------------
SQDIST_N = (1, 15, 16, 17, 33, "draw")
SQDIST_C = (1, 31, 32, 33, 64, 65, 1024)
SQDIST_VALUES = ("offset", "duplicates", "scale_1e-6", "scale_1e6", "integers")
# class j: n class j % 6, c class j % 7, value class j % 5, float32 for odd j: 42 classes meet every (n, c) pair, every
# (n, values) pair and every (c, values) pair, since 5, 6 and 7 are pairwise coprime
SQDIST_CLASSES = tuple((SQDIST_N[j % 6], SQDIST_C[j % 7], SQDIST_VALUES[j % 5], bool(j % 2)) for j in range(42))


def sqdist_cases(seed, count):
    """Cases of test_fuzz_pair_sqdist: offset columns (the differences cancel: 1e3 ... 1e6 plus unit noise), duplicated
    rows (d2 exactly 0 off the diagonal too), scales 1e-6 and 1e6, small integers (every sum exact)."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        ncls, c, vcls, f32 = cls = SQDIST_CLASSES[i % len(SQDIST_CLASSES)]
        n = int(rs.randint(34, 301)) if ncls == "draw" else int(ncls)
        if c == 1024:
            n = min(n, int(rs.randint(34, 80)))
        dt = np.float32 if f32 else np.float64
        x = rs.standard_normal((n, c))
        if vcls == "offset":
            x = x + 10.0 ** rs.uniform(3, 6, size=c)
        elif vcls == "duplicates":
            x[rs.randint(0, n, size=max(1, n // 3))] = x[rs.randint(0, n)]
        elif vcls == "scale_1e-6":
            x = x * 1e-6
        elif vcls == "scale_1e6":
            x = x * 1e6
        else:
            x = rs.randint(-40, 41, size=(n, c)).astype(np.float64)
        yield dict(i=i, cls=cls, x=np.ascontiguousarray(x.astype(dt)), off=int(rs.randint(0, 8)), tail=int(rs.randint(0, 9)))


def test_fuzz_pair_sqdist(gpu):
    """d2 bit-equal to ts.pair_sqdist_f32, inside a float32 sentinel buffer; duplicated rows are exactly 0 apart."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fill = _sentinel(np.float32)
    for case in sqdist_cases(SEED + 80, case_count(SQDIST_CLASSES)):
        x = case["x"]
        n, c = x.shape
        tag = "case %d: class=%s n=%d c=%d %s off=%d (PXSOM_FUZZ_SEED=%d)" % (case["i"], case["cls"], n, c, x.dtype, case["off"], SEED)
        xt = torch.from_numpy(x).to(gpu)
        buf, d2 = _view1d(gpu, np.full((n, n), fill), case["off"], case["tail"], fill)
        rc = lib.pxsom_pair_sqdist_f32(xt.data_ptr(), n, c, _capi.dtype_code(xt), d2.data_ptr(),
                                       _capi.stream_ptr())
        torch.cuda.synchronize()
        assert rc == PXSOM_OK, tag
        got, want = d2.cpu().numpy(), ts.pair_sqdist_f32(x)
        assert _bytes_equal(got, want), tag + ": %d of %d entries differ" % (int((got != want).sum()), got.size)
        if case["cls"][2] == "duplicates":
            same = (x[:, None, :] == x[None, :, :]).all(-1)
            assert (same.sum() > n or n == 1) and np.all(got[same] == 0), tag      # (one row has no other to equal)
        assert _guard_intact(buf.cpu().numpy(), slice(case["off"], case["off"] + n * n), fill), tag + ": d2 guard"


# ---- pxsom_column_moments / pxsom_project_rows -----------------------------------------------------------------------------
MOMENT_ROWS = (65535, 65536, 65537, "draw")
# class j: the row class j % 4, but 2^20 rows in the last; 2 columns, 3 for j = 4 ... 7; float32 when j + j // 4 is odd
MOMENT_CLASSES = tuple(((1 << 20) if j == 11 else MOMENT_ROWS[j % 4], 3 if 4 <= j < 8 else 2, bool((j + j // 4) % 2))
                       for j in range(12))


def moment_trips(n):
    """Trips of ``for (b = threadIdx.x; b < blocks; b += 256)`` in column_mean_kernel / column_cov_kernel."""
    blocks = (n + kMomentRows - 1) // kMomentRows
    return (blocks + kThreads - 1) // kThreads


def moment_cases(seed, count):
    """Cases of test_fuzz_moments_and_projection: n around the 65 536 rows that one trip of a workgroup's 256 threads
    covers, a draw up to 70 000, and the contract's 2^20 rows (16 trips, 32 KiB of dynamic LDS) once per run of the
    classes; the table is test_gpu_tsne.py's: falling spreads on offset columns."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        ncls, c, f32 = cls = MOMENT_CLASSES[i % len(MOMENT_CLASSES)]
        n = int(rs.randint(65538, 70001)) if ncls == "draw" else int(ncls)
        x = (rs.standard_normal((n, c)) * (3.0 * 0.6 ** np.arange(c)) + 2.0 * rs.standard_normal(c)).astype(
            np.float32 if f32 else np.float64)
        yield dict(i=i, cls=cls, x=x, trips=moment_trips(n), axes=rs.standard_normal((2, c)),
                   mean_off=int(rs.randint(0, 4)), cov_off=int(rs.randint(0, 4)), scores_off=int(rs.randint(0, 4)))


def test_fuzz_moments_and_projection(gpu):
    """Means and covariance within 4 n U of the sums of absolute terms (tests/test_gpu_tsne.py's bound), the covariance
    symmetric bit for bit, the projection within 4 (c + 2) U; mean, cov and scores inside sentinel buffers."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fill = _sentinel(np.float64)
    for case in moment_cases(SEED + 81, case_count(MOMENT_CLASSES)):
        x = case["x"]
        n, c = x.shape
        tag = "case %d: class=%s n=%d c=%d %s trips=%d (PXSOM_FUZZ_SEED=%d)" % (case["i"], case["cls"], n, c, x.dtype,
                                                                               case["trips"], SEED)
        xt = torch.from_numpy(x).to(gpu)
        code = _capi.dtype_code(xt)
        mbuf, mean = _view1d(gpu, np.full(c, fill), case["mean_off"], 3, fill)
        cbuf, cov = _view1d(gpu, np.full((c, c), fill), case["cov_off"], 3, fill)
        sbuf, scores = _view1d(gpu, np.full((n, 2), fill), case["scores_off"], 5, fill)
        rc = lib.pxsom_column_moments(xt.data_ptr(), n, c, code, mean.data_ptr(), cov.data_ptr(), _capi.stream_ptr())
        torch.cuda.synchronize()
        assert rc == PXSOM_OK, tag
        want_mean, want_cov, mean_abs, cov_abs = ts.column_moments(x)
        got_mean, got_cov = mean.cpu().numpy(), cov.cpu().numpy()
        assert np.all(np.abs(got_mean - want_mean) <= 4 * n * U * mean_abs), tag
        assert np.all(np.abs(got_cov - want_cov) <= 4 * n * U * cov_abs), tag
        assert np.array_equal(got_cov, got_cov.T), tag
        assert _guard_intact(mbuf.cpu().numpy(), slice(case["mean_off"], case["mean_off"] + c), fill), tag + ": mean guard"
        assert _guard_intact(cbuf.cpu().numpy(), slice(case["cov_off"], case["cov_off"] + c * c), fill), tag + ": cov guard"
        axes = torch.from_numpy(case["axes"]).to(gpu)
        mean_t = torch.from_numpy(want_mean).to(gpu)
        rc = lib.pxsom_project_rows(xt.data_ptr(), n, c, code, mean_t.data_ptr(), axes.data_ptr(), scores.data_ptr(),
                                    _capi.stream_ptr())
        torch.cuda.synchronize()
        assert rc == PXSOM_OK, tag
        d = x.astype(np.float64) - want_mean
        assert np.all(np.abs(scores.cpu().numpy() - d @ case["axes"].T) <= 4 * (c + 2) * U * (np.abs(d) @ np.abs(case["axes"]).T)), tag
        assert _guard_intact(sbuf.cpu().numpy(), slice(case["scores_off"], case["scores_off"] + 2 * n), fill), tag + ": scores guard"


# ---- pxsom_tsne_affinities ---------------------------------------------------------------------------------------------------
AFFINITY_DATA = ("blobs", "lattice", "outliers", "scale_1e-6_f32", "scale_1e6")
AFFINITY_ROWS = (2, 3, "around_32", "around_64", "around_512", "draw", "draw_small")
AFFINITY_PERPLEXITY = ("low", "draw", "high")
# class j: data class j % 5 and row class j % 7 (35 classes: every pair); the perplexity class j % 3
# meets every data class and every row class but 2, which takes perplexity 1.01 only.  Perplexity exactly 1.0 stays in
# tests/test_gpu_tsne.py: there the entropy difference of 2 or 3 rows is an exact zero by symmetry
AFFINITY_CLASSES = tuple((AFFINITY_DATA[j % 5], AFFINITY_ROWS[j % 7],
                          "low" if AFFINITY_ROWS[j % 7] == 2 else AFFINITY_PERPLEXITY[j % 3]) for j in range(35))
EXEMPT_SHARE = 0.01


def affinity_cases(seed, count):
    """Cases of test_fuzz_affinities: blobs; an integer lattice with duplicated rows; blobs with a sixteenth of the rows
    moved out 1e4-fold; blobs scaled by 1e-6 in float32; by 1e6.  Perplexity 1.01, 0.98 (n - 1) or a draw between them.
    d32 is the statement's float32 matrix of squared distances."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        data, rows, pcls = cls = AFFINITY_CLASSES[i % len(AFFINITY_CLASSES)]
        n = {"around_32": int(rs.choice([31, 32, 33])), "around_64": int(rs.choice([63, 64, 65])),
             "around_512": int(rs.choice([511, 512, 513])), "draw": int(rs.randint(66, 601)),
             "draw_small": int(rs.randint(4, 31))}.get(rows, rows)
        c = int(rs.randint(2, 8))
        x = ts.blobs(n, c, 3, int(rs.randint(0, 2 ** 31 - 1)))[0]
        if data == "lattice":
            x = rs.randint(0, 6, size=(n, c)).astype(np.float64)
            if n > 3:
                x[rs.randint(0, n, size=max(1, n // 8))] = x[rs.randint(0, n)]
        elif data == "outliers":
            x[rs.choice(n, max(1, n // 16), replace=False)] *= 1e4
        elif data == "scale_1e-6_f32":
            x = (x * 1e-6).astype(np.float32)
        elif data == "scale_1e6":
            x = x * 1e6
        top = 0.98 * (n - 1)
        perplexity = 1.01 if pcls == "low" or top <= 1.01 else top if pcls == "high" else float(rs.uniform(1.01, top))
        yield dict(i=i, cls=cls, x=x, d32=ts.pair_sqdist_f32(x), perplexity=perplexity, p_off=int(rs.randint(0, 4)),
                   beta_off=int(rs.randint(0, 4)), steps_off=int(rs.randint(0, 4)), ws_off=2 * int(rs.randint(0, 4)))


def test_fuzz_affinities(gpu):
    """pxsom_tsne_affinities against ts.conditional_p.  A row whose margin (ts.conditional_p) is above 1 must have the
    statement's beta and steps bit for bit and its conditional row within (n + 16) 2 U; a row with margin <= 1 may have
    taken another path and must then satisfy the statement's stopping rule; at most 1 % of a case's rows may be such rows.
    The joint P is compared from the device's own conditional P.  P, beta, steps and a workspace of exactly
    pxsom_tsne_workspace_bytes(n) lie inside sentinel buffers, the workspace at a multiple of 16 bytes."""
    import torch
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    fd, fi = _sentinel(np.float64), _sentinel(np.int32)
    tol = float(np.float32(1e-5))
    for case in affinity_cases(SEED + 82, case_count(AFFINITY_CLASSES)):
        d32, perp = case["d32"], case["perplexity"]
        n = d32.shape[0]
        tag = "case %d: class=%s n=%d perplexity=%r offsets P %d beta %d steps %d workspace %d (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], case["cls"], n, perp, case["p_off"], case["beta_off"], case["steps_off"], case["ws_off"], SEED)
        cond, beta, steps, margins = ts.conditional_p(d32, perp, margin=True)
        dt = torch.from_numpy(d32).to(gpu)
        wsb = lib.pxsom_tsne_workspace_bytes(n)
        assert wsb >= (3 * n + 2) * 8 and wsb % 8 == 0, tag
        got = {}
        for joint in (0, 1):
            pbuf, P = _view1d(gpu, np.full((n, n), fd), case["p_off"], 5, fd)
            bbuf, bt = _view1d(gpu, np.full(n, fd), case["beta_off"], 3, fd)
            sbuf, st = _view1d(gpu, np.full(n, fi), case["steps_off"], 3, fi)
            wbuf, ws = _view1d(gpu, np.full(wsb // 8, fd), case["ws_off"], 4, fd)
            assert ws.data_ptr() % 16 == 0, tag
            rc = lib.pxsom_tsne_affinities(dt.data_ptr(), n, float(perp), joint, bt.data_ptr(), st.data_ptr(), P.data_ptr(),
                                           ws.data_ptr(), wsb, _capi.stream_ptr())
            torch.cuda.synchronize()
            assert rc == PXSOM_OK, tag
            got[joint] = (P.cpu().numpy(), bt.cpu().numpy(), st.cpu().numpy())
            t = tag + " joint=%d" % joint
            assert _guard_intact(pbuf.cpu().numpy(), slice(case["p_off"], case["p_off"] + n * n), fd), t + ": P guard"
            assert _guard_intact(bbuf.cpu().numpy(), slice(case["beta_off"], case["beta_off"] + n), fd), t + ": beta guard"
            assert _guard_intact(sbuf.cpu().numpy(), slice(case["steps_off"], case["steps_off"] + n), fi), t + ": steps guard"
            assert _guard_intact(wbuf.cpu().numpy(), slice(case["ws_off"], case["ws_off"] + wsb // 8), fd), t + ": workspace guard"
        got_cond, got_beta, got_steps = got[0]
        sure = margins > 1
        exempt = np.flatnonzero(~sure)
        assert exempt.size <= EXEMPT_SHARE * n, tag + ": %d of %d rows have margin <= 1" % (exempt.size, n)
        bad = np.flatnonzero(sure & ((got_beta != beta) | (got_steps != steps)))
        assert bad.size == 0, tag + ": rows %s (margins %s): beta %r steps %r, statement %r %r" % (
            bad[:4], margins[bad[:4]], got_beta[bad[:4]], got_steps[bad[:4]], beta[bad[:4]], steps[bad[:4]])
        assert np.all(np.diag(got_cond) == 0), tag
        assert np.all(np.abs(got_cond - cond)[sure] <= (n + 16) * 2 * U * cond[sure]), tag
        for r in exempt:
            assert got_steps[r] == 99 or abs(ts.row_entropy_diff(d32[r], r, got_beta[r], perp)) <= tol + 1e-9, tag + ": row %d" % r
        got_joint = got[1][0]
        assert np.array_equal(got[1][1], got_beta) and np.array_equal(got[1][2], got_steps), tag
        want = ts.joint_p(got_cond)
        off = ~np.eye(n, dtype=bool)
        assert np.all(np.abs(got_joint - want)[off] <= (n * n + 8) * U * want[off]), tag
        assert np.all(np.diag(got_joint) == ts.EPS) and np.array_equal(got_joint, got_joint.T), tag


# ---- pxsom_tsne_step -----------------------------------------------------------------------------------------------------------
STEP_SCALES = (1e-4, 5.0, 200.0)
STEP_P = ("statement", "uniform", "eps_rows")
# class j: n even for even j, P 16-byte aligned for (j // 2) % 2 == 0 (the four pairs at j % 4); the scale j % 3 and the kind
# of P (j // 3) % 3 (the nine pairs at j % 9; 36 classes meet every pair of the two); want_error and grad by other periods
STEP_CLASSES = tuple(dict(j=j, even=j % 2 == 0, aligned=(j // 2) % 2 == 0, scale=STEP_SCALES[j % 3], p=STEP_P[(j // 3) % 3],
                          want_error=(j // 4 + j // 12) % 2 == 0, grad=(j // 4 + j // 8) % 3 != 0,
                          e=12.0 if (j // 6) % 2 == 0 else 1.0) for j in range(36))


def step_route(n, p_off):
    """VEC of pxsom_tsne_step: 16-byte loads of P when n is even and P (``p_off`` doubles into a 16-byte aligned buffer)
    is 16-byte aligned."""
    return n % 2 == 0 and p_off % 2 == 0


def step_cases(seed, count):
    """Cases of test_fuzz_step: P the statement's joint affinities of blobs, a uniform matrix, or the statement's with a
    few rows and columns of eps (outliers); the embedding ts.step_embedding's at the three scales."""
    rs = np.random.RandomState(seed)
    for i in range(count):
        cls = STEP_CLASSES[i % len(STEP_CLASSES)]
        n = int(rs.choice([2, 4, 6, 16, 64, 66, 128, 130, 2 * int(rs.randint(8, 120))]))
        n += 0 if cls["even"] else 1
        if cls["p"] == "uniform":
            P = np.full((n, n), 1.0 / (n * (n - 1)))
        else:
            d32 = ts.pair_sqdist_f32(ts.blobs(n, 4, 3, int(rs.randint(0, 2 ** 31 - 1)))[0])
            P = ts.joint_p(ts.conditional_p(d32, 1.01 if n < 5 else min(30.0, (n - 1) / 3.0))[0])
            if cls["p"] == "eps_rows":
                out = rs.choice(n, max(1, n // 10), replace=False)
                P[out, :] = ts.EPS
                P[:, out] = ts.EPS
        np.fill_diagonal(P, ts.EPS)
        seed_y = int(rs.randint(0, 2 ** 31 - 1))
        Y = ts.step_embedding(n, cls["scale"], seed_y)
        upd = 0.01 * cls["scale"] * rs.standard_normal((n, 2))
        gains = rs.uniform(0.005, 2.0, size=(n, 2))
        p_off = 2 * int(rs.randint(0, 2)) + (0 if cls["aligned"] else 1)
        yield dict(i=i, cls=cls, P=P, Y=Y, upd=upd, gains=gains, p_off=p_off, route=step_route(n, p_off),
                   offs=[int(v) for v in rs.randint(0, 4, size=5)], ws_off=2 * int(rs.randint(0, 4)))


def _launch_step(gpu, lib, case, grad_given, guards):
    """One pxsom_tsne_step of the case -> (y_out, update, gains, grad or None, error or None) as numpy, after the guard
    checks when ``guards``."""
    import torch
    from ark_analysis_amd import _capi
    cls, n = case["cls"], len(case["Y"])
    fd = _sentinel(np.float64)
    offs = case["offs"] if guards else [0] * 5
    pbuf, P = _view1d(gpu, case["P"], case["p_off"], 2, fd)
    assert pbuf.data_ptr() % 16 == 0 and (P.data_ptr() % 16 == 0) == (case["p_off"] % 2 == 0)
    y_in = torch.from_numpy(case["Y"]).to(gpu)
    views = [_view1d(gpu, a, o, 3, fd) for a, o in zip((np.full((n, 2), fd), case["upd"], case["gains"], np.full((n, 2), fd),
                                                       np.full(2, fd)), offs)]
    (_, y_out), (_, upd), (_, gains), (_, grad), (_, err) = views
    wsb = lib.pxsom_tsne_workspace_bytes(n)
    wbuf, ws = _view1d(gpu, np.full(wsb // 8, fd), case["ws_off"], 4, fd)
    rc = lib.pxsom_tsne_step(P.data_ptr(), n, y_in.data_ptr(), y_out.data_ptr(), upd.data_ptr(), gains.data_ptr(), cls["e"], 0.5,
                             max(n / 48.0, 50.0), ts.MIN_GAIN, int(cls["want_error"]),
                             err.data_ptr() if cls["want_error"] else None, grad.data_ptr() if grad_given else None,
                             ws.data_ptr(), wsb, _capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == PXSOM_OK
    assert np.array_equal(y_in.cpu().numpy(), case["Y"])
    if guards:
        sizes = (2 * n, 2 * n, 2 * n, 2 * n if grad_given else 0, 2 if cls["want_error"] else 0)
        for name, (buf, _), o, size in zip(("y_out", "update", "gains", "grad", "error"), views, offs, sizes):
            assert _guard_intact(buf.cpu().numpy(), slice(o, o + size), fd), name + " guard"
        assert _guard_intact(wbuf.cpu().numpy(), slice(case["ws_off"], case["ws_off"] + wsb // 8), fd), "workspace guard"
    return (y_out.cpu().numpy(), upd.cpu().numpy(), gains.cpu().numpy(), grad.cpu().numpy() if grad_given else None,
            err.cpu().numpy() if cls["want_error"] else None)


def test_fuzz_step(gpu):
    """pxsom_tsne_step with tests/test_gpu_tsne.py test_one_step's tolerances: the gradient within 4 (32 n U A + n^2 U B),
    the KL divergence within (n^2 + 64) U of its absolute sum plus (2 n + 16) U e sum P, the elementwise update exact on the
    gradient the device returned.  The second KL term is what test_one_step's cases never needed: every term
    pe log(pe / q) carries the relative error of q in its logarithm, an absolute pe times that error, and q = n_ij / Z
    carries Z's -- a row sum of n terms folded over n rows, 2 n U, with the division, the reciprocal and the logarithm's
    own roundings in the 16.  With the statement's affinities the terms are large and the first part covers it; with a
    uniform P on a tiny embedding q equals p to eight digits, the terms cancel to 1e-8 of sum pe, and only this part is
    left.  Without ``grad`` the outputs must be the bits of the same launch with it.  y_out, update, gains, grad,
    error and the exact workspace lie inside sentinel buffers; a null grad or error leaves its buffer untouched."""
    from ark_analysis_amd import _capi
    lib = _capi.lib()
    for case in step_cases(SEED + 83, case_count(STEP_CLASSES)):
        cls, P, Y = case["cls"], case["P"], case["Y"]
        n = len(Y)
        tag = "case %d: class=%s n=%d VEC=%s p_off=%d offsets %s workspace %d (PXSOM_FUZZ_SEED=%d)" % (
            case["i"], cls, n, case["route"], case["p_off"], case["offs"], case["ws_off"], SEED)
        try:
            y_out, u, g, grad, err = _launch_step(gpu, lib, case, cls["grad"], True)
        except AssertionError as exc:
            raise AssertionError(tag + ": " + str(exc))
        if grad is None:                       # the same launch with the gradient written out: the same bits
            y2, u2, g2, grad, err2 = _launch_step(gpu, lib, case, True, False)
            assert np.array_equal(y_out, y2) and np.array_equal(u, u2) and np.array_equal(g, g2), tag
            assert err is None or np.array_equal(err, err2), tag
        o = ts.objective(Y, P, cls["e"])
        bound = 4 * (32 * n * U * o["A"] + n * n * U * o["B"])
        assert np.all(np.abs(grad - o["grad"]) <= bound), tag + ": gradient error / bound %.3g" % np.max(
            np.abs(grad - o["grad"]) / np.maximum(bound, 1e-300))
        want_y, want_u, want_g, scaled = ts.update(grad, Y, case["upd"], case["gains"], 0.5, max(n / 48.0, 50.0))
        assert np.array_equal(y_out, want_y) and np.array_equal(u, want_u) and np.array_equal(g, want_g), tag
        if err is not None:
            pe_sum = cls["e"] * P[~np.eye(n, dtype=bool)].sum()
            assert abs(err[0] - o["kl"]) <= (n * n + 64) * U * o["kl_abs"] + (2 * n + 16) * U * pe_sum, tag + ": KL %r, statement %r" % (
                err[0], o["kl"])
            assert abs(err[1] - np.linalg.norm(scaled)) <= (2 * n + 8) * U * np.linalg.norm(scaled), tag
