"""K30 on the device: the column moments, PCA scores, squared distances, affinities and descent step of csrc/pxsom_embed.hip
against the numpy statement (tests/tsne_reference.py) and scikit-learn.  Every tolerance is derived from the length of the
sums it covers (U = 2^-53); none is tuned.

Sizes: 2 and 3 rows; one below, at and one above the step kernels' row block (4), the distance tile (16), the tile of the
symmetrisation (32), the wave (64), the workgroup and the row block of the moments (256) and the 512 elements a workgroup
takes from a row per trip; columns below, at and above the 32-channel chunk of the distance kernel and the 64 lanes of a
wave."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import tsne_reference as ts

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
ROWS = (2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513)
COLUMNS = (1, 2, 3, 22, 31, 32, 33, 64, 65, 100)
STEP_ROWS = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513)
KL_M = 0.102          # twice the largest spread among reference runs on seeds 0-5 (DESIGN.md "K30")
END_TO_END_SEED = 0


def _up(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _table(n, c, seed, dtype):
    """An anisotropic table with offset columns: the spreads fall by 0.6 per column down to 0.14, which keeps the three
    leading variances apart and every spread far above the rounding error of its column's mean."""
    r = np.random.RandomState(seed)
    return (r.standard_normal((n, c)) * (3.0 * 0.6 ** np.minimum(np.arange(c), 6)) + 2.0 * r.standard_normal(c)).astype(dtype)


def _perplexity(n):
    return 1.0 if n == 2 else max(1.5, min(30.0, (n - 1) / 3.0))


@functools.lru_cache(maxsize=None)
def _statement_affinities(n):
    x = ts.blobs(n, 5, 3, n)[0]
    d32 = ts.pair_sqdist_f32(x)
    cond, beta, steps = ts.conditional_p(d32, _perplexity(n))
    return x, d32, cond, beta, steps, ts.joint_p(cond)


# ---- distances, moments, PCA -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_pair_sqdist_equals_the_statement(gpu, n):
    from ark_analysis_amd import som_device as sd
    for c in COLUMNS:
        for dtype in (np.float32, np.float64):
            x = _table(n, c, 100 * n + c, dtype)
            got = sd.pair_sqdist_f32(_up(x, gpu)).cpu().numpy()
            assert got.dtype == np.float32 and np.array_equal(got, ts.pair_sqdist_f32(x)), (n, c, dtype)
            assert np.all(np.diag(got) == 0)


@pytest.mark.parametrize("n", ROWS)
def test_column_moments_and_projection(gpu, n):
    from ark_analysis_amd import som_device as sd
    for c in COLUMNS[1:]:
        for dtype in (np.float32, np.float64):
            x = _table(n, c, 7 * n + c, dtype)
            mean, cov, mean_abs, cov_abs = ts.column_moments(x)
            got_mean, got_cov = (t.cpu().numpy() for t in sd.column_moments(_up(x, gpu)))
            assert np.all(np.abs(got_mean - mean) <= 4 * n * U * mean_abs), (n, c, dtype)
            assert np.all(np.abs(got_cov - cov) <= 4 * n * U * cov_abs), (n, c, dtype)
            assert np.array_equal(got_cov, got_cov.T)
            axes = np.random.RandomState(c).standard_normal((2, c))
            got = sd.project_rows(_up(x, gpu), _up(mean, gpu), _up(axes, gpu)).cpu().numpy()
            d = x.astype(np.float64) - mean
            assert np.all(np.abs(got - d @ axes.T) <= 4 * (c + 2) * U * (np.abs(d) @ np.abs(axes).T)), (n, c, dtype)


# Every row count, 2 and 3 included.  With fewer than four rows sklearn has fewer than three explained variances; the guard
# then takes the gaps among those it has (a zero variance after a positive one is a gap of 1).
@pytest.mark.parametrize("n", ROWS)
def test_pca_scores_equal_sklearn(gpu, n):
    from sklearn.decomposition import PCA
    from ark_analysis_amd import som_device as sd
    for c in COLUMNS[1:]:
        for dtype in (np.float32, np.float64):
            x = _table(n, c, 3 * n + c, dtype)
            x64 = x.astype(np.float64)
            est = PCA()
            want = est.fit_transform(x64)[:, :2]
            ev = est.explained_variance_[:3]
            g = float(np.min((ev[:-1] - ev[1:]) / ev[:-1]))
            assert g >= 0.1, (n, c, g)                               # on sklearn's result alone
            rownorm = np.linalg.norm(x64 - x64.mean(0), axis=1).max()
            got = sd.pca_scores(_up(x, gpu)).cpu().numpy()
            assert np.abs(got - want).max() <= 64 * n * U * rownorm / g, (n, c, dtype)


# ---- affinities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_affinities(gpu, n):
    from ark_analysis_amd import som_device as sd
    x, d32, cond, beta, steps, joint = _statement_affinities(n)
    perp = _perplexity(n)
    d2 = sd.pair_sqdist_f32(_up(x, gpu))
    assert np.array_equal(d2.cpu().numpy(), d32)
    got_cond, got_beta, got_steps = (t.cpu().numpy() for t in sd.tsne_affinities(d2, perp, joint=False))
    same = got_beta == beta
    print("n=%d: %d of %d rows took another search path" % (n, int((~same).sum()), n))
    assert (~same).sum() <= 0.01 * n
    assert np.array_equal(got_steps[same], steps[same])
    assert np.all(np.diag(got_cond) == 0)
    assert np.all(np.abs(got_cond - cond)[same] <= (n + 16) * 2 * U * cond[same])
    for i in np.nonzero(~same)[0]:
        # the device stopped (or ran out of steps) elsewhere: its beta must satisfy the statement's stopping rule
        assert got_steps[i] == 99 or abs(ts.row_entropy_diff(d32[i], i, got_beta[i], perp)) <= float(np.float32(1e-5)) + 1e-9
    # the joint P from the device's own conditional P
    got_joint = sd.tsne_affinities(d2, perp)[0].cpu().numpy()
    want = ts.joint_p(got_cond)
    off = ~np.eye(n, dtype=bool)
    assert np.all(np.abs(got_joint - want)[off] <= (n * n + 8) * U * want[off])
    assert np.all(np.diag(got_joint) == ts.EPS) and np.array_equal(got_joint, got_joint.T)


def test_a_search_that_runs_out_of_steps(gpu):
    """Perplexity 1 asks for zero entropy, which four points reach only in the limit: rows stop at the 100th evaluation."""
    from ark_analysis_amd import som_device as sd
    d32 = ts.pair_sqdist_f32(ts.blobs(4, 5, 3, 4)[0])
    cond, beta, steps = ts.conditional_p(d32, 1.0)
    assert steps.max() == 99
    got_cond, got_beta, got_steps = (t.cpu().numpy() for t in sd.tsne_affinities(_up(d32, gpu), 1.0, joint=False))
    assert np.array_equal(got_steps, steps)
    same = got_beta == beta
    assert same[steps < 99].all() and np.all(np.abs(got_cond - cond)[same] <= (4 + 16) * 2 * U * cond[same])
    # the row that ran out of steps ends where exp underflows: its sum is zero, replaced by 1e-8, and the row stays empty
    assert np.array_equal(cond.sum(axis=1) == 0, steps == 99)
    assert np.allclose(got_cond.sum(axis=1), cond.sum(axis=1), rtol=1e-14, atol=0)


# ---- one step -----------------------------------------------------------------------------------------------------------
def _step_state(n, scale, seed):
    r = np.random.RandomState(seed)
    Y = ts.step_embedding(n, scale, seed)
    upd = 0.01 * scale * r.standard_normal((n, 2))
    gains = r.uniform(0.005, 2.0, size=(n, 2))
    return Y, upd, gains


def _device_step(gpu, P, Y, upd, gains, e, momentum, lr, want_error=True, shift=0):
    """One pxsom_tsne_step -> (y_out, update, gains, grad, error); with ``shift`` P starts 8 bytes off a 16-byte boundary."""
    from ark_analysis_amd import som_device as sd
    n = len(Y)
    Pd = _up(P, gpu)
    if shift:
        flat = torch.empty(n * n + 2, dtype=torch.float64, device=gpu)
        off = 1 if flat.data_ptr() % 16 == 0 else 2
        flat[off:off + n * n] = Pd.reshape(-1)
        Pd = flat[off:off + n * n].view(n, n)
        assert Pd.data_ptr() % 16 == 8
    y_in, u, g = _up(Y, gpu), _up(upd, gpu), _up(gains, gpu)
    y_out, grad = torch.full_like(y_in, float("nan")), torch.full_like(y_in, float("nan"))
    err = torch.full((2,), float("nan"), dtype=torch.float64, device=gpu) if want_error else None
    sd.tsne_step(Pd, y_in, y_out, u, g, e, momentum, lr, error=err, grad=grad)
    assert np.array_equal(y_in.cpu().numpy(), Y)
    return (y_out.cpu().numpy(), u.cpu().numpy(), g.cpu().numpy(), grad.cpu().numpy(),
            err.cpu().numpy() if want_error else None)


@pytest.mark.parametrize("e", (12.0, 1.0))
@pytest.mark.parametrize("scale", (1e-4, 5.0, 200.0))
@pytest.mark.parametrize("n", STEP_ROWS)
def test_one_step(gpu, n, scale, e):
    P = _statement_affinities(n)[5]
    Y, upd, gains = _step_state(n, scale, 11 * n + int(e))
    momentum, lr = 0.5, max(n / 48.0, 50.0)
    o = ts.objective(Y, P, e)
    if scale == 200.0:
        # the clamp on q is active, asserted on the statement.  Below 16 rows it cannot be reached: Z is then a sum of so few
        # terms that the smallest n_ij / Z stays above eps however far a row is moved out (with 2 rows q = 1 / 2 exactly)
        assert (o["q"][~np.eye(n, dtype=bool)] == ts.EPS).any() == (n >= 16)
    y_out, u, g, grad, err = _device_step(gpu, P, Y, upd, gains, e, momentum, lr)
    tol = 4 * (32 * n * U * o["A"] + n * n * U * o["B"])
    excess = np.abs(grad - o["grad"]) - tol
    print("n=%d scale=%g e=%g: gradient error / tolerance %.3g, KL error / tolerance %.3g" % (
        n, scale, e, np.max(np.abs(grad - o["grad"]) / np.maximum(tol, 1e-300)),
        abs(err[0] - o["kl"]) / max((n * n + 64) * U * o["kl_abs"], 1e-300)))
    assert np.all(excess <= 0)
    assert abs(err[0] - o["kl"]) <= (n * n + 64) * U * o["kl_abs"]
    # the elementwise update has no sums in it: exact, on the gradient the device returned
    want_y, want_u, want_g, scaled = ts.update(grad, Y, upd, gains, momentum, lr)
    assert np.array_equal(y_out, want_y) and np.array_equal(u, want_u) and np.array_equal(g, want_g)
    assert (upd * grad < 0).any() or n < 4
    assert abs(err[1] - np.linalg.norm(scaled)) <= (2 * n + 8) * U * np.linalg.norm(scaled)
    # the launch without the KL terms, and the one that cannot use 16-byte loads, give the same bits
    for kwargs in ({"want_error": False}, {"shift": 1}):
        other = _device_step(gpu, P, Y, upd, gains, e, momentum, lr, **kwargs)
        for a, b in zip((y_out, u, g, grad), other[:4]):
            assert np.array_equal(a, b), kwargs
        if other[4] is not None:
            assert np.array_equal(other[4], err)


def test_ten_iterations_stay_with_the_statement(gpu):
    from ark_analysis_amd import som_device as sd
    n = 257
    P = _statement_affinities(n)[5]
    Y0 = 1e-4 * np.random.RandomState(21).standard_normal((n, 2))
    lr = sd.tsne_learning_rate(n)
    want, margin = ts.steps(P, Y0, 10)
    signs = np.where(np.random.RandomState(22).rand(n, 2) < 0.5, -1.0, 1.0)
    nudged, _ = ts.steps(P, Y0 * (1.0 + 2.0 ** -40 * signs), 10)
    assert margin >= 1e-10                       # no gain decision of the statement sits on a rounding error
    Pd, y, y_next = _up(P, gpu), _up(Y0, gpu), torch.empty((n, 2), dtype=torch.float64, device=gpu)
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    for _ in range(10):
        sd.tsne_step(Pd, y, y_next, update, gains, 12.0, 0.5, lr)
        y, y_next = y_next, y
    spread = np.abs(nudged - want).max()
    got = np.abs(y.cpu().numpy() - want).max()
    print("ten iterations: device %.3g, statement against its nudged self %.3g, margin %.3g" % (got, spread, margin))
    assert got <= 4 * spread


def test_two_runs_give_the_same_bits(gpu):
    from ark_analysis_amd import som_device as sd
    n = 257
    P = _up(_statement_affinities(n)[5], gpu)
    y0 = _up(1e-4 * np.random.RandomState(31).standard_normal((n, 2)), gpu)
    a = sd.tsne(P, y0)
    b = sd.tsne(P, y0)
    assert a.n_iter == b.n_iter == 999 and a.kl_divergence == b.kl_divergence
    assert np.isfinite(a.embedding.cpu().numpy()).all()
    assert np.array_equal(a.embedding.cpu().numpy(), b.embedding.cpu().numpy())
    # the affinities too
    x = _up(_statement_affinities(n)[0], gpu)
    p1, p2 = (sd.tsne_affinities(sd.pair_sqdist_f32(x), 30.0)[0].cpu().numpy() for _ in range(2))
    assert np.array_equal(p1, p2)


# ---- end to end --------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_sklearn(gpu, tmp_path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import pandas as pd
    from ark_analysis_amd.analysis import dimensionality_reduction as dr
    with np.load(os.path.join(HERE, "golden", "g33_tsne.npz")) as g:
        kl_sklearn = float(g["kl_sklearn"][list(g["kl_seeds"]).index(END_TO_END_SEED)])
    x, lab, y0 = ts.end_to_end_case(END_TO_END_SEED)
    emb = dr.reduce_dimensions(x, "tSNE", perplexity=30.0, init=y0)
    print("end to end: KL %.6f, sklearn's %.6f, ratio - 1 = %.4f, purity %.3f, n_iter %d" % (
        emb.kl_divergence_, kl_sklearn, emb.kl_divergence_ / kl_sklearn - 1, ts.purity(np.asarray(emb), lab), emb.n_iter_))
    assert emb.shape == (300, 2) and emb.n_iter_ == 999
    assert ts.purity(np.asarray(emb), lab) == 1.0
    assert abs(emb.kl_divergence_ / kl_sklearn - 1) <= KL_M
    # through the visualiser (PCA initialisation, so only the structure is compared), and its PCA plot
    df = pd.DataFrame(x, columns=["m%d" % i for i in range(10)])
    df["cell_type"] = np.array(["a", "b", "c"])[lab]
    shown = dr.visualize_dimensionality_reduction(df, list(df.columns[:10]), "cell_type", algorithm="tSNE", dpi=40,
                                                  save_dir=str(tmp_path))
    assert ts.purity(np.asarray(shown), lab) == 1.0 and shown.n_iter_ == 999 and 0 < shown.kl_divergence_ < 10
    pcs = dr.visualize_dimensionality_reduction(df, list(df.columns[:10]), "cell_type", algorithm="PCA", dpi=40,
                                                save_dir=str(tmp_path))
    assert pcs.shape == (300, 2) and pcs.kl_divergence_ is None
    plt.close("all")
    for name in ("tSNEVisualization.png", "PCAVisualization.png"):
        with open(tmp_path / name, "rb") as f:
            assert f.read(8) == b"\x89PNG\r\n\x1a\n"


def test_init_choices(gpu):
    from ark_analysis_amd.analysis import dimensionality_reduction as dr
    x, lab = ts.blobs(90, 6, 3, 5)
    for kwargs in ({"init": "pca"}, {"init": "random", "random_state": 3}):
        a = dr.reduce_dimensions(x.astype(np.float32), "tSNE", perplexity=10.0, max_iter=300, **kwargs)
        b = dr.reduce_dimensions(x.astype(np.float32), "tSNE", perplexity=10.0, max_iter=300, **kwargs)
        assert np.array_equal(a, b) and a.n_iter_ == 299 and ts.purity(np.asarray(a), lab) == 1.0, kwargs


# ---- the driver's stop rules ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ts.DESCENT_SCRIPTS))
def test_driver_stop_rules_follow_the_statement(gpu, monkeypatch, name):
    """som_device.tsne over a stub of tsne_step that copies y_in to y_out and, when asked for the error, writes the script's
    (KL, gradient norm): n_iter, the KL and the calls per phase equal ts.descend's on the same script (which
    tests/test_tsne.py pins to sklearn's TSNE._tsne), and the error is asked for on every 50th iteration and on the last
    of a phase, nowhere else."""
    from ark_analysis_amd import som_device as sd
    from ark_analysis_amd.som_device import embedding
    max_iter, window, kl, zero_grad, want_it, want_calls = ts.DESCENT_SCRIPTS[name]
    want_calls_seen = []

    def objective(Y, P, e):
        i = len(want_calls_seen)
        want_calls_seen.append(e)
        return {"kl": kl(i), "grad": np.zeros_like(Y) if i in zero_grad else np.full_like(Y, 1e-3)}
    monkeypatch.setattr(ts, "objective", objective)
    _, want_kl, it = ts.descend(None, np.zeros((8, 2)), max_iter=max_iter, n_iter_without_progress=window)
    assert it == want_it

    calls = []

    def stub(P, y_in, y_out, update, gains, exaggeration, momentum, learning_rate, min_gain=0.01, error=None, grad=None,
             workspace=None):
        i = len(calls)
        calls.append((exaggeration, momentum, error is not None))
        assert learning_rate == 50.0 and min_gain == 0.01 and grad is None and workspace is not None
        assert y_in.data_ptr() != y_out.data_ptr()
        # a phase starts from zero updates and unit gains, which the stub leaves as they are
        assert not bool(update.any()) and bool((gains == 1.0).all())
        y_out.copy_(y_in)
        if error is not None:
            error.copy_(torch.tensor([kl(i), 0.0 if i in zero_grad else 1.0], dtype=torch.float64))
    monkeypatch.setattr(embedding, "tsne_step", stub)
    y0 = _up(np.random.RandomState(1).standard_normal((8, 2)), gpu)
    res = sd.tsne(torch.zeros((8, 8), dtype=torch.float64, device=gpu), y0, max_iter=max_iter, n_iter_without_progress=window)
    assert res.n_iter == want_it and res.kl_divergence == want_kl
    assert [c[0] for c in calls] == want_calls_seen
    assert [c[:2] for c in calls] == [(12.0, 0.5)] * want_calls[0] + [(1.0, 0.8)] * want_calls[1]
    ends = [ts.EXPLORATION_ITER] * want_calls[0] + [max_iter] * want_calls[1]
    assert [c[2] for c in calls] == [ts.asks_error(i, end) for i, end in enumerate(ends)]
    assert torch.equal(res.embedding, y0) and res.embedding.data_ptr() != y0.data_ptr()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(gpu, monkeypatch):
    from ark_analysis_amd import som_device as sd
    from ark_analysis_amd.analysis import dimensionality_reduction as dr
    x = ts.blobs(40, 3, 2, 0)[0]
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        dr.reduce_dimensions(x, "tSNE", perplexity=40.0)
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        sd.tsne_embed(_up(x, gpu), perplexity=40.0)
    bad = x.copy()
    bad[7, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        dr.reduce_dimensions(bad, "tSNE", perplexity=5.0)
    with pytest.raises(ValueError, match="contiguous float32 or float64"):
        sd.pair_sqdist_f32(_up(x, gpu).to(torch.float16))
    with pytest.raises(ValueError, match="contiguous float32 or float64"):
        sd.column_moments(_up(x, gpu)[:, :2])
    with pytest.raises(ValueError, match="2 .. 1024 columns"):
        sd.column_moments(_up(x[:, :1], gpu))
    y = _up(np.zeros((40, 2)), gpu)
    with pytest.raises(ValueError, match="different buffers"):
        sd.tsne_step(_up(np.zeros((40, 40)), gpu), y, y, y.clone(), y.clone(), 1.0, 0.5, 50.0)
    # a table past the memory check: the free-memory query is swapped, nothing is allocated
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (12 * 39 * 39 + sd.tsne_workspace_bytes(39), 1 << 40))
    with pytest.raises(NotImplementedError, match="the largest table that fits has 39 rows"):
        dr.reduce_dimensions(x, "tSNE", perplexity=5.0)
    assert dr.reduce_dimensions(x[:39], "tSNE", perplexity=5.0, max_iter=250).shape == (39, 2)
