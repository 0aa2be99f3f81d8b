"""K30 on the CPU: the numpy statement (tests/tsne_reference.py) pinned to scikit-learn itself -- the perplexity search, the
joint P, the objective and gradient, ten descent iterations and the PCA scores -- then the public functions with the device
hook swapped for the statement, every refusal, the PNG files, the fixture and the ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
from scipy.spatial.distance import squareform
from sklearn.decomposition import PCA
from sklearn.manifold import _t_sne, _utils

from tests import tsne_reference as ts

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "g33_tsne.npz")
NEW_SYMBOLS = ("pxsom_tsne_workspace_bytes", "pxsom_column_moments", "pxsom_project_rows", "pxsom_pair_sqdist_f32",
               "pxsom_tsne_affinities", "pxsom_tsne_step")
U = 2.0 ** -53
CASES = ((96, 5, 2, 10.0, 0), (257, 10, 3, 30.0, 1), (130, 22, 4, 30.0, 2))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def affinities():
    """Per case: d32, sklearn's conditional P, the statement's (P, beta, steps)."""
    out = []
    for n, c, k, perp, seed in CASES:
        d32 = ts.pair_sqdist_f32(ts.blobs(n, c, k, seed)[0])
        out.append((d32, perp, _utils._binary_search_perplexity(d32, perp, 0), ts.conditional_p(d32, perp)))
    return out


# ---- the statement equals scikit-learn -----------------------------------------------------------------------------------
def test_conditional_p_equals_sklearn(affinities):
    for d32, perp, want, (got, beta, steps) in affinities:
        n = d32.shape[0]
        assert np.all(np.diag(got) == 0) and steps.max() < 99 and np.all(beta > 0)
        assert np.all(np.abs(got - want) <= (n + 16) * 2 * U * want + 1e-300)
        assert np.allclose(got.sum(axis=1), 1.0, rtol=n * 2 * U, atol=0)


def test_joint_p_equals_sklearn(affinities, golden):
    for d32, perp, _, (cond, _, _) in affinities:
        n = d32.shape[0]
        want = squareform(_t_sne._joint_probabilities(d32, perp, 0))
        got = ts.joint_p(cond)
        off = ~np.eye(n, dtype=bool)
        assert np.all(np.abs(got - want)[off] <= (n * n + 8) * U * want[off] + (n + 16) * 2 * U * want[off])
        assert np.all(np.diag(got) == ts.EPS) and np.array_equal(got, got.T)
    x = golden["p96_x"]
    got = ts.joint_p(ts.conditional_p(ts.pair_sqdist_f32(x), float(golden["p96_perplexity"]))[0])
    off = ~np.eye(96, dtype=bool)
    assert np.allclose(got[off], golden["p96_joint"][off], rtol=(96 * 96 + 8) * U + (96 + 16) * 2 * U, atol=0)


@pytest.mark.parametrize("scale", (1e-4, 5.0, 200.0))
@pytest.mark.parametrize("e", (1.0, 12.0))
def test_objective_and_gradient_equal_sklearn(affinities, scale, e):
    d32, perp, _, (cond, _, _) = affinities[1]
    n = d32.shape[0]
    P = ts.joint_p(cond)
    Y = ts.step_embedding(n, scale, 5)
    o = ts.objective(Y, P, e)
    kl, grad = _t_sne._kl_divergence(Y.ravel().copy(), squareform(P, checks=False) * e, 1, n, 2)
    assert abs(o["kl"] - kl) <= (n * n + 64) * U * o["kl_abs"]
    assert np.all(np.abs(o["grad"] - grad.reshape(n, 2)) <= 4 * (32 * n * U * o["A"] + n * n * U * o["B"]) + 1e-300)
    if scale == 200.0:
        assert (o["q"][~np.eye(n, dtype=bool)] == ts.EPS).any()      # the clamp on q is active here


def test_ten_iterations_equal_sklearn(affinities):
    d32, perp, _, (cond, _, _) = affinities[1]
    n = d32.shape[0]
    P = ts.joint_p(cond)
    Y0 = 1e-4 * np.random.RandomState(11).standard_normal((n, 2))
    lr = max(n / 12.0 / 4, 50.0)
    want, _, it = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), it=0, max_iter=10, n_iter_check=50,
                                           momentum=0.5, learning_rate=lr, args=[squareform(P, checks=False) * 12.0, 1, n, 2],
                                           kwargs={})
    got, margin = ts.steps(P, Y0, 10)
    assert it == 9
    # a 1e-13 perturbation grows at most 200-fold in ten iterations (DESIGN.md "K30"); the two gradients differ by 1e-14
    assert np.abs(got - want.reshape(n, 2)).max() <= 1e-10 * np.abs(got).max()


def test_descent_loop_follows_sklearns_schedule(monkeypatch):
    """The phases, the reset and the checks of TSNE._tsne, on a recorded objective."""
    calls = []

    def objective(Y, P, e):
        calls.append(e)
        return {"kl": 1.0 / len(calls), "grad": np.full_like(Y, 1e-3)}
    monkeypatch.setattr(ts, "objective", objective)
    Y, kl, it = ts.descend(None, np.zeros((8, 2)), max_iter=300)
    assert it == 299 and calls == [12.0] * 250 + [1.0] * 50 and kl == 1.0 / 300


def _sklearn_on_script(monkeypatch, max_iter, window, kl, zero_grad):
    """TSNE._tsne itself with _kl_divergence replaced by the script -> (n_iter_, kl_divergence_, [(exaggeration,
    compute_error)] per objective call).  The exaggeration is read off P, which _tsne scales in place around phase 1."""
    calls = []

    def scripted(params, P, degrees_of_freedom, n_samples, n_components, skip_num_points=0, compute_error=True):
        i = len(calls)
        calls.append((float(P[0]), bool(compute_error)))
        grad = np.zeros_like(params) if i in zero_grad else np.full_like(params, 1e-3)
        return (kl(i) if compute_error else np.nan), grad
    monkeypatch.setattr(_t_sne, "_kl_divergence", scripted)
    est = _t_sne.TSNE(method="exact", max_iter=max_iter, n_iter_without_progress=window)
    est.learning_rate_ = 50.0
    est._tsne(np.ones(1), 1, 8, np.zeros((8, 2)))
    return est.n_iter_, est.kl_divergence_, calls


def _statement_on_script(monkeypatch, max_iter, window, kl, zero_grad):
    calls = []

    def objective(Y, P, e):
        i = len(calls)
        calls.append(e)
        return {"kl": kl(i), "grad": np.zeros_like(Y) if i in zero_grad else np.full_like(Y, 1e-3)}
    monkeypatch.setattr(ts, "objective", objective)
    Y, got_kl, it = ts.descend(None, np.zeros((8, 2)), max_iter=max_iter, n_iter_without_progress=window)
    return it, got_kl, calls


@pytest.mark.parametrize("name", sorted(ts.DESCENT_SCRIPTS))
def test_descent_stop_rules_equal_sklearn(monkeypatch, name):
    """Both early exits, the restart of phase 2 one past a stopped phase 1 and the fall-through, each on a scripted
    objective: the statement's loop and sklearn's TSNE._tsne give the same n_iter, the same KL and the same number of
    objective calls per phase, and both give what the rules say by hand (tests/tsne_reference.py DESCENT_SCRIPTS)."""
    max_iter, window, kl, zero_grad, want_it, want_calls = ts.DESCENT_SCRIPTS[name]
    sk_it, sk_kl, sk_calls = _sklearn_on_script(monkeypatch, max_iter, window, kl, zero_grad)
    it, got_kl, calls = _statement_on_script(monkeypatch, max_iter, window, kl, zero_grad)
    per_phase = (calls.count(12.0), calls.count(1.0))
    assert (sk_it, ([c[0] for c in sk_calls].count(12.0), [c[0] for c in sk_calls].count(1.0))) == (want_it, want_calls)
    assert (it, per_phase) == (want_it, want_calls)
    assert calls == [c[0] for c in sk_calls]
    # sklearn asks for the error on every 50th iteration and on the last one a phase can reach, nowhere else
    ends = [ts.EXPLORATION_ITER] * want_calls[0] + [max_iter] * want_calls[1]
    first2 = want_it + 1 - want_calls[1]
    index = list(range(want_calls[0])) + list(range(first2, first2 + want_calls[1]))
    assert [c[1] for c in sk_calls] == [ts.asks_error(i, end) for i, end in zip(index, ends)]
    if want_calls[1] == 0:
        # the one place where the statement leaves sklearn on purpose (DESIGN.md "K30", Driver): a second phase without an
        # iteration returns _gradient_descent's initial error, the largest float, as kl_divergence_; the statement and the
        # device driver report the last error computed, that of iteration 249
        assert sk_kl == np.finfo(np.float64).max and got_kl == kl(ts.EXPLORATION_ITER - 1)
    else:
        assert got_kl == sk_kl == kl(want_it)


def test_pca_scores_equal_sklearn():
    for n, c, seed, dtype in ((64, 2, 0, np.float64), (257, 22, 1, np.float32), (300, 100, 2, np.float64)):
        r = np.random.RandomState(seed)
        x = (r.standard_normal((n, c)) * (3.0 * 0.6 ** np.minimum(np.arange(c), 6)) + r.standard_normal(c)).astype(dtype)
        est = PCA()
        want = est.fit_transform(x.astype(np.float64))[:, :2]
        ev = est.explained_variance_[:3] if c > 2 else np.append(est.explained_variance_[:2], 0.0)
        g = min((ev[0] - ev[1]) / ev[0], (ev[1] - ev[2]) / ev[1])
        assert g >= 0.1
        rownorm = np.linalg.norm(x.astype(np.float64) - x.astype(np.float64).mean(0), axis=1).max()
        assert np.abs(ts.pca_scores(x) - want).max() <= 64 * n * U * rownorm / g


# ---- the public functions --------------------------------------------------------------------------------------------------
@pytest.fixture
def statement_hook(monkeypatch):
    from ark_analysis_amd.analysis import dimensionality_reduction as dr
    calls = []

    def hook(values, algorithm, random_state, perplexity, max_iter, init):
        calls.append((values.dtype, values.shape, algorithm, perplexity, max_iter))
        return ts.embed(values, algorithm, random_state, perplexity, max_iter, init)
    monkeypatch.setattr(dr, "_embed_device", hook)
    return dr, calls


def _cell_table(n=60, seed=3):
    x, lab = ts.blobs(n, 4, 3, seed)
    df = pd.DataFrame(x, columns=["A", "B", "C", "D"])
    df["cell_type"] = np.array(["T", "B", "NK"])[lab]
    return df, lab


def test_reduce_dimensions_over_the_statement(statement_hook):
    dr, calls = statement_hook
    df, lab = _cell_table()
    x = df[["A", "B", "C", "D"]].values
    pca = dr.reduce_dimensions(x, "PCA")
    assert pca.shape == (60, 2) and pca.kl_divergence_ is None
    assert np.allclose(pca, PCA().fit_transform(x)[:, :2], rtol=0, atol=1e-10)
    emb = dr.reduce_dimensions(x.astype(np.float32), "tSNE", perplexity=10.0, max_iter=250, init="random", random_state=4)
    assert emb.shape == (60, 2) and emb.dtype == np.float64 and np.isfinite(emb).all()
    # max_iter = 250 leaves the second phase empty: sklearn reports n_iter_ = 250 then; the KL is the last one computed
    assert emb.n_iter_ == 250 and 0 < emb.kl_divergence_ < 100
    assert [c[0] for c in calls] == [np.float64, np.float32]
    again = dr.reduce_dimensions(x.astype(np.float32), "tSNE", perplexity=10.0, max_iter=250, init="random", random_state=4)
    assert np.array_equal(emb, again)


@pytest.mark.parametrize("algorithm,fname", (("PCA", "PCAVisualization.png"), ("tSNE", "tSNEVisualization.png")))
def test_visualiser_writes_the_png(statement_hook, tmp_path, algorithm, fname):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    dr, calls = statement_hook
    df, _ = _cell_table()
    df.loc[5, "B"] = np.nan                     # dropped, as the reference drops it
    emb = dr.visualize_dimensionality_reduction(df, ["A", "B", "C", "D"], "cell_type", algorithm=algorithm, dpi=40,
                                                save_dir=str(tmp_path), perplexity=10.0, max_iter=250, random_state=0)
    assert emb.shape == (59, 2) and calls[0][1] == (59, 4)
    with open(tmp_path / fname, "rb") as f:
        assert f.read(8) == b"\x89PNG\r\n\x1a\n"
    fig = plt.figure({"PCA": 2, "tSNE": 3}[algorithm])
    ax = fig.axes[0]
    assert ax.get_title() == "%s projection of data" % algorithm
    assert [t.get_text() for t in ax.get_legend().get_texts()] == ["B", "NK", "T"]
    assert sum(len(coll.get_offsets()) for coll in ax.collections) == 59
    plt.close("all")
    with pytest.raises(FileNotFoundError):
        dr.plot_dim_reduced_data(emb[:, 0], emb[:, 1], 9, df.dropna()["cell_type"], df, "t", save_dir=str(tmp_path / "no"),
                                 save_file="x.png")
    plt.close("all")


def test_refusals(statement_hook):
    dr, calls = statement_hook
    x = ts.blobs(40, 3, 2, 0)[0]
    with pytest.raises(ValueError, match="Not all values given in list algorithm"):
        dr.reduce_dimensions(x, "MDS")
    with pytest.raises(ValueError, match="Not all values given in list algorithm"):
        dr.visualize_dimensionality_reduction(pd.DataFrame(x, columns=list("abc")), ["a", "b"], "c", algorithm="mds")
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        dr.reduce_dimensions(x, "tSNE", perplexity=40.0)
    bad = x.copy()
    bad[3, 1] = np.inf
    for algorithm in ("PCA", "tSNE"):
        with pytest.raises(ValueError, match="NaN or infinity"):
            dr.reduce_dimensions(bad, algorithm)
    for table in (x[:, :1], x[:1]):
        with pytest.raises(ValueError, match="at least 2 rows and 2 columns"):
            dr.reduce_dimensions(table, "PCA")
    with pytest.raises(ValueError, match="init"):
        dr.reduce_dimensions(x, "tSNE", perplexity=5.0, init=np.zeros((39, 2)))
    with pytest.raises(ValueError, match="init"):
        dr.reduce_dimensions(x, "tSNE", perplexity=5.0, init="spectral")
    with pytest.raises(ValueError, match="max_iter"):
        dr.reduce_dimensions(x, "tSNE", perplexity=5.0, max_iter=100)
    with pytest.raises(ValueError, match="2-D"):
        dr.reduce_dimensions(x[0], "PCA")
    assert calls == []


def test_umap_needs_the_package():
    from ark_analysis_amd.analysis import dimensionality_reduction as dr
    try:
        import umap  # noqa: F401
    except ImportError:
        pass
    else:
        pytest.skip("umap imports here")
    with pytest.raises(ImportError, match='"tSNE" and "PCA"'):
        dr.reduce_dimensions(ts.blobs(40, 3, 2, 0)[0], "UMAP")


def test_without_a_device_there_is_no_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from ark_analysis_amd.analysis import dimensionality_reduction as dr
    with pytest.raises(RuntimeError, match="no HIP device"):
        dr.reduce_dimensions(ts.blobs(40, 3, 2, 0)[0], "PCA")


# ---- the ABI and the fixture -------------------------------------------------------------------------------------------
def test_abi_and_refusals_before_any_hip_call():
    from ark_analysis_amd import _capi, som_device as sd
    lib = _capi.lib()
    with open(os.path.join(ROOT, "include", "pxsom.h")) as f:
        header = f.read()
    assert lib.pxsom_abi_version() == 9
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and re.search(r"\b%s\(" % name, header) and hasattr(lib, name), name
    assert re.search(r"^#define PXSOM_TSNE_MAX_ROWS %d$" % sd.TSNE_MAX_ROWS, header, flags=re.M)
    assert "embedding" in open(os.path.join(ROOT, "ark_analysis_amd", "som_device", "__init__.py")).read()
    ws = lib.pxsom_tsne_workspace_bytes
    assert ws(0) == 0 and ws(sd.TSNE_MAX_ROWS + 1) == 0 and ws(300) >= 3 * 300 * 8 and ws(300) % 256 == 0
    p = ctypes.c_void_p(4096)           # never dereferenced: every call below is refused before any HIP call
    inv, unsup, wsp = -1, -2, -3
    assert lib.pxsom_column_moments(p, 10, 1, 1, p, p, None) == unsup
    assert lib.pxsom_column_moments(p, 1, 4, 1, p, p, None) == unsup
    assert lib.pxsom_column_moments(p, 10, 1025, 1, p, p, None) == unsup
    assert lib.pxsom_column_moments(p, 10, 4, 2, p, p, None) == unsup          # float16 is not taken
    assert lib.pxsom_column_moments(None, 10, 4, 1, p, p, None) == inv
    assert lib.pxsom_column_moments(p, 10, 4, 1, None, p, None) == inv
    assert lib.pxsom_project_rows(p, 10, 4, 0, p, None, p, None) == inv
    assert lib.pxsom_project_rows(p, 0, 4, 0, p, p, p, None) == unsup
    assert lib.pxsom_pair_sqdist_f32(p, 10, 4, 0, None, None) == inv
    assert lib.pxsom_pair_sqdist_f32(p, sd.TSNE_MAX_ROWS + 1, 4, 0, p, None) == unsup
    big = ws(10)
    assert lib.pxsom_tsne_affinities(p, 1, 30.0, 1, p, p, p, p, big, None) == unsup
    assert lib.pxsom_tsne_affinities(p, 10, 0.0, 1, p, p, p, p, big, None) == inv
    assert lib.pxsom_tsne_affinities(p, 10, 3.0, 1, p, None, p, p, big, None) == inv
    assert lib.pxsom_tsne_affinities(p, 10, 3.0, 1, p, p, p, p, big - 1, None) == wsp
    assert lib.pxsom_tsne_affinities(p, 10, 3.0, 1, p, p, p, None, big, None) == wsp
    q = ctypes.c_void_p(8192)
    step = lambda *a: lib.pxsom_tsne_step(*a)       # noqa: E731
    assert step(p, 1, p, q, p, p, 1.0, 0.5, 50.0, 0.01, 0, None, None, p, big, None) == unsup
    assert step(p, 10, p, p, p, p, 1.0, 0.5, 50.0, 0.01, 0, None, None, p, big, None) == inv     # y_in is y_out
    assert step(p, 10, p, q, p, p, 1.0, 0.5, 50.0, 0.01, 1, None, None, p, big, None) == inv     # an error without its buffer
    assert step(p, 10, p, q, p, p, float("nan"), 0.5, 50.0, 0.01, 0, None, None, p, big, None) == inv
    assert step(None, 10, p, q, p, p, 1.0, 0.5, 50.0, 0.01, 0, None, None, p, big, None) == inv
    assert step(p, 10, ctypes.c_void_p(4104), q, p, p, 1.0, 0.5, 50.0, 0.01, 0, None, None, p, big, None) == inv
    assert step(p, 10, p, q, p, p, 1.0, 0.5, 50.0, 0.01, 0, None, None, p, big - 1, None) == wsp
    assert step(p, 10, p, q, p, p, 1.0, 0.5, 50.0, 0.01, 0, None, None, ctypes.c_void_p(4104), big, None) == wsp
    assert b"workspace" in lib.pxsom_last_error()


def test_largest_table_that_fits():
    from ark_analysis_amd import som_device as sd
    for free in (1 << 20, 1 << 30, 200 << 30):
        n = sd.tsne_max_rows(free)
        assert 12 * n * n + sd.tsne_workspace_bytes(n) <= free < 12 * (n + 1) ** 2 + sd.tsne_workspace_bytes(n + 1)
    assert sd.tsne_max_rows(0) == 0 and sd.tsne_max_rows(1 << 60) == sd.TSNE_MAX_ROWS
    assert sd.tsne_learning_rate(300) == 50.0 and sd.tsne_learning_rate(48000) == 1000.0


def test_generator_reproduces_the_committed_fixture(golden, tmp_path):
    """One seed and the 96-row P again (a whole run of the generator takes six exact fits).  The KL is compared to 1e-9:
    sklearn forms it with a BLAS dot product."""
    seed = int(golden["kl_seeds"][0])
    env = dict(os.environ, PXSOM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_tsne.py"), "--seeds", str(seed)], check=True,
                   env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with np.load(tmp_path / "g33_tsne.npz") as g:
        assert sorted(g.files) == sorted(golden)
        assert np.array_equal(g["p96_x"], golden["p96_x"]) and g["p96_perplexity"] == golden["p96_perplexity"]
        assert np.allclose(g["p96_joint"], golden["p96_joint"], rtol=1e-13, atol=0)
        assert np.allclose(g["kl_sklearn"], golden["kl_sklearn"][:1], rtol=1e-9, atol=0)
        assert np.array_equal(g["n_iter_sklearn"], golden["n_iter_sklearn"][:1])
    assert len(golden["kl_seeds"]) == 6 and np.all((golden["kl_sklearn"] > 0.3) & (golden["kl_sklearn"] < 1.0))
