"""The numpy statement of K30 (include/pxsom.h, csrc/pxsom_embed.hip): column moments and PCA scores, the squared distances,
sklearn's perplexity search and dense joint P, one exact t-SNE iteration and the descent loop.  tests/test_tsne.py pins it to
scikit-learn itself; tests/test_gpu_tsne.py compares the kernels with it."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)       # 2^-52, sklearn's MACHINE_EPSILON
EXPLORATION_ITER, ITER_CHECK, EARLY_EXAGGERATION, MIN_GAIN, MIN_GRAD_NORM = 250, 50, 12.0, 0.01, 1e-7


def blobs(n, c, k, seed, sep=6.0):
    """k blobs with centres N(0, sep^2), unit noise and label i mod k."""
    r = np.random.RandomState(seed)
    cent = r.normal(0, sep, size=(k, c))
    lab = np.arange(n) % k
    return cent[lab] + r.normal(0, 1, size=(n, c)), lab


def end_to_end_case(seed):
    """The end-to-end case: three blobs of 300 x 10, their labels, and the fixed initial embedding of that seed."""
    x, lab = blobs(300, 10, 3, seed)
    return x, lab, 1e-4 * np.random.RandomState(100 + seed).standard_normal((300, 2))


# ---- PCA ---------------------------------------------------------------------------------------------------------------
def column_moments(x):
    """Means and the centred covariance over n - 1, with the sums of absolute terms behind each entry."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    d = x - mean
    cov = d.T @ d / (n - 1)
    return mean, cov, np.abs(x).sum(axis=0) / n, np.abs(d).T @ np.abs(d) / (n - 1)


def principal_axes(cov):
    vals, vecs = np.linalg.eigh(cov)
    axes = np.ascontiguousarray(vecs[:, ::-1][:, :2].T)
    signs = np.sign(axes[np.arange(2), np.argmax(np.abs(axes), axis=1)])
    signs[signs == 0] = 1.0
    return axes * signs[:, None]


def pca_scores(x):
    x = np.asarray(x, dtype=np.float64)
    mean, cov, _, _ = column_moments(x)
    return (x - mean) @ principal_axes(cov).T


# ---- affinities --------------------------------------------------------------------------------------------------------
def pair_sqdist_f32(x):
    """d2[i, j] = sum_t (x_it - x_jt)^2 in binary64, t ascending, one rounding per operation, then float32."""
    x = np.asarray(x).astype(np.float64)
    s = np.zeros((x.shape[0], x.shape[0]))
    for t in range(x.shape[1]):
        d = x[:, None, t] - x[None, :, t]
        s += d * d
    return s.astype(np.float32)


def row_entropy_diff(drow, i, beta, perplexity):
    """H - log(perplexity) of row i at beta, as the search evaluates it."""
    d = drow.astype(np.float64)
    mask = np.ones(d.size, bool)
    mask[i] = False
    p = np.where(mask, np.exp(-d * beta), 0.0)
    s = p.sum()
    if s == 0.0:
        s = float(np.float32(1e-8))
    return np.log(s) + beta * (d * (p / s)).sum() - np.log(float(np.float32(perplexity)))


def conditional_p(d32, perplexity, margin=False):
    """sklearn/manifold/_utils.pyx _binary_search_perplexity on a dense float32 matrix -> (P, beta, steps), with ``margin``
    also a per-row margin [n].

    The margin says how far a row's search is from taking another path on an implementation that rounds differently.  The
    search branches on diff = log s + beta * sum_j d_j p_j - log perplexity twice: on |diff| <= tol (stop) and on the sign of
    diff (which bound moves).  Another path needs |diff| to cross tol or diff to cross 0, so at one evaluation the distance
    to a branch is min(|diff|, ||diff| - tol|).  The rounding bound E of diff at that evaluation, U = 2^-53: s is a sum of
    n - 1 terms exp(-d_j beta), each with a relative error of a few U (the product, the exponential; a term whose argument
    is large enough for the product's error to matter weighs x exp(-x) <= 0.37 of that), so s carries at most (n + 16) U
    relatively, log s that much absolutely plus U |log s| of its own; beta * sum d p is a sum of n - 1 non-negative terms
    over the same s: (n + 16) U of its value; log perplexity one rounding, U |log perplexity|.  Together at most
    (n + 16) U (1 + |log s| + beta sum d p + |log perplexity|) for one implementation, twice that between two:
        E = 2 (n + 16) U (1 + |log s| + beta * sum d p + |log perplexity|).
    The row's margin is the smallest min(|diff|, ||diff| - tol|) / E over its evaluations: above 1, no rounding within
    the bound changes beta or steps."""
    n = d32.shape[0]
    P, betas, steps, margins = np.zeros((n, n)), np.zeros(n), np.zeros(n, np.int32), np.full(n, np.inf)
    tol, tiny = float(np.float32(1e-5)), float(np.float32(1e-8))
    target = np.log(float(np.float32(perplexity)))
    d = d32.astype(np.float64)
    for i in range(n):
        lo, hi, b = -np.inf, np.inf, 1.0
        mask = np.ones(n, bool)
        mask[i] = False
        for it in range(100):
            p = np.where(mask, np.exp(-d[i] * b), 0.0)
            s = p.sum()
            if s == 0.0:
                s = tiny
            p = p / s
            energy = b * (d[i] * p).sum()
            diff = np.log(s) + energy - target
            if margin:
                e = 2 * (n + 16) * 2.0 ** -53 * (1 + abs(np.log(s)) + energy + abs(target))
                margins[i] = min(margins[i], min(abs(diff), abs(abs(diff) - tol)) / e)
            if abs(diff) <= tol:
                break
            if diff > 0:
                lo = b
                b = b * 2 if hi == np.inf else (b + hi) / 2
            else:
                hi = b
                b = b / 2 if lo == -np.inf else (b + lo) / 2
        P[i], betas[i], steps[i] = p, b, it
    return (P, betas, steps, margins) if margin else (P, betas, steps)


def joint_p(cond):
    """The dense form of _joint_probabilities: max((Pc + Pc^T) / max(sum, eps), eps); the diagonal holds eps, unused."""
    P = cond + cond.T
    return np.maximum(P / max(P.sum(), EPS), EPS)


def step_embedding(n, scale, seed):
    """A normal embedding of standard deviation ``scale``.  At scale 200 a few rows are moved out a million-fold: the bare
    draw never reaches the clamp on q (n_ij / Z >= 1e-12 for n <= 513), with them q = eps for their pairs once n >= 16."""
    Y = scale * np.random.RandomState(seed).standard_normal((n, 2))
    if scale == 200.0:
        Y[:max(1, min(3, n // 8))] *= 1e6
    return Y


# ---- one iteration -----------------------------------------------------------------------------------------------------
def objective(Y, P, e=1.0):
    """-> dict: kl, grad [n, 2], Z, q [n, n] (diagonal 0), and the tolerance sums A, B [n, 2] and kl_abs."""
    diff = Y[:, None, :] - Y[None, :, :]
    nn = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(nn, 0.0)
    Z = nn.sum()
    off = ~np.eye(len(Y), dtype=bool)
    q = np.where(off, np.maximum(nn / Z, EPS), 0.0)
    pe = np.where(off, P * e, 0.0)
    terms = np.zeros_like(pe)
    terms[off] = pe[off] * np.log(np.maximum(pe[off], EPS) / q[off])
    w = (pe - q) * nn
    grad = 4.0 * (w[:, :, None] * diff).sum(1)
    A = ((pe + q) * nn)[:, :, None] * np.abs(diff)
    B = (q * nn)[:, :, None] * np.abs(diff)
    return {"kl": terms.sum(), "kl_abs": np.abs(terms).sum(), "grad": grad, "Z": Z, "q": q, "A": A.sum(1), "B": B.sum(1)}


def update(grad, Y, upd, gains, momentum, learning_rate, min_gain=MIN_GAIN):
    """sklearn's _gradient_descent update, elementwise -> (Y, update, gains, grad * gains)."""
    inc = upd * grad < 0.0
    gains = np.where(inc, gains + 0.2, gains * 0.8)
    gains = np.clip(gains, min_gain, np.inf)
    g = grad * gains
    upd = momentum * upd - learning_rate * g
    return Y + upd, upd, gains, g


def steps(P, Y0, count, e=EARLY_EXAGGERATION, momentum=0.5, learning_rate=None):
    """``count`` iterations from Y0 -> (Y, the smallest |update * grad| / (max|update| max|grad|) met after the first)."""
    lr = max(len(Y0) / EARLY_EXAGGERATION / 4, 50.0) if learning_rate is None else learning_rate
    Y, upd, gains, margin = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0), np.inf
    for i in range(count):
        g = objective(Y, P, e)["grad"]
        if i > 0:
            margin = min(margin, np.abs(upd * g).min() / (np.abs(upd).max() * np.abs(g).max()))
        Y, upd, gains, _ = update(g, Y, upd, gains, momentum, lr)
    return Y, margin


def descend(P, Y0, max_iter=1000, n_iter_without_progress=300):
    """sklearn's TSNE._tsne: two _gradient_descent calls -> (Y, kl_divergence, n_iter)."""
    lr = max(len(Y0) / EARLY_EXAGGERATION / 4, 50.0)
    state = {"Y": Y0.copy(), "kl": np.nan}

    def phase(it, end, momentum, e, window):
        Y, upd, gains = state["Y"], np.zeros_like(Y0), np.ones_like(Y0)
        best, best_it, i = np.finfo(np.float64).max, it, it
        for i in range(it, end):
            check = (i + 1) % ITER_CHECK == 0
            o = objective(Y, P, e)
            Y, upd, gains, g = update(o["grad"], Y, upd, gains, momentum, lr)
            if check or i == end - 1:
                state["kl"] = o["kl"]
            if check:
                if o["kl"] < best:
                    best, best_it = o["kl"], i
                elif i - best_it > window:
                    break
                if np.linalg.norm(g) <= MIN_GRAD_NORM:
                    break
        state["Y"] = Y
        return i

    it = phase(0, EXPLORATION_ITER, 0.5, EARLY_EXAGGERATION, EXPLORATION_ITER)
    if it < EXPLORATION_ITER or max_iter - EXPLORATION_ITER > 0:
        it = phase(it + 1, max_iter, 0.8, 1.0, n_iter_without_progress)
    return state["Y"], float(state["kl"]), it


# ---- scripted objectives for the stop rules ------------------------------------------------------------------------------
# The descent is chaotic, so its stop rules are tested on an objective that ignores Y: call number i (which is iteration i,
# since the second phase starts one past the first phase's last iteration) returns kl(i) and a gradient that is zero at the
# iterations listed in ``zero_grad`` and 1e-3 everywhere else.  Each entry: name -> (max_iter, n_iter_without_progress, kl,
# zero_grad, n_iter expected, calls in the two phases expected) -- the expectations worked out by hand from sklearn's rules:
# a check at every i with (i + 1) % 50 == 0; kl < best moves best_it to i, else i - best_it > window stops; then a gradient
# norm <= 1e-7 stops; phase 2 runs from the first phase's last iteration + 1 with best_it set to its first iteration.
def _falling(i):
    return 1.0 / (i + 1)


def _flat_from_300(i):
    return 1.0 / (i + 1) if i < 300 else 1.0        # the best check is i = 299


DESCENT_SCRIPTS = {
    "no_stop": (1000, 300, _falling, (), 999, (250, 750)),
    # a zero gradient stops only where it is looked at: 123, 301 and 310 are no checks
    "grad_stop_phase2": (1000, 300, _falling, (123, 301, 310, 449), 449, (250, 200)),
    "grad_stop_at_49": (1000, 300, _falling, (49,), 999, (50, 950)),
    "grad_stop_at_49_then_99": (1000, 300, _falling, (49, 99), 99, (50, 50)),
    "grad_stop_at_49_max_250": (250, 300, _falling, (49,), 249, (50, 200)),
    # 349 - 299 = 50 is not past a window of 50; 399 - 299 is
    "window_50": (1000, 50, _flat_from_300, (), 399, (250, 150)),
    "window_100": (1000, 100, _flat_from_300, (), 449, (250, 200)),
    "window_300": (1000, 300, _flat_from_300, (), 649, (250, 400)),
    # ends at max_iter on the check where i - best_it equals the window
    "window_300_max_600": (600, 300, _flat_from_300, (), 599, (250, 350)),
    # a KL equal to the best is no progress: best_it stays 299 (49 in the first phase, whose window of 250 cannot run out)
    "kl_equal_best": (1000, 50, lambda i: 0.5, (), 399, (250, 150)),
    # progress at 449 restarts the window
    "progress_restarts_window": (1000, 100, lambda i: 1e-4 if i == 449 else _flat_from_300(i), (), 599, (250, 350)),
    "max_iter_250": (250, 300, _falling, (), 250, (250, 0)),
    "max_iter_251": (251, 300, _falling, (), 250, (250, 1)),
}


def asks_error(i, phase_end):
    """Whether iteration i of a phase that ends before ``phase_end`` computes the error: every 50th and the phase's last."""
    return (i + 1) % ITER_CHECK == 0 or i == phase_end - 1


def embed(values, algorithm, random_state=None, perplexity=30.0, max_iter=1000, init="pca"):
    """What the device hook of analysis.dimensionality_reduction computes -> (embedding, kl, n_iter)."""
    x = np.asarray(values, dtype=np.float64)
    if algorithm == "PCA":
        return pca_scores(x), None, None
    n = x.shape[0]
    if isinstance(init, str):
        if init == "pca":
            y0 = pca_scores(x)
            y0 = y0 / np.std(y0[:, 0]) * 1e-4
        else:
            y0 = 1e-4 * np.random.RandomState(random_state).standard_normal((n, 2))
    else:
        y0 = np.asarray(init, dtype=np.float64)
    P = joint_p(conditional_p(pair_sqdist_f32(values), perplexity)[0])
    return descend(P, y0, max_iter)


def purity(Y, lab, k=5):
    """The share of each point's k nearest embedded neighbours that carry its label."""
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nearest = np.argsort(d, axis=1)[:, :k]
    return float((lab[nearest] == lab[:, None]).mean())
