"""Inputs that put pxsom_kmeans_lloyd (K19) on its register, block and group edges; no device is needed to build them.

Every case is a dict: ``name``, ``x`` [n, d], ``inits`` (a list of [k_p, d] centres: the problems of one call), ``tol`` and
``max_iter`` (one number, or one per problem).  Rows are integer-valued with x.sum() < 2^53, so every sum of rows is exact
in any order and the device has to equal the statement of tests/kmeans_reference.py in every bit; ``_case`` asserts both.
The seed of an input is a function of its shape, as in tests/test_gpu_kmeans.py.  tests/test_kmeans_edge_cases.py checks on
the statement that each family does what it is built for (so many empty clusters, a tie at the cut, groups that close
and re-form); tests/test_gpu_kmeans_edges.py runs them on the device.  The real-valued family at the end is the one that
is compared within a tolerance."""
import numpy as np

from tests import kmeans_reference as kr
from tests import test_kmeans as tk

GRID_N = (255, 256, 257, 511, 512, 513, 769)                          # around one, two and three blocks of 256 rows
GRID_D = (2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)           # both sides of 8|9, 16|17, 32|33; d % 4 = 0 .. 3
DUPLICATE_D = (8, 9, 17, 33, 63)
# (n, d, seed of the init rows): the seed is 3 as in the duplicate-init family, except where that puts the farthest row f
# at f + 256 >= n -- the planted copy would wrap to a lower row and be taken before f - 1 (769 x 17: f = 590 under seed 3)
TIE_SHAPES = ((513, 9, 3), (769, 17, 0), (600, 33, 3))
ALL_EQUAL_SHAPES = ((257, 33), (513, 9), (300, 17), (64, 64), (32, 8))
REAL_D, REAL_K, REAL_N = (9, 17, 33), (3, 7), 513
# RandomState seed of the kmeans_plusplus draws per d, chosen on the statement so that no row of any iteration has its
# two best distances closer than BAND = 1e-9 relative, with the narrowest gap each gives (k = 3 and k = 7 together)
REAL_SEEDS = {9: (0, 1.25e-3), 17: (0, 7.25e-4), 33: (0, 1.47e-4)}

# ---- the grouping rule of csrc/pxsom_kmeans.hip, restated ----------------------------------------------------------
LDS_BUDGET = 65536
MAX_GROUP = 32


def group_bytes(sum_k, n_problems, d):
    """LDS bytes of a group: centres padded to four columns, per-wave distance sums, a block's labels, and six bytes
    per centre for which problem, which centre and which table row it is."""
    dp = (d + 3) // 4 * 4
    return sum_k * dp * 8 + n_problems * 4 * 8 + n_problems * 256 + sum_k * 6


def groups(d, ks):
    """The problems 0 .. len(ks) - 1 cut into groups: taken in order, a group closes when the next problem would not
    fit the budget or it holds 32.  A list of lists of problem indices."""
    out, cur, sum_k = [], [], 0
    for p, k in enumerate(ks):
        if cur and (len(cur) == MAX_GROUP or group_bytes(sum_k + k, len(cur) + 1, d) > LDS_BUDGET):
            out.append(cur)
            cur, sum_k = [], 0
        cur.append(p)
        sum_k += k
    if cur:
        out.append(cur)
    return out


# ---- builders --------------------------------------------------------------------------------------------------------
def _case(name, x, inits, tol=None, max_iter=tk.MAX_ITER):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert (x == np.round(x)).all() and x.sum() < 2.0 ** 53, name
    inits = [np.ascontiguousarray(c, dtype=np.float64) for c in inits]
    assert all(c.ndim == 2 and c.shape[1] == x.shape[1] and 1 <= len(c) <= len(x) for c in inits), name
    return {"name": name, "x": x, "inits": inits, "tol": tk.tolerance(x) if tol is None else tol, "max_iter": max_iter}


def _seed(n, d, k):
    return 1000 * n + 10 * d + k


def _duplicated(n, d, init_seed=3):
    """Rows, and six centres of which 3, 4 and 5 equal centre 0: the first minimum wins, so they win no row."""
    x = tk.counts_matrix(n, d, _seed(n, d, 6))
    init = tk.rows_as_inits(x, 6, init_seed)
    init[3:] = init[0]
    return x, init


def shape_grid():
    out = []
    for n in GRID_N:
        for d in GRID_D:
            x = tk.counts_matrix(n, d, _seed(n, d, 0))
            out.append(_case("grid-n%d-d%d" % (n, d), x, [tk.rows_as_inits(x, 6, 1), tk.rows_as_inits(x, 7, 2)]))
    return out


def duplicate_init_cases():
    out = []
    for n in GRID_N:
        for d in DUPLICATE_D:
            x, init = _duplicated(n, d)
            out.append(_case("duplicate-n%d-d%d" % (n, d), x, [init]))
    return out


def tie_row(x, init):
    """The row the statement finds farthest from its centre under ``init``."""
    return int(kr.farthest_rows(kr.assign(x, init)[1], 1)[0])


def mirrored(x, init, f, count):
    """``count`` rows as far from their centre as row f is and different from it and from each other: row f with one
    column mirrored at its centre, kept where no other centre comes nearer."""
    labels, best, _ = kr.assign(x, init)
    centre, out = init[labels[f]], []
    for j in np.flatnonzero(x[f] != centre):
        row = x[f].copy()
        row[j] = 2 * centre[j] - row[j]
        if kr.assign(row[None], init)[1][0] == best[f]:
            out.append(row)
        if len(out) == count:
            return np.stack(out)
    raise AssertionError("fewer than %d mirrored rows keep the distance" % count)


def tie_at_the_cut_cases():
    """The farthest row f copied to f - 1, f + 1 and (f + 256) % n: four rows tie for the three empty clusters, f and
    f + 256 in one thread of the strided search, f + 256 in another block of the sums.  ``f`` rides in the case.

    Copies are equal rows of one cluster, so which three of the four are taken shows nowhere in the result.  Each shape
    therefore comes a second time (``tie-distinct-``) with three *mirrored* rows in the copies' places: the same distance,
    four different rows, and the centres tell which rows were taken and in which order."""
    out = []
    for n, d, init_seed in TIE_SHAPES:
        for distinct in (False, True):
            x, init = _duplicated(n, d, init_seed)
            f = tie_row(x, init)
            assert 1 <= f and f + 256 < n, (n, d, f)
            x[[f - 1, f + 1, (f + 256) % n]] = mirrored(x, init, f, 3) if distinct else x[f]
            case = _case("tie-%sn%d-d%d" % ("distinct-" if distinct else "", n, d), x, [init])
            case["f"], case["distinct"] = f, distinct
            out.append(case)
    return out


def all_equal_init_cases():
    """k = 32 with every centre equal to row 0: centre 0 wins every row and 31 clusters are empty in iteration 1."""
    out = []
    for n, d in ALL_EQUAL_SHAPES:
        x = tk.counts_matrix(n, d, _seed(n, d, 32))
        out.append(_case("all-equal-n%d-d%d" % (n, d), x, [np.repeat(x[:1], 32, axis=0)]))
    return out


def limit_cases():
    out = []
    for n in (1, 63, 257):
        x = tk.counts_matrix(n, 5, _seed(n, 5, 1))
        out.append(_case("k1-n%d" % n, x, [tk.rows_as_inits(x, 1, 1)]))
    x = tk.counts_matrix(32, 5, 1)
    assert len(np.unique(x, axis=0)) == 32
    out.append(_case("k32-n32", x, [tk.rows_as_inits(x, 32, 1)]))
    x = tk.counts_matrix(1, 64, _seed(1, 64, 1))
    out.append(_case("k1-n1-d64", x, [x.copy()]))
    return out


GROUP_KS = {"many": [1 + p % 2 for p in range(33)],                   # two groups by the 32-problem limit
            "mixed": [32, 31, 1, 32, 2, 32, 32, 5],                   # two groups by the byte rule, unequal offsets
            "leaving": list(range(2, 14))}                            # one group that shrinks as its problems stop
GROUP_D = {"many": 3, "mixed": 64, "leaving": 17}


def group_cases():
    out = []
    for which in ("many", "mixed", "leaving"):
        d, ks = GROUP_D[which], GROUP_KS[which]
        x = tk.counts_matrix(300, d, _seed(300, d, len(ks)))
        inits = [tk.rows_as_inits(x, k, p) for p, k in enumerate(ks)]
        if which == "leaving":
            tol = [0.0 if p % 2 == 0 else 1e9 for p in range(len(ks))]
            max_iter = [(1, 2, tk.MAX_ITER)[p % 3] for p in range(len(ks))]
            out.append(_case("group-" + which, x, inits, tol, max_iter))
        else:
            out.append(_case("group-" + which, x, inits))
    return out


FAMILIES = (("shape_grid", shape_grid), ("duplicate_init", duplicate_init_cases), ("tie_at_the_cut", tie_at_the_cut_cases),
            ("all_equal_init", all_equal_init_cases), ("limit", limit_cases), ("group", group_cases))
_BUILT = {}


def family(name):
    """The cases of a family, built once per process."""
    if name not in _BUILT:
        _BUILT[name] = dict(FAMILIES)[name]()
    return _BUILT[name]


def all_cases():
    return [case for name, _ in FAMILIES for case in family(name)]


def names(family_name):
    """The case names of a family from its shapes alone: what a parametrised test is keyed by.  Nothing is built, so
    collecting the tests costs nothing; tests/test_kmeans_edge_cases.py checks the names against the built cases."""
    return {"shape_grid": ["grid-n%d-d%d" % (n, d) for n in GRID_N for d in GRID_D],
            "duplicate_init": ["duplicate-n%d-d%d" % (n, d) for n in GRID_N for d in DUPLICATE_D],
            "tie_at_the_cut": ["tie-%sn%d-d%d" % (kind, n, d) for n, d, _ in TIE_SHAPES for kind in ("", "distinct-")],
            "all_equal_init": ["all-equal-n%d-d%d" % shape for shape in ALL_EQUAL_SHAPES],
            "limit": ["k1-n1", "k1-n63", "k1-n257", "k32-n32", "k1-n1-d64"],
            "group": ["group-" + which for which in ("many", "mixed", "leaving")]}[family_name]


def by_name(name):
    """A case by its name; only its family is built."""
    for family_name, _ in FAMILIES:
        if name in names(family_name):
            return family(family_name)[names(family_name).index(name)]
    raise KeyError(name)


def per_problem(case):
    """(init, tol, max_iter) of every problem of a case."""
    p = len(case["inits"])
    return list(zip(case["inits"], np.broadcast_to(case["tol"], (p,)), np.broadcast_to(case["max_iter"], (p,))))


# ---- real-valued rows across the register classes -------------------------------------------------------------------
def freq_rows(n, d):
    """tk.freq_matrix with n rows and d columns: counts divided by their sum, five archetypes."""
    rs = np.random.RandomState(_seed(n, d, 5))
    arche = rs.choice([0.3, 2.0, 9.0], size=(5, d))
    counts = rs.poisson(arche[rs.randint(0, 5, n)]).astype(np.float64)
    counts[counts.sum(axis=1) == 0, 0] = 1
    return counts / counts.sum(axis=1, keepdims=True)


def real_valued_case(d, seed=None):
    """Centred frequencies [513, d] with kmeans_plusplus inits for k = 3 and 7 from one RandomState(REAL_SEEDS[d])."""
    from sklearn.cluster import kmeans_plusplus
    f = freq_rows(REAL_N, d)
    x = f - f.mean(axis=0)
    rs = np.random.RandomState(REAL_SEEDS[d][0] if seed is None else seed)
    return {"name": "real-d%d" % d, "x": x, "inits": [kmeans_plusplus(x, k, random_state=rs)[0] for k in REAL_K],
            "tol": tk.tolerance(f), "max_iter": tk.MAX_ITER}


def narrowest_gap(case):
    """(the statement's results per problem, the smallest relative gap between a row's two best distances over every
    iteration of every problem)."""
    wants, gaps = [], []
    for init, tol, max_iter in per_problem(case):
        trace = []
        wants.append(kr.lloyd(case["x"], init, tol, max_iter, trace))
        gaps.extend(step[3] for step in trace)
    return wants, min(gaps)
