"""The conditions that make tests/test_gpu_kmeans_edges.py mean something, checked on the numpy statement alone: each
family of tests/kmeans_edge_cases.py does what it is built for.  These are conditions on the reference, not on the
kernel; every case of every family is checked, none is skipped or filtered."""
import numpy as np
import pytest

from tests import kmeans_edge_cases as ec
from tests import kmeans_reference as kr
from tests import test_kmeans as tk

BAND = 1e-9          # tests/test_gpu_kmeans.py's
_TRACES = {}


def traced(case):
    """[(statement result, trace)] per problem of a case, computed once."""
    if case["name"] not in _TRACES:
        runs = []
        for init, tol, max_iter in ec.per_problem(case):
            trace = []
            runs.append((kr.lloyd(case["x"], init, tol, max_iter, trace), trace))
        _TRACES[case["name"]] = runs
    return _TRACES[case["name"]]


def test_the_families_are_whole():
    assert [len(ec.family(name)) for name, _ in ec.FAMILIES] == [98, 35, 6, 5, 5, 3]
    names = [case["name"] for case in ec.all_cases()]
    assert names == [name for family, _ in ec.FAMILIES for name in ec.names(family)]
    assert all(ec.by_name(name)["name"] == name for name in names)
    assert len(set(names)) == len(names) == 152
    grid = {(len(c["x"]), c["x"].shape[1]) for c in ec.family("shape_grid")}
    assert grid == {(n, d) for n in ec.GRID_N for d in ec.GRID_D}
    assert {d % 4 for d in ec.GRID_D} == {0, 1, 2, 3}
    for edge in (8, 16, 32):
        assert edge in ec.GRID_D and edge + 1 in ec.GRID_D
    for case in ec.family("shape_grid"):
        assert [len(c) for c in case["inits"]] == [6, 7]
    assert [(len(c["x"]), c["x"].shape[1], len(c["inits"][0])) for c in ec.family("limit")] == \
        [(1, 5, 1), (63, 5, 1), (257, 5, 1), (32, 5, 32), (1, 64, 1)]


@pytest.mark.parametrize("family", [name for name, _ in ec.FAMILIES])
def test_every_case_is_integer_valued_and_the_statement_terminates(family):
    for case in ec.family(family):
        x = case["x"]
        assert (x == np.round(x)).all() and x.sum() < 2.0 ** 53 and len(x) <= 769, case["name"]
        for (want, trace), (init, tol, max_iter) in zip(traced(case), ec.per_problem(case)):
            labels, centres, inertia, n_iter, why = want
            assert n_iter < tk.MAX_ITER or n_iter == max_iter, case["name"]
            assert why != "max_iter" or max_iter < tk.MAX_ITER, case["name"]
            assert labels.min() >= 0 and labels.max() < len(init), case["name"]
            assert np.isfinite(centres).all() and np.isfinite(inertia), case["name"]


def test_duplicate_inits_leave_exactly_three_empty_clusters():
    for case in ec.family("duplicate_init"):
        (want, trace), = traced(case)
        init = case["inits"][0]
        assert (init[3:] == init[0]).all() and len(np.unique(init[:3], axis=0)) == 3, case["name"]
        assert trace[0][1] == 3, case["name"]
        assert sorted(set(trace[0][0])) == [0, 1, 2], case["name"]


def test_four_rows_tie_for_three_empty_clusters():
    for case in ec.family("tie_at_the_cut"):
        (want, trace), = traced(case)
        x, init, f = case["x"], case["inits"][0], case["f"]
        best = kr.assign(x, init)[1]
        top = np.sort(best)[::-1]
        assert trace[0][1] == 3, case["name"]
        assert top[0] == top[3] > top[4], case["name"]                    # 3rd and 4th largest equal: a tie at the cut
        assert set(kr.farthest_rows(best, 3)) == {f - 1, f, f + 1}, case["name"]
        assert list(kr.farthest_rows(best, 4)) == [f - 1, f, f + 1, f + 256], case["name"]
        assert f % 256 == (f + 256) % 256 and f // 256 != (f + 256) // 256      # one thread of the search, two blocks
        four = x[[f - 1, f, f + 1, f + 256]]
        if case["distinct"]:                                              # four different rows: the centres tell which
            assert len(np.unique(four, axis=0)) == 4, case["name"]
        else:                                                             # copies: equal centres, so empties again later
            assert (four == x[f]).all() and max(step[1] for step in trace[1:]) >= 1, case["name"]
        assert ec.tie_row(x, init) == f - 1                               # the lower row of the tie comes first


def test_all_equal_inits_fill_the_relocation_lists():
    for case in ec.family("all_equal_init"):
        (want, trace), = traced(case)
        init = case["inits"][0]
        assert len(init) == 32 and (init == case["x"][0]).all(), case["name"]
        assert trace[0][1] == 31 and (trace[0][0] == 0).all(), case["name"]
        assert np.bincount(want[0], minlength=32).min() >= 1, case["name"]
    last = ec.family("all_equal_init")[-1]
    assert len(last["x"]) == 32 == len(last["inits"][0])                  # k = n, less than one wave


def test_group_cases_close_and_re_form_groups():
    many, mixed, leaving = ec.family("group")
    for case, which in ((many, "many"), (mixed, "mixed"), (leaving, "leaving")):
        assert [len(c) for c in case["inits"]] == ec.GROUP_KS[which] and len(case["x"]) == 300
        assert case["x"].shape[1] == ec.GROUP_D[which]
    assert [len(g) for g in ec.groups(3, ec.GROUP_KS["many"])] == [32, 1]                 # the 32-problem limit
    assert set(ec.GROUP_KS["many"]) == {1, 2}
    cut = ec.groups(64, ec.GROUP_KS["mixed"])
    assert len(cut) >= 2 and all(len(g) < ec.MAX_GROUP for g in cut)                       # the byte rule
    ks = ec.GROUP_KS["mixed"]
    for g, nxt in zip(cut, cut[1:]):
        assert ec.group_bytes(sum(ks[p] for p in g), len(g), 64) <= ec.LDS_BUDGET
        assert ec.group_bytes(sum(ks[p] for p in g) + ks[nxt[0]], len(g) + 1, 64) > ec.LDS_BUDGET
    assert len({ks[g[0]] for g in cut} | {ks[g[-1]] for g in cut}) > 1                    # unequal k at the group edges
    n_iter = [want[3] for want, _ in traced(leaving)]
    assert len(set(n_iter)) >= 3, n_iter
    assert ec.GROUP_KS["leaving"] == list(range(2, 14))
    assert list(leaving["tol"][:2]) == [0.0, 1e9] and list(leaving["max_iter"][:3]) == [1, 2, tk.MAX_ITER]


def test_the_python_rule_on_the_documented_figures():
    """The figures DESIGN.md K19 and the kernel's header give for the rule."""
    assert ec.group_bytes(32, 1, 64) == 16864 and ec.group_bytes(54, 9, 20) == 11556
    assert [len(g) for g in ec.groups(64, [32] * 10)] == [3, 3, 3, 1]
    assert len(ec.groups(20, range(2, 11))) == 1 and len(ec.groups(20, [10] * 10)) == 1
    assert [len(g) for g in ec.groups(1, [1] * 65)] == [32, 32, 1]


@pytest.mark.parametrize("d", ec.REAL_D)
def test_real_valued_inputs_keep_every_row_outside_the_band(d):
    case = ec.real_valued_case(d)
    assert case["x"].shape == (ec.REAL_N, d) and [len(c) for c in case["inits"]] == list(ec.REAL_K)
    np.testing.assert_allclose(case["x"].mean(axis=0), 0, atol=1e-15)
    assert not (case["x"] == np.round(case["x"])).all()
    wants, narrowest = ec.narrowest_gap(case)
    print("d=%d: narrowest relative gap %.3g over %s iterations" % (d, narrowest, [w[3] for w in wants]))
    assert narrowest > BAND
    assert abs(narrowest / ec.REAL_SEEDS[d][1] - 1) < 0.01                # the gap written beside the seed
