"""pxsom_kmeans_lloyd on the GPU at its register, block and group edges: the cases of tests/kmeans_edge_cases.py against
the numpy statement of tests/kmeans_reference.py.  The rows are integer-valued, so labels, centres, inertia and iteration
counts are compared bit for bit; tests/test_kmeans_edge_cases.py checks on the statement that every case does what it is
built for.  The last test, on real-valued rows, is the only one with a tolerance: the band and the bounds of
tests/test_gpu_kmeans.py::test_real_valued_rows_against_the_statement."""
import numpy as np
import pytest

from tests import kmeans_edge_cases as ec
from tests import test_kmeans as tk
from tests.test_gpu_kmeans import BAND, _assert_equals_statement, _assert_same_bits, _device

pytestmark = pytest.mark.gpu


def _run(gpu, case, workgroups=0):
    return _device(gpu, case["x"], case["inits"], case["tol"], case["max_iter"], workgroups=workgroups)


def _problems(got, first, last):
    """Problems first .. last - 1 of a device result."""
    return got[0][first:last], got[1][first:last], got[2][first:last], got[3][first:last]


def _alone(gpu, case, p):
    init, tol, max_iter = ec.per_problem(case)[p]
    return _device(gpu, case["x"], [init], tol, max_iter)


def _against_the_statement(gpu, case):
    got = _run(gpu, case)
    _assert_equals_statement(got, case["x"], case["inits"], case["tol"], case["max_iter"], case["name"])
    return got


@pytest.mark.parametrize("name", ec.names("shape_grid"))
def test_shape_grid_equals_the_statement(gpu, name):
    _against_the_statement(gpu, ec.by_name(name))


@pytest.mark.parametrize("name", ec.names("duplicate_init"))
def test_duplicate_inits_equal_the_statement(gpu, name):
    _against_the_statement(gpu, ec.by_name(name))


@pytest.mark.parametrize("name", ec.names("tie_at_the_cut"))
def test_tie_at_the_cut_equals_the_statement(gpu, name):
    case = ec.by_name(name)
    first = _device(gpu, case["x"], case["inits"], 0.0, 1)            # one iteration: the relocated centres themselves
    _assert_equals_statement(first, case["x"], case["inits"], 0.0, 1, name + " after one iteration")
    f = case["f"]
    np.testing.assert_array_equal(first[1][0][3:], case["x"][[f - 1, f, f + 1]])      # rows f - 1, f, f + 1, in that order
    _against_the_statement(gpu, case)


@pytest.mark.parametrize("name", ec.names("all_equal_init"))
def test_all_equal_inits_equal_the_statement(gpu, name):
    _against_the_statement(gpu, ec.by_name(name))


@pytest.mark.parametrize("name", ec.names("limit"))
def test_limit_sizes_equal_the_statement(gpu, name):
    _against_the_statement(gpu, ec.by_name(name))


@pytest.mark.parametrize("name", ec.names("tie_at_the_cut")
                         + ["all-equal-n%d-d%d" % (n, d) for n, d in ec.ALL_EQUAL_SHAPES if n > 256])
def test_relocation_gives_the_same_bits_on_any_grid(gpu, name):
    case = ec.by_name(name)
    nblocks = -(-len(case["x"]) // 256)
    assert nblocks >= 2
    default = _run(gpu, case)
    for workgroups in (1, nblocks, nblocks + 5):
        _assert_same_bits(default, _run(gpu, case, workgroups))


@pytest.mark.parametrize("name", ec.names("group"))
def test_groups_close_by_the_rule_and_change_nothing_a_problem_computes(gpu, name):
    from ark_analysis_amd import som_device
    case = ec.by_name(name)
    d, ks = case["x"].shape[1], [len(c) for c in case["inits"]]
    cut = ec.groups(d, ks)
    assert som_device.kmeans_group_count(d, ks) == len(cut)
    together = _against_the_statement(gpu, case)
    edges = sorted({p for g in cut for p in (g[0], g[-1])})
    if name == "group-many":
        assert edges == [0, 31, 32]
    for p in edges:                                                   # the first and the last problem of each group, alone
        _assert_same_bits(_alone(gpu, case, p), _problems(together, p, p + 1))


@pytest.mark.parametrize("name", ["duplicate-n513-d9", "duplicate-n257-d33"])
def test_relocation_inside_a_shared_group(gpu, name):
    """A problem that relocates three empty clusters and a plain one on the same rows, in one call, in both orders."""
    case = ec.by_name(name)
    x, emptying, tol = case["x"], case["inits"][0], case["tol"]
    plain = tk.rows_as_inits(x, 7, 2)
    alone = [_device(gpu, x, [init], tol, tk.MAX_ITER) for init in (emptying, plain)]
    both = _device(gpu, x, [emptying, plain], tol, tk.MAX_ITER)
    swapped = _device(gpu, x, [plain, emptying], tol, tk.MAX_ITER)
    for p in (0, 1):
        _assert_same_bits(alone[p], _problems(both, p, p + 1))
        _assert_same_bits(alone[p], _problems(swapped, 1 - p, 2 - p))


@pytest.mark.parametrize("d", ec.REAL_D)
def test_real_valued_rows_across_the_register_classes(gpu, d):
    case = ec.real_valued_case(d)
    wants, narrowest = ec.narrowest_gap(case)
    print("d=%d: smallest relative gap between the two best distances over every iteration: %.3g" % (d, narrowest))
    assert narrowest > BAND                          # the condition: no row of any iteration inside the band
    labels, centres, inertia, n_iter = _run(gpu, case)
    scale = np.abs(case["x"]).max()
    for p, want in enumerate(wants):
        err = np.abs(centres[p] - want[1]).max() / scale
        print("d=%d k=%d: %d / %d iterations, centres within %.3g, inertia %.17g / %.17g"
              % (d, len(case["inits"][p]), n_iter[p], want[3], err, inertia[p], want[2]))
        np.testing.assert_array_equal(labels[p], want[0])            # every row lies outside the band
        assert n_iter[p] == want[3]
        assert err <= 1e-12
        assert abs(inertia[p] - want[2]) <= 1e-12 * want[2]
