"""Every launch form of the exact online SOM trainers x every storage type against the oracle, bit for bit.

The cases come from tests/online_routes.py, which reads the set of forms from the library's own planning function
(pxsom_train_online_route) and places cases on each form's edges; tests/test_online_routes.py checks on CPU that the list
covers forms x {f16, f32, f64}.  Here each case asserts that the form the library reports is the one it was built for,
trains, and compares the codebook as int64 bit patterns: pxsom_train_online_ex with oracle.som_online, the metric
trainers with tests/metric_reference.py som_online.  No tolerance, no case skipped."""
import numpy as np
import pytest
import torch

from tests import online_routes as orr
from tests.test_gpu_fuzz_parity import TORCH_DT
from tests.test_online_routes import SEED

pytestmark = pytest.mark.gpu


def _run(case, dev):
    from ark_analysis_amd import som_device
    from ark_analysis_amd.flowsom import default_radius_range
    n, c, off, pad = case["n"], case["c"], case["off"], case["pad"]
    tag = orr.tag(case, SEED)
    r = som_device.train_online_route(c, case["xdim"], case["ydim"], orr.DTYPE_CODE[case["dtype"]], case["metric"])
    assert (r["family"], r["width"], r["span"], r["in_place"]) == case["form"] and r["chunk"] == case["chunk"], \
        tag + ": the library routes this shape to %r" % (r,)
    buf = torch.zeros((n, off + c + pad), dtype=TORCH_DT[case["dtype"]])
    buf[:, off:off + c] = torch.from_numpy(case["x"])
    x = buf.to(dev)[:, off:off + c]                                       # a strided view at a column offset
    assert np.array_equal(x.cpu().to(torch.float64).numpy(), case["host"]), tag + ": upload"
    w = torch.from_numpy(case["w0"].copy()).to(dev)
    alpha, radius = (0.05, 0.01), default_radius_range(case["xdim"], case["ydim"])
    som_device.train_online(x, w, case["xdim"], case["ydim"], case["rlen"], alpha, radius,
                            torch.from_numpy(case["order"]).to(dev), int_abs=case["int_abs"], metric=case["metric"])
    return w.cpu().numpy(), alpha, radius, tag


def _assert_bits(got, want, tag):
    diff = got.view(np.int64) != want.view(np.int64)
    assert not diff.any(), tag + ": %d of %d values differ, first at (node, channel) %s" % (
        int(diff.sum()), diff.size, np.argwhere(diff)[:3].tolist())


def test_every_euclidean_form_and_storage_type(gpu, oracle):
    table = orr.forms(orr.EUCLIDEAN)
    ran, fired = set(), set()
    for case in orr.cases(SEED, "euclidean"):
        got, alpha, radius, tag = _run(case, gpu)
        variant = oracle.V_INT_ABS if case["int_abs"] else 0
        args = (case["host"], case["w0"], case["xdim"], case["ydim"], case["rlen"], alpha, radius, case["order"])
        want = oracle.som_online(*args, variant=variant)
        _assert_bits(got, want, tag)
        if case["stop"]:
            full = oracle.som_online(*args, variant=variant | oracle.V_NO_EARLY_STOP)
            assert not np.array_equal(want, full), tag + ": the early stop did not fire"
            fired.add((case["form"][0], case["stop"]))
        ran.add((case["form"], case["dtype"]))
    assert ran == {(f, d) for f in table for d in orr.DTYPES}
    assert fired == {(family, stop) for family in (0, 1) for stop in ("int_abs", "fabs")}
    print("\nonline routes, Euclidean: %d forms x %d storage types, %d cases" % (len(table), len(orr.DTYPES), case["i"] + 1))


def test_every_metric_form_and_storage_type(gpu):
    from tests import metric_reference as mr
    table = orr.forms(orr.METRICS[0])
    ran, fired = set(), set()
    for case in orr.cases(SEED + 1, "metric"):
        got, alpha, radius, tag = _run(case, gpu)
        args = (case["host"], case["w0"], case["xdim"], case["ydim"], case["rlen"], alpha, radius, case["order"], case["metric"])
        want = mr.som_online(*args, int_abs=case["int_abs"])
        _assert_bits(got, want, tag)
        if case["stop"] == "int_abs":           # the reference has no switch for the stop: the other reading runs on
            assert not np.array_equal(want, mr.som_online(*args, int_abs=False)), tag + ": the early stop did not fire"
            fired.add(case["form"])
        ran.add((case["form"], case["dtype"], case["metric"]))
    assert {(f, d) for f, d, _ in ran} == {(f, d) for f in table for d in orr.DTYPES}
    assert {(f, m) for f, _, m in ran} == {(f, m) for f in table for m in orr.METRICS}
    assert fired == set(table)
    print("\nonline routes, metrics 1/3/4: %d forms x %d storage types, %d cases" % (len(table), len(orr.DTYPES), case["i"] + 1))


@pytest.mark.parametrize("metric", (orr.EUCLIDEAN,) + orr.METRICS)
def test_shapes_past_the_limits_raise(gpu, metric):
    from ark_analysis_amd import _capi, som_device
    for c, xdim, ydim in orr.unsupported_shapes():
        for dtype in orr.DTYPES:
            x = torch.zeros((3, c), dtype=TORCH_DT[dtype], device=gpu)
            w = torch.zeros((xdim * ydim, c), dtype=torch.float64, device=gpu)
            order = torch.zeros(3, dtype=torch.int64, device=gpu)
            with pytest.raises(_capi.PxsomError):
                som_device.train_online_route(c, xdim, ydim, orr.DTYPE_CODE[dtype], metric)
            with pytest.raises(_capi.PxsomError):
                som_device.train_online(x, w, xdim, ydim, 1, (0.05, 0.01), (1.0, 0.0), order, metric=metric)
            assert not w.any().item(), "a refused call wrote the codebook"
