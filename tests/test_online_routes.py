"""The route table of the online SOM trainers (csrc/pxsom_online.h plan_online, asked through pxsom_train_online_route)
on CPU: what the plan promises holds on every (K, c) of the domain for every metric and storage type, shapes past the
limits get the training call's own error and no plan, and the case list of tests/online_routes.py -- what
test_gpu_online_routes.py runs -- covers every form the library can launch with every storage type.  The set of forms is
read from the library here, so a rung added to the table without a case fails on CPU."""
import ctypes

import numpy as np
import pytest

from tests import online_routes as orr
from tests import test_gpu_fuzz_parity as fp
from tests.test_fuzz_generators import _same_cases

SEED = 20261017
ALL_METRICS = (orr.EUCLIDEAN,) + orr.METRICS
# the bounds of the table as DESIGN.md "K6a" states it: a form changes between c | c + 1 and between K | K + 1 here and
# nowhere else (the in-place variants aside: their bound is the LDS budget, a curve in K * c)
C_BOUNDS = {orr.EUCLIDEAN: {8, 16, 24, 40, 64, 80, 104}, "metric": {8, 16, 24, 40, 64}}
K_BOUNDS = {orr.EUCLIDEAN: {64, 128, 256, 512}, "metric": {256, 512}}


def _lib():
    from ark_analysis_amd import _capi
    return _capi.lib()


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_plan_keeps_its_promises_on_the_whole_domain(metric):
    per_dtype = {}
    for dtype in orr.DTYPES:
        k, c, rec = orr.sweep(metric, dtype)
        status, family, width, span, in_place, threads, chunk, lds = (rec[..., i].astype(np.int64) for i in range(8))
        assert (status == 0).all(), "unsupported inside the limits: K=%d c=%d" % (k[status != 0][0], c[status != 0][0])
        lanes = family == 0
        assert ((family == 0) | (family == 1)).all()
        assert (threads % 64 == 0).all() and (threads <= 1024).all()
        assert (threads >= np.where(lanes, k * span, k)).all()
        assert (threads <= np.where(lanes, np.where(width * span > 40, 512, 256), span)).all(), "past __launch_bounds__"
        assert (width[lanes] * span[lanes] >= c[lanes]).all()
        reg = ~lanes & (width > 0)
        assert (width[reg] >= c[reg]).all()
        assert ((chunk >= 1) & (chunk <= 64) & (chunk & (chunk - 1) == 0)).all()
        assert ((chunk * c + threads - 1) // threads <= 16).all(), "more gather registers than the kernels hold"
        assert ((lds > 0) & (lds <= 160 * 1024)).all()
        assert (k[lanes] <= 128).all(), "the lanes-per-node kernel exchanges 128 distance slots"
        # what each kernel lays out in LDS (pxsom_online.h) fits the bytes the plan asks for
        nwv = threads // 64
        ring = 2 * chunk * np.where(lanes, width * span, np.where(width > 0, width, c)) * 8
        need_thread = np.where((width == 0) & (in_place == 0), c * k * 8, 0) + ring + 32 * nwv + 16 * chunk
        need_lanes = ring + (3 * 128 + 8) * 8 + chunk * 8 + 2 * chunk * 8 + (width * span + 2) * 8
        assert (np.where(lanes, need_lanes, need_thread) <= lds).all()
        # in place only where the codebook-in-LDS plan does not fit: CMAX 0, and the codebook beside the smallest ring
        # the gather allows is past the 160 KiB of a workgroup
        assert (in_place[lanes | reg] == 0).all()
        free = ~lanes & (width == 0)
        chunk_lds = np.full(k.shape, 64)
        fixed = c * k * 8 + 32 * nwv + 2 * 64 * 8 + 64
        for _ in range(3):
            chunk_lds = np.where((chunk_lds > 8) & (fixed + 2 * chunk_lds * c * 8 > 150 * 1024), chunk_lds // 2, chunk_lds)
        for _ in range(7):
            chunk_lds = np.where((chunk_lds * c + threads - 1) // threads > 16, chunk_lds // 2, chunk_lds)
        fits = (chunk_lds >= 1) & (fixed + 2 * chunk_lds * c * 8 <= 160 * 1024)
        assert np.array_equal(in_place[free] == 1, ~fits[free])
        per_dtype[dtype] = rec
    for dtype in orr.DTYPES[1:]:
        assert np.array_equal(per_dtype[dtype], per_dtype[orr.DTYPES[0]]), "the storage type changed the route"


def test_the_three_metrics_share_one_table():
    want = orr.sweep(orr.METRICS[0])[2]
    for metric in orr.METRICS[1:]:
        assert np.array_equal(orr.sweep(metric)[2], want)
    assert {f[0] for f in orr.forms(orr.METRICS[0])} == {1}, "a metric trainer took the lanes-per-node kernel"
    assert {f[0] for f in orr.forms(orr.EUCLIDEAN)} == {0, 1}


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_route_depends_on_the_node_count_alone(metric):
    from ark_analysis_amd import som_device
    rs = np.random.RandomState(SEED + metric)
    shapes = []
    for k in [1, 2, 36, 64, 100, 128, 144, 256, 400, 512, 576, 1024] + [int(v) for v in rs.randint(1, 1025, 40)]:
        for xdim in [d for d in range(1, k + 1) if k % d == 0]:
            for c in (1, 8, 9, 24, 25, 40, 41, 64, 65, 104, 105, 300, 1024, int(rs.randint(1, 1025))):
                shapes.append((c, xdim, k // xdim, 0, metric))
    shapes = np.array(shapes)
    got = som_device.train_online_routes(shapes)
    flat = som_device.train_online_routes(np.stack([shapes[:, 0], shapes[:, 1] * shapes[:, 2], np.ones(len(shapes), dtype=int),
                                                    shapes[:, 3], shapes[:, 4]], axis=1))
    assert np.array_equal(got, flat) and (got[:, 0] == 0).all()
    one = som_device.train_online_route(22, 10, 10, metric=metric)      # the single query is the batched one
    assert [0] + [one[f] for f in som_device.ONLINE_ROUTE_FIELDS] == list(
        som_device.train_online_routes([[22, 10, 10, 0, metric]])[0])


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_table_bounds_are_the_documented_ones(metric):
    """Where the form (in-place aside) changes along c and along K.  A rung moved by one shows up here."""
    rec = orr.sweep(metric)[2][..., 1:4]
    along_c = np.flatnonzero((rec[:, 1:] != rec[:, :-1]).any(axis=(0, 2))) + 1
    along_k = np.flatnonzero((rec[1:] != rec[:-1]).any(axis=(1, 2))) + 1
    key = metric if metric == orr.EUCLIDEAN else "metric"
    assert set(along_c.tolist()) == C_BOUNDS[key]
    assert set(along_k.tolist()) == K_BOUNDS[key]


def _train_entry_error(c, xdim, ydim, dtype, metric):
    """(status, message) of the training entry itself on a shape it refuses (refused before any HIP call)."""
    lib = _lib()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    if metric == orr.EUCLIDEAN:
        rc = lib.pxsom_train_online_ex(p, 1, c, max(c, 1), dtype, p, xdim, ydim, 1, 0.05, 0.01, 1.0, 0.0, p, 0, None)
    else:
        rc = lib.pxsom_train_online_metric(p, 1, c, max(c, 1), dtype, p, xdim, ydim, 1, 0.05, 0.01, 1.0, 0.0, p, metric, 0, None)
    return rc, lib.pxsom_last_error()


def test_shapes_past_the_limits_get_the_trainers_error_and_no_plan():
    from ark_analysis_amd import _capi, som_device
    lib = _lib()
    bad = [(c, x, y, 0) for c, x, y in orr.unsupported_shapes()]
    bad += [(0, 3, 3, 0), (-5, 3, 3, 0), (8, 0, 5, 0), (8, 5, 0, 0), (8, -1, -1, 0), (8, 65536, 65536, 0),
            (8, 3, 3, 3), (8, 3, 3, -1), (1025, 3, 3, 9)]
    for metric in ALL_METRICS:
        for c, xdim, ydim, dtype in bad:
            out = np.full(7, 12345, dtype=np.int32)
            rc = lib.pxsom_train_online_route(c, xdim, ydim, dtype, metric, out.ctypes.data)
            msg = lib.pxsom_last_error()
            assert rc == -2 and (out == -1).all(), (metric, c, xdim, ydim, dtype, rc, out)
            assert (rc, msg) == _train_entry_error(c, xdim, ydim, dtype, metric), (metric, c, xdim, ydim, dtype, msg)
            with pytest.raises(_capi.PxsomError):
                som_device.train_online_route(c, xdim, ydim, dtype, metric)
            row = som_device.train_online_routes([[c, xdim, ydim, dtype, metric]])[0]
            assert row[0] == rc and (row[1:] == -1).all()
    for metric in (0, 5, -2, 77):                                       # an unknown metric: the metric entry's error
        out = np.full(7, 12345, dtype=np.int32)
        rc = lib.pxsom_train_online_route(8, 3, 3, 0, metric, out.ctypes.data)
        msg = lib.pxsom_last_error()
        assert rc == -1 and (out == -1).all()
        assert (rc, msg) == _train_entry_error(8, 3, 3, 0, metric)
    assert lib.pxsom_train_online_route(8, 3, 3, 0, 2, None) == -1
    assert lib.pxsom_abi_version() == _capi.ABI_VERSION == 9            # symbols added, none changed


def test_online_metric_route_is_the_librarys_rule():
    """The route classes of the fuzz generator (test_gpu_fuzz_parity.online_metric_route) over the whole domain."""
    k, c, rec = orr.sweep(orr.METRICS[0])
    width, in_place = rec[..., 2], rec[..., 4]
    want = np.where(width > 0, "register", np.where(in_place == 1, "in_place", "lds"))
    rs = np.random.RandomState(SEED)
    for kk, cc in [(1, 1), (256, 64), (256, 65), (257, 40), (257, 41), (512, 40), (513, 1), (1024, 1024), (264, 128),
                   (100, 150)] + [(int(a), int(b)) for a, b in rs.randint(1, 1025, size=(300, 2))]:
        assert fp.online_metric_route(kk, cc) == want[kk - 1, cc - 1], (kk, cc)
    for kk, cc in [(1025, 1), (1, 1025), (33 * 32, 8), (2000, 2000)]:
        assert fp.online_metric_route(kk, cc) == "unsupported"


@pytest.mark.parametrize("metric_class", ["euclidean", "metric"])
def test_case_list_covers_every_form_with_every_storage_type(metric_class):
    first, again = list(orr.cases(SEED, metric_class)), list(orr.cases(SEED, metric_class))
    _same_cases([{k: v for k, v in c.items() if k != "form"} for c in first],
                [{k: v for k, v in c.items() if k != "form"} for c in again])
    assert [c["form"] for c in first] == [c["form"] for c in again]
    metrics = (orr.EUCLIDEAN,) if metric_class == "euclidean" else orr.METRICS
    table = orr.forms(metrics[0])
    assert {(c["form"], c["dtype"]) for c in first} == {(f, d) for f in table for d in orr.DTYPES}
    assert {(c["form"], c["metric"]) for c in first} == {(f, m) for f in table for m in metrics}
    from ark_analysis_amd import som_device
    for c in first:                                        # each case lies in its form, at the chunk it was built around
        r = som_device.train_online_route(c["c"], c["xdim"], c["ydim"], orr.DTYPE_CODE[c["dtype"]], c["metric"])
        assert (r["family"], r["width"], r["span"], r["in_place"]) == c["form"] and r["chunk"] == c["chunk"], orr.tag(c, SEED)
        assert c["x"].shape == (c["n"], c["c"]) and c["w0"].shape == (c["k"], c["c"]) and c["xdim"] * c["ydim"] == c["k"]
        assert c["order"].shape == (c["n"] * c["rlen"],) and c["kind"] in orr.KINDS and 1 <= c["n"] < 1000
        assert np.isfinite(c["host"]).all() and np.array_equal(c["x"].astype(np.float64), c["host"])
    for form, region in table.items():
        mine = [c for c in first if c["form"] == form]
        tag = orr.form_name(form)
        kc = {(c["k"], c["c"]) for c in mine}
        for cs in (region["c"].min(), region["c"].max()):               # the form's narrowest and widest rows ...
            ks = region["k"][region["c"] == cs]
            assert {(ks.min(), cs), (ks.max(), cs)} <= kc, tag          # ... on its smallest and largest map there
        for ks in (region["k"].min(), region["k"].max()):
            cs = region["c"][region["k"] == ks]
            assert {(ks, cs.min()), (ks, cs.max())} <= kc, tag
        assert region["lds"].max() in {region["lds"][(region["k"] == k) & (region["c"] == c)][0] for k, c in kc}, tag
        assert region["chunk"].min() in {c["chunk"] for c in mine}, tag
        assert (region["k"] % 64 == 0).all() or any(c["k"] % 64 for c in mine), tag
        assert region["k"].min() > 1 or any(c["k"] == 1 for c in mine), tag
        assert {c["n_kind"] for c in mine} == set(orr.N_KINDS), tag
        for c in mine:
            q = c["chunk"]
            assert c["n"] == {"one": 1, "chunk-1": max(1, q - 1), "chunk": q, "chunk+1": q + 1, "2chunk+1": 2 * q + 1}.get(
                c["n_kind"], c["n"]), tag
        assert {c["rlen"] for c in mine} == {1, 2} and {c["int_abs"] for c in mine} == {False, True}, tag
        assert {(c["rlen"], c["int_abs"]) for c in mine} == {(1, False), (1, True), (2, False), (2, True)}, tag
        assert region["k"].max() == 1 or any(c["k"] > c["n"] for c in mine), tag
        assert any(c["off"] or c["pad"] for c in mine), tag + ": no strided row view"
        assert any(len(np.unique(c["order"])) < len(c["order"]) for c in mine), tag + ": no repeated row"
        assert len({c["kind"] for c in mine}) >= 4, tag
        assert {c["stop"] for c in mine} >= {None, "int_abs"}, tag
    assert {c["kind"] for c in first} == set(orr.KINDS)
    for family in {f[0] for f in table}:
        assert {c["stop"] for c in first if c["form"][0] == family} == {None, "int_abs", "fabs"}


def test_early_stop_fires_where_the_case_list_says(oracle):
    """Euclidean cases marked `stop`: the oracle without its early stop (V_NO_EARLY_STOP) ends elsewhere."""
    from ark_analysis_amd.flowsom import default_radius_range
    seen = 0
    for c in orr.cases(SEED, "euclidean"):
        if not c["stop"]:
            continue
        variant = oracle.V_INT_ABS if c["int_abs"] else 0
        ar, rr = (0.05, 0.01), default_radius_range(c["xdim"], c["ydim"])
        stopped = oracle.som_online(c["host"], c["w0"], c["xdim"], c["ydim"], c["rlen"], ar, rr, c["order"], variant=variant)
        full = oracle.som_online(c["host"], c["w0"], c["xdim"], c["ydim"], c["rlen"], ar, rr, c["order"],
                                 variant=variant | oracle.V_NO_EARLY_STOP)
        assert not np.array_equal(stopped, full), orr.tag(c, SEED)
        seen += 1
    assert seen >= 2 * len(orr.forms(orr.EUCLIDEAN))
