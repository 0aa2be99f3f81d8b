"""The launch forms of the exact online SOM trainers, as the library's own planning function reports them, and a
deterministic case list that visits every form with every storage type.  TEST INFRASTRUCTURE (numpy only; the library is
asked through som_device.train_online_routes, which runs no GPU call).

A *form* is what pxsom_train_online_route calls (family, width, span, in_place): one kernel instantiation per row type.
``forms(metric)`` sweeps every (K, c) in [1, 1024]^2 and groups the points by form, so the set of forms is whatever the
library can launch today -- nothing here names a form.  ``cases(seed, metric_class)`` then walks each form's region:
its corners in (K, c), the point of its largest LDS plan and of its smallest chunk, K = 1 and a K off the multiples of
64 where the region has them; row counts around the plan's own chunk; rlen 1 and 2; both readings of the early-stop
accumulator, with runs where the stop fires; strided row views; every value kind but "wild".
"""
import functools

import numpy as np

from tests.test_gpu_fuzz_parity import _rows, _storage

DTYPES = ("f16", "f32", "f64")
DTYPE_CODE = {"f32": 0, "f64": 1, "f16": 2}          # include/pxsom.h pxsom_dtype
EUCLIDEAN, METRICS = 2, (1, 3, 4)
LIMIT = 1024                                           # PXSOM_MAX_NODES == PXSOM_MAX_CHANNELS
KINDS = ("mixture", "blob", "quantised", "sparse", "range")
N_KINDS = ("one", "chunk-1", "chunk", "chunk+1", "2chunk+1", "hundreds")
FAMILY_NAME = {0: "lanes", 1: "thread"}


def form_name(form):
    family, width, span, in_place = form
    return "%s[%dx%d%s]" % (FAMILY_NAME.get(family, "?"), width, span, ",in-place" if in_place else "")


def sweep(metric, dtype="f32"):
    """(K [1024, 1024], c [1024, 1024], records [1024, 1024, 8]) of the query over the whole domain, grid K x 1."""
    from ark_analysis_amd import som_device
    k, c = np.meshgrid(np.arange(1, LIMIT + 1), np.arange(1, LIMIT + 1), indexing="ij")
    shapes = np.stack([c.ravel(), k.ravel(), np.ones(k.size, dtype=np.int64), np.full(k.size, DTYPE_CODE[dtype]),
                       np.full(k.size, metric)], axis=1)
    return k, c, som_device.train_online_routes(shapes).reshape(LIMIT, LIMIT, 8)


@functools.lru_cache(maxsize=None)
def forms(metric):
    """{form: dict(k, c, chunk, lds, threads -- 1-D arrays over the form's points, K-major)} for one metric."""
    k, c, rec = sweep(metric)
    ok = rec[..., 0] == 0
    out = {}
    key = rec[..., 1:5].reshape(-1, 4)
    uniq, inv = np.unique(key[ok.ravel()], axis=0, return_inverse=True)
    inv = inv.ravel()
    kk, cc, flat = k.ravel()[ok.ravel()], c.ravel()[ok.ravel()], rec.reshape(-1, 8)[ok.ravel()]
    for i, f in enumerate(uniq):
        sel = inv == i
        out[tuple(int(v) for v in f)] = dict(k=kk[sel], c=cc[sel], threads=flat[sel, 5], chunk=flat[sel, 6], lds=flat[sel, 7])
    return out


def edge_points(region):
    """The (K, c, chunk) points of a form's region that a case must sit on, without repeats."""
    k, c = region["k"], region["c"]
    picks = []

    def add(sel, what):
        idx = np.flatnonzero(sel)
        for i in (idx[np.argmax(what[idx])], idx[np.argmin(what[idx])]):
            picks.append(int(i))

    add(k == k.max(), c)                    # the largest map of the form, widest and narrowest rows (the first point
                                            #  meets the one-row case: more nodes than rows)
    add(k == k.min(), c)                    # the smallest
    add(c == c.min(), k)                    # the narrowest rows, on the largest and the smallest map that has them
    add(c == c.max(), k)                    # the widest
    picks.append(int(np.argmax(region["lds"])))
    picks.append(int(np.argmin(region["chunk"])))
    odd = np.flatnonzero(k % 64 != 0)
    if odd.size:
        picks.append(int(odd[odd.size // 2]))
    seen, out = set(), []
    for i in picks:
        p = (int(k[i]), int(c[i]), int(region["chunk"][i]))
        if p[:2] not in seen:
            seen.add(p[:2])
            out.append(p)
    return out


def _grid(rs, k):
    """A factorisation xdim * ydim == k drawn over all of them (1 x k and k x 1 included)."""
    div = [d for d in range(1, k + 1) if k % d == 0]
    xdim = int(div[rs.randint(0, len(div))])
    return xdim, k // xdim


def _n_of(kind, chunk, big):
    return {"one": 1, "chunk-1": max(1, chunk - 1), "chunk": chunk, "chunk+1": chunk + 1, "2chunk+1": 2 * chunk + 1,
            "hundreds": big}[kind]


def cases(seed, metric_class):
    """The case list of one trainer: ``metric_class`` "euclidean" (pxsom_train_online_ex) or "metric"
    (pxsom_train_online_metric; the metric of a case rotates over 1, 3, 4 with the storage type, so every form meets all
    three).  Every form gets at least nine cases -- three per storage type -- and one per edge point."""
    rs = np.random.RandomState(seed)
    table = forms(EUCLIDEAN if metric_class == "euclidean" else METRICS[0])
    i = 0
    for fi, form in enumerate(sorted(table)):
        points = edge_points(table[form])
        count = 3 * ((max(9, len(points)) + 2) // 3)
        for j in range(count):
            k, c, chunk = points[j % len(points)]
            dtype = DTYPES[(j + fi) % 3]
            metric = EUCLIDEAN if metric_class == "euclidean" else METRICS[(j // 3 + fi) % 3]
            # cases 1 and 2 of a form are runs whose early stop fires: under the integer reading (every |x - w| < 1 adds 0)
            # and under fabs (a pass that moves the codebook by less than 1 in total; binary16 cannot hold rows that small)
            stop = {1: "int_abs", 2: "int_abs" if dtype == "f16" else "fabs"}.get(j)
            n_kind = "hundreds" if stop else N_KINDS[(j + j // 6) % len(N_KINDS)]
            per_row = k * c if metric_class == "euclidean" else 40 * c     # the references: C loop | numpy per channel
            big = int(max(2 * chunk + 2, min(int(rs.randint(100, 400)), 3e8 / per_row if metric_class == "euclidean"
                                             else 4e4 / c)))
            n = _n_of(n_kind, chunk, big)
            rlen = 2 if stop else 1 + (j + j // 2) % 2
            int_abs = stop == "int_abs" or (stop is None and bool((j // 2 + fi) % 2))
            kind = "mixture" if stop else KINDS[(j + fi) % len(KINDS)]
            rows = _rows(rs, n, c, kind)
            if stop == "int_abs":
                rows = np.minimum(rows, 0.9)
            elif stop == "fabs":
                rows = rows * (0.25 / (max(1.0, rows.max()) * n * k * c))
            elif int_abs:
                rows = rows * 3.0                                          # differences on both sides of 1
            stored, host, off, pad = _storage(rs, rows, dtype)
            xdim, ydim = _grid(rs, k)
            w0 = np.ascontiguousarray(host[rs.choice(n, k, replace=n < k)])   # k > n: duplicated initial nodes
            order = rs.randint(0, n, size=n * rlen).astype(np.int64)          # (drawn with repeats)
            yield dict(i=i, form=form, metric=metric, dtype=dtype, xdim=xdim, ydim=ydim, k=k, c=c, chunk=chunk, n=n,
                       n_kind=n_kind, rlen=rlen, int_abs=int_abs, stop=stop, kind=kind, x=stored, host=host, w0=w0,
                       order=order, off=off, pad=pad)
            i += 1


def unsupported_shapes():
    """(c, xdim, ydim) past the limits of the trainers: each must raise and must never get a plan."""
    return [(LIMIT + 1, 1, 1), (LIMIT + 1, 10, 10), (1, LIMIT + 1, 1), (1, 1, LIMIT + 1), (8, 33, 32), (24, 32, 33),
            (LIMIT + 1, 33, 32), (2000, 5, 5), (16, 1, 2048)]


def tag(case, seed):
    return "case %d: form=%s metric=%d %s grid=%dx%d (K=%d) c=%d chunk=%d n=%d (%s) rlen=%d int_abs=%s stop=%s %s " \
           "off=%d pad=%d (seed %d)" % (case["i"], form_name(case["form"]), case["metric"], case["dtype"], case["xdim"],
                                        case["ydim"], case["k"], case["c"], case["chunk"], case["n"], case["n_kind"],
                                        case["rlen"], case["int_abs"], case["stop"], case["kind"], case["off"],
                                        case["pad"], seed)
