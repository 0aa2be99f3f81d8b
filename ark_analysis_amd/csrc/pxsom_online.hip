// pxsom_online.hip -- entry points of the exact online SOM (kernels: pxsom_online.h, one unit per row type).
//
//   pxsom_train_online  replaces pyFlowSOM.som: FlowSOM's C_SOM loop, n*rlen strictly sequential steps.
#include "pxsom_online.h"

namespace {

const char *entry_name(int metric) { return metric == PXSOM_METRIC_EUCLIDEAN ? "pxsom_train_online" : "pxsom_train_online_metric"; }

int check_metric(int metric)
{
    if (metric < PXSOM_METRIC_MANHATTAN || metric > PXSOM_METRIC_COSINE)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG,
                           "pxsom_train_online_metric: unknown metric %d (FlowSOM distf: 1 Manhattan, 2 Euclidean, "
                           "3 Chebyshev, 4 cosine)", metric);
    return PXSOM_OK;
}

int check_grid(const char *fn, int xdim, int ydim)
{
    if (xdim < 1 || ydim < 1 || (int64_t)xdim * ydim > PXSOM_MAX_NODES)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: grid %dx%d outside [1, %d] nodes", fn, xdim, ydim, PXSOM_MAX_NODES);
    return PXSOM_OK;
}

// arguments of an online training call; *nothing_to_do: valid, and no step to run (n == 0 or rlen == 0)
int check_online(const char *fn, const void *x, int64_t n, int c, int64_t ldx, int dtype, const double *w, int xdim,
                 int ydim, int rlen, const int64_t *order, int flags, bool *nothing_to_do)
{
    *nothing_to_do = false;
    int rc = pxsom::check_matrix(fn, x, n, c, ldx, dtype);
    if (rc) return rc;
    rc = check_grid(fn, xdim, ydim);
    if (rc) return rc;
    if (rlen < 0 || !w) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad rlen / null codebook", fn);
    if (flags & ~PXSOM_ONLINE_INT_ABS) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: unknown flags %d", fn, flags);
    if (n == 0 || rlen == 0) {
        *nothing_to_do = true;
        return PXSOM_OK;
    }
    if (!order) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null order", fn);
    return PXSOM_OK;
}

// The shape checks of a training call in the call's own order, then the plan the call would launch: what
// pxsom_train_online_route answers.  No HIP call.
int route_of(int c, int xdim, int ydim, int dtype, int metric, pxsom::OnlinePlan *p)
{
    int rc = check_metric(metric);
    if (rc) return rc;
    const char *fn = entry_name(metric);
    rc = pxsom::check_matrix(fn, p, 1, c, c, dtype);   // (any non-null pointer: the shape and the type are what is asked)
    if (rc) return rc;
    rc = check_grid(fn, xdim, ydim);
    if (rc) return rc;
    return pxsom::plan_online(xdim * ydim, c, metric, p);
}

void store_route(int rc, const pxsom::OnlinePlan &p, int32_t *out)
{
    const int32_t f[PXSOM_ONLINE_ROUTE_FIELDS] = {p.family, p.width, p.span, p.in_place, p.threads, p.chunk, p.lds_bytes};
    for (int i = 0; i < PXSOM_ONLINE_ROUTE_FIELDS; i++) out[i] = rc == PXSOM_OK ? f[i] : -1;   // an error leaves no plan
}

}  // namespace

PXSOM_EXPORT int pxsom_train_online_ex(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *w_dev,
                                       int xdim, int ydim, int rlen, double a0, double a1, double r0, double r1,
                                       const int64_t *order_dev, int flags, void *stream)
{
    bool nothing_to_do = false;
    int rc = check_online("pxsom_train_online", x_dev, n, c, ldx, dtype, w_dev, xdim, ydim, rlen, order_dev, flags,
                          &nothing_to_do);
    if (rc || nothing_to_do) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_DISPATCH_DTYPE(dtype, x_dev, xp,
                         (pxsom::train_online<T>(xp, n, c, ldx, w_dev, xdim, ydim, rlen, a0, a1, r0, r1, order_dev,
                                                 PXSOM_METRIC_EUCLIDEAN, flags, st)));
}

PXSOM_EXPORT int pxsom_train_online(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *w_dev,
                                    int xdim, int ydim, int rlen, double a0, double a1, double r0, double r1,
                                    const int64_t *order_dev, void *stream)
{
    return pxsom_train_online_ex(x_dev, n, c, ldx, dtype, w_dev, xdim, ydim, rlen, a0, a1, r0, r1, order_dev, 0, stream);
}

PXSOM_EXPORT int pxsom_train_online_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *w_dev,
                                           int xdim, int ydim, int rlen, double a0, double a1, double r0, double r1,
                                           const int64_t *order_dev, int metric, int flags, void *stream)
{
    int rc = check_metric(metric);
    if (rc) return rc;
    if (metric == PXSOM_METRIC_EUCLIDEAN)
        return pxsom_train_online_ex(x_dev, n, c, ldx, dtype, w_dev, xdim, ydim, rlen, a0, a1, r0, r1, order_dev, flags, stream);
    bool nothing_to_do = false;
    rc = check_online("pxsom_train_online_metric", x_dev, n, c, ldx, dtype, w_dev, xdim, ydim, rlen, order_dev, flags,
                          &nothing_to_do);
    if (rc || nothing_to_do) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_DISPATCH_DTYPE(dtype, x_dev, xp,
                         (pxsom::train_online<T>(xp, n, c, ldx, w_dev, xdim, ydim, rlen, a0, a1, r0, r1, order_dev, metric,
                                                 flags, st)));
}

PXSOM_EXPORT int pxsom_train_online_route(int c, int xdim, int ydim, int dtype, int metric, int32_t *out)
{
    if (!out) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_train_online_route: null record");
    pxsom::OnlinePlan p;
    const int rc = route_of(c, xdim, ydim, dtype, metric, &p);
    store_route(rc, p, out);
    return rc;
}

PXSOM_EXPORT int pxsom_train_online_routes(int64_t count, const int32_t *shapes, int32_t *out)
{
    if (count < 0 || (count > 0 && (!shapes || !out)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_train_online_routes: bad count / null table");
    for (int64_t i = 0; i < count; i++) {
        const int32_t *s = shapes + 5 * i;
        int32_t *o = out + (PXSOM_ONLINE_ROUTE_FIELDS + 1) * i;
        pxsom::OnlinePlan p;
        o[0] = route_of(s[0], s[1], s[2], s[3], s[4], &p);
        store_route(o[0], p, o + 1);
    }
    return PXSOM_OK;
}
