// pxsom_online.hip -- entry points of the exact online SOM (kernels: pxsom_online.h, one unit per row type).
//
//   pxsom_train_online  replaces pyFlowSOM.som: FlowSOM's C_SOM loop, n*rlen strictly sequential steps.
#include "pxsom_online.h"

namespace {

// arguments of an online training call; *nothing_to_do: valid, and no step to run (n == 0 or rlen == 0)
int check_online(const char *fn, const void *x, int64_t n, int c, int64_t ldx, int dtype, const double *w, int xdim,
                 int ydim, int rlen, const int64_t *order, int flags, bool *nothing_to_do)
{
    *nothing_to_do = false;
    int rc = pxsom::check_matrix(fn, x, n, c, ldx, dtype);
    if (rc) return rc;
    if (xdim < 1 || ydim < 1 || (int64_t)xdim * ydim > PXSOM_MAX_NODES)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: grid %dx%d outside [1, %d] nodes", fn, xdim, ydim, PXSOM_MAX_NODES);
    if (rlen < 0 || !w) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad rlen / null codebook", fn);
    if (flags & ~PXSOM_ONLINE_INT_ABS) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: unknown flags %d", fn, flags);
    if (n == 0 || rlen == 0) {
        *nothing_to_do = true;
        return PXSOM_OK;
    }
    if (!order) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null order", fn);
    return PXSOM_OK;
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
    if (metric < PXSOM_METRIC_MANHATTAN || metric > PXSOM_METRIC_COSINE)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG,
                           "pxsom_train_online_metric: unknown metric %d (FlowSOM distf: 1 Manhattan, 2 Euclidean, "
                           "3 Chebyshev, 4 cosine)", metric);
    if (metric == PXSOM_METRIC_EUCLIDEAN)
        return pxsom_train_online_ex(x_dev, n, c, ldx, dtype, w_dev, xdim, ydim, rlen, a0, a1, r0, r1, order_dev, flags, stream);
    bool nothing_to_do = false;
    int rc = check_online("pxsom_train_online_metric", x_dev, n, c, ldx, dtype, w_dev, xdim, ydim, rlen, order_dev, flags,
                          &nothing_to_do);
    if (rc || nothing_to_do) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_DISPATCH_DTYPE(dtype, x_dev, xp,
                         (pxsom::train_online<T>(xp, n, c, ldx, w_dev, xdim, ydim, rlen, a0, a1, r0, r1, order_dev, metric,
                                                 flags, st)));
}
