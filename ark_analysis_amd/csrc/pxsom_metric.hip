// pxsom_metric.hip -- BMU assignment for FlowSOM's other distances (distf 1 Manhattan, 3 Chebyshev, 4 cosine):
// pxsom_assign_metric (include/pxsom.h; DESIGN.md "K7m").
//
// Every (row, node) pair is evaluated in binary64 in the oracle's order (pxsom_metric.h); there is no screen, so the
// result is the table of pxsom.h bit for bit by construction, ties and NaN included.  The prepared codebook and the search of a
// wave's rows are pxsom_metric_bmu.h's (shared with pxsom_metric_step.hip, which adds the batch statistics to the same search).
#include "pxsom_metric_bmu.h"

namespace {

using namespace pxsom_metric;

// CX > 0: rows of c <= CX channels, converted once into registers; CX == 0: any width, staged in LDS per chunk
// (staged rows: at least kStagedWavesPerSimd waves per SIMD -- the register budget these kernels had before the search moved to
// pxsom_metric_bmu.h, which the allocator no longer finds by itself for binary64 rows)
template <int M, typename T, int CX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CX > 0 ? 1 : kStagedWavesPerSimd))) void bmu_metric_kernel(const T *__restrict__ x, int64_t n, int c, int64_t ldx,
                                                         const double *__restrict__ wt, const double *__restrict__ wn,
                                                         int k, int kp, int32_t *__restrict__ labels,
                                                         double *__restrict__ dist)
{
    extern __shared__ double stage_raw[];
    const int lane = threadIdx.x & 63;
    double *xs = stage_raw + (threadIdx.x >> 6) * (kStageCh * kStageLd);   // this wave's [kStageCh][kStageLd] chunk
    const int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63);
    // wave-uniform loop: the last wave's idle lanes work on row n - 1 and store nothing
    for (int64_t base = wave0; base < n; base += (int64_t)gridDim.x * 256) {
        const int64_t row = base + lane;
        double xr[CX > 0 ? CX : 1], best;
        const int bk = bmu_search<M, T, CX, kStageCh>(x, ldx, c, [&](int r) { return base + r < n ? base + r : n - 1; }, lane, xs,
                                                      wt, wn, k, kp, xr, &best);
        if (row < n) {
            labels[row] = bk + 1;
            if (dist) dist[row] = best;
        }
    }
}

template <int M, typename T>
int assign_metric_typed(const T *x, int64_t n, int c, int64_t ldx, const double *w, int k, int32_t *labels,
                        double *dist, char *ws, hipStream_t st)
{
    Prepared p;
    int rc = launch_metric_prep(w, k, c, M, ws, (unsigned)n, st, &p);
    if (rc) return rc;
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)pxsom::device_cu_count() * 8));
    const bool reg = c <= kRegChannels;
    auto kern = reg ? bmu_metric_kernel<M, T, kRegChannels> : bmu_metric_kernel<M, T, 0>;
    const size_t lds = reg ? 0 : stage_bytes(kStageCh);
    pxsom::Prof *prof = pxsom::current_prof();
    pxsom::prof_mark(prof, st, true, n);
    PXSOM_TIMED_LAUNCH(kern, dim3((unsigned)grid), dim3(256), lds, st, x, n, c, ldx, p.wt, p.wn, k, p.kp, labels, dist);
    pxsom::prof_mark(prof, st, false, n);
    PXSOM_LAUNCH_CHECK("bmu_metric_kernel");
    return PXSOM_OK;
}

template <int M>
int assign_metric(const void *x, int64_t n, int c, int64_t ldx, int dtype, const double *w, int k, int32_t *labels,
                  double *dist, char *ws, hipStream_t st)
{
    PXSOM_DISPATCH_DTYPE(dtype, x, xp, (assign_metric_typed<M, T>(xp, n, c, ldx, w, k, labels, dist, ws, st)));
}

}  // namespace

PXSOM_EXPORT size_t pxsom_assign_metric_workspace_bytes(int64_t n, int c, int k, int metric)
{
    if (metric == PXSOM_METRIC_EUCLIDEAN) return pxsom_assign_workspace_bytes(n, c, k);
    if (!metric_known(metric) || n < 0 || c < 1 || c > PXSOM_MAX_CHANNELS || k < 1 || k > PXSOM_MAX_NODES) return 0;
    return metric_workspace_bytes(c, k);
}

PXSOM_EXPORT int pxsom_assign_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev,
                                     int k, int32_t *labels_dev, double *dist_dev, void *workspace_dev,
                                     size_t workspace_bytes, int metric, void *stream)
{
    if (!metric_known(metric))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG,
                           "pxsom_assign_metric: unknown metric %d (FlowSOM distf: 1 Manhattan, 2 Euclidean, 3 Chebyshev, "
                           "4 cosine)", metric);
    if (metric == PXSOM_METRIC_EUCLIDEAN)
        return pxsom_assign(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, dist_dev, workspace_dev, workspace_bytes, stream);
    if (n < 0 || n > 0x7fffffffLL)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_metric: n=%lld outside [0, 2^31)", (long long)n);
    if (c < 1 || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_metric: c=%d outside [1, %d]", c, PXSOM_MAX_CHANNELS);
    if (k < 1 || k > PXSOM_MAX_NODES)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_metric: k=%d outside [1, %d]", k, PXSOM_MAX_NODES);
    if (ldx < c) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_metric: ldx=%lld < c=%d", (long long)ldx, c);
    if (!pxsom::dtype_ok(dtype)) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_metric: dtype %d", dtype);
    if (!w_dev || (n > 0 && (!x_dev || !labels_dev)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_metric: null pointer");
    const size_t need = metric_workspace_bytes(c, k);
    if (!workspace_dev || workspace_bytes < need)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "pxsom_assign_metric: workspace %zu < %zu bytes", workspace_bytes, need);
    if (pxsom::row_view_active())
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_metric: the metric kernels do not take row views");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = reinterpret_cast<char *>(workspace_dev);
    if (n == 0) {
        PXSOM_HIP_TRY(hipMemsetAsync(ws, 0, kHdrBytes, st));
        return PXSOM_OK;
    }
    switch (metric) {
    case PXSOM_METRIC_MANHATTAN: return assign_metric<PXSOM_METRIC_MANHATTAN>(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, dist_dev, ws, st);
    case PXSOM_METRIC_CHEBYSHEV: return assign_metric<PXSOM_METRIC_CHEBYSHEV>(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, dist_dev, ws, st);
    default: return assign_metric<PXSOM_METRIC_COSINE>(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, dist_dev, ws, st);
    }
}
