// pxsom_assign_sums.hip -- labels + per-cluster tables in ONE pass over x (pxsom_assign_sums, pxsom_assign_means).
#include "pxsom_assign.h"

// ------------------------------------------------------------------------------------------------
// labels + per-cluster sums / counts in ONE pass over x (pxsom_assign_sums): for the register-resident shapes the
// accumulating filter (labels, listed rows settled in binary64 inside the launch, per-workgroup binary64 tables) leaves
// [k*c sums | k counts as binary64] in a scratch region behind the assign workspace; a small kernel adds them into the
// caller's tables.  Other shapes: pxsom_assign, then pxsom_cluster_sums.
// ------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void stats_to_tables_kernel(double *__restrict__ stats, int k, int c, double *sums,
                                                              long long *counts)
{
    // (every element is read by exactly one thread, which clears it: the statistics region is left zero, include/pxsom.h)
    for (int e = blockIdx.x * 256 + threadIdx.x; e < k * c + k; e += gridDim.x * 256) {
        if (e < k * c) sums[e] += stats[e];
        else counts[e - k * c] += (long long)stats[e];
        stats[e] = 0.0;
    }
}

// the same, OVERWRITING the caller's tables and forming the means (pxsom_assign_means)
__global__ __launch_bounds__(256) void stats_to_means_kernel(double *__restrict__ stats, int k, int c, double *sums,
                                                             long long *counts, double *means, int *done)
{
    for (int e = blockIdx.x * 256 + threadIdx.x; e < k * c + k; e += gridDim.x * 256) {
        if (e < k * c) {
            const double s = stats[e], cnt = stats[(size_t)k * c + e / c];
            sums[e] = s;
            if (means) means[e] = s / (cnt > 0.0 ? cnt : 1.0);
        } else {
            counts[e - k * c] = (long long)stats[e];
        }
    }
    // the counts are read by the threads of the sums too: the region is cleared by the LAST workgroup to finish (a ticket in the
    // word behind the statistics), so that it is left zero (include/pxsom.h)
    __shared__ int s_last;
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (s_last) {
        for (int e = threadIdx.x; e < k * c + k; e += 256) stats[e] = 0.0;
        if (threadIdx.x == 0) *done = 0;
    }
}
__global__ __launch_bounds__(256) void tables_to_means_kernel(const double *__restrict__ sums, const long long *__restrict__ counts,
                                                              int k, int c, double *means)
{
    for (int e = blockIdx.x * 256 + threadIdx.x; e < k * c; e += gridDim.x * 256) {
        const long long cnt = counts[e / c];
        means[e] = sums[e] / (double)(cnt > 0 ? cnt : 1);
    }
}
}  // namespace

PXSOM_EXPORT size_t pxsom_assign_sums_scratch_bytes(int c, int k)
{
    if (c < 1 || c > PXSOM_MAX_CHANNELS || k < 1 || k > PXSOM_MAX_NODES) return 0;
    return pxsom::align_up((size_t)k * (c + 1) * sizeof(double), 256) + 256;
}

PXSOM_EXPORT size_t pxsom_assign_sums_workspace_bytes(int64_t n, int c, int k)
{
    const size_t a = pxsom_assign_workspace_bytes(n, c, k);
    // [statistics | 256 bytes: the ticket word of the launch that finishes the tables itself] [assign workspace]: the statistics
    // region sits at the START, where it does not move with n (pxsom_assign_sums_scratch_bytes)
    return a ? pxsom_assign_sums_scratch_bytes(c, k) + pxsom::align_up(a, 256) : 0;
}

namespace {
// What pxsom_assign_sums and pxsom_assign_means share: the argument checks, the carving of the workspace, the clearing of the
// statistics (+ ticket) unless the caller vouches for them, and the tables the accumulating launch may finish itself.
struct TablesCall {
    double *scratch;     // [statistics | ticket], at the start of the workspace
    void *assign_dev;    // the assign workspace behind them
    size_t assign_ws;
    pxsom_bmu::FinishTables fin;
};
int tables_call(const char *fn, const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, void *workspace_dev, size_t workspace_bytes, int flags,
                hipStream_t st, TablesCall *t)
{
    int rc = pxsom::check_matrix(fn, x_dev, n, c, ldx, dtype);
    if (rc) return rc;
    if (k < 1 || k > PXSOM_MAX_NODES) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: k=%d outside [1, %d]", fn, k, PXSOM_MAX_NODES);
    if (!w_dev || !sums_dev || !counts_dev || (n > 0 && !labels_dev)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    const size_t need = pxsom_assign_sums_workspace_bytes(n, c, k);
    if (!workspace_dev || workspace_bytes < need)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    const size_t scratch_bytes = pxsom_assign_sums_scratch_bytes(c, k), stats_bytes = scratch_bytes - 256;
    t->scratch = reinterpret_cast<double *>(workspace_dev);
    t->assign_dev = reinterpret_cast<char *>(workspace_dev) + scratch_bytes;
    t->assign_ws = workspace_bytes - scratch_bytes;
    // cleared ahead of the empty case too: a caller may pass the flag again after any successful call, an empty one included
    if (!(flags & PXSOM_TABLES_SCRATCH_CLEAN)) PXSOM_HIP_TRY(hipMemsetAsync(t->scratch, 0, scratch_bytes, st));   // statistics + ticket
    t->fin.sums = sums_dev;
    t->fin.counts = reinterpret_cast<long long *>(counts_dev);
    t->fin.ticket = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(t->scratch) + stats_bytes);
    return PXSOM_OK;
}
}  // namespace

PXSOM_EXPORT int pxsom_assign_sums(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                                   int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, void *workspace_dev,
                                   size_t workspace_bytes, void *stream)
{
    return pxsom_assign_sums_ex(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, sums_dev, counts_dev, workspace_dev, workspace_bytes, 0, stream);
}

PXSOM_EXPORT int pxsom_assign_sums_ex(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                                      int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, void *workspace_dev,
                                      size_t workspace_bytes, int flags, void *stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    TablesCall t;
    int rc = tables_call("pxsom_assign_sums", x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, sums_dev, counts_dev, workspace_dev,
                         workspace_bytes, flags, st, &t);
    if (rc) return rc;
    if (n == 0) return PXSOM_OK;
    bool fused = false;
    rc = pxsom_bmu::assign_accumulate(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, t.scratch, t.assign_dev, t.assign_ws, st,
                                      &fused, &t.fin);
    if (rc) return rc;
    if (fused && t.fin.done) return PXSOM_OK;   // the last workgroup of the launch added the statistics into the tables (and cleared them)
    if (fused) {
        hipLaunchKernelGGL(stats_to_tables_kernel, dim3((k * (c + 1) + 255) / 256), dim3(256), 0, st, t.scratch, k, c, sums_dev,
                           reinterpret_cast<long long *>(counts_dev));
        PXSOM_LAUNCH_CHECK("stats_to_tables_kernel");
        return PXSOM_OK;
    }
    rc = pxsom_assign(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, nullptr, t.assign_dev, t.assign_ws, stream);
    if (rc) return rc;
    return pxsom_cluster_sums(x_dev, n, c, ldx, dtype, labels_dev, k, sums_dev, counts_dev, stream);
}

PXSOM_EXPORT int pxsom_assign_means(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                                    int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, double *means_dev,
                                    void *workspace_dev, size_t workspace_bytes, void *stream)
{
    return pxsom_assign_means_ex(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, sums_dev, counts_dev, means_dev, workspace_dev,
                                 workspace_bytes, 0, stream);
}

PXSOM_EXPORT int pxsom_assign_means_ex(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                                       int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, double *means_dev,
                                       void *workspace_dev, size_t workspace_bytes, int flags, void *stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    TablesCall t;
    int rc = tables_call("pxsom_assign_means", x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, sums_dev, counts_dev, workspace_dev,
                         workspace_bytes, flags, st, &t);
    if (rc) return rc;
    t.fin.means = means_dev;
    t.fin.overwrite = 1;
    const unsigned fgrid = (unsigned)((k * (c + 1) + 255) / 256);
    bool fused = false;
    if (n > 0) {
        rc = pxsom_bmu::assign_accumulate(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, t.scratch, t.assign_dev, t.assign_ws, st,
                                          &fused, &t.fin);
        if (rc) return rc;
    }
    if (fused && t.fin.done) return PXSOM_OK;   // the last workgroup of the launch wrote the three tables (and cleared the statistics)
    if (fused || n == 0) {   // one launch writes the three tables
        hipLaunchKernelGGL(stats_to_means_kernel, dim3(fgrid), dim3(256), 0, st, t.scratch, k, c, sums_dev,
                           reinterpret_cast<long long *>(counts_dev), means_dev, reinterpret_cast<int *>(t.fin.ticket));
        PXSOM_LAUNCH_CHECK("stats_to_means_kernel");
        return PXSOM_OK;
    }
    PXSOM_HIP_TRY(hipMemsetAsync(sums_dev, 0, (size_t)k * c * sizeof(double), st));
    PXSOM_HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)k * sizeof(int64_t), st));
    rc = pxsom_assign(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, nullptr, t.assign_dev, t.assign_ws, stream);
    if (rc) return rc;
    rc = pxsom_cluster_sums(x_dev, n, c, ldx, dtype, labels_dev, k, sums_dev, counts_dev, stream);
    if (rc || !means_dev) return rc;
    hipLaunchKernelGGL(tables_to_means_kernel, dim3(fgrid), dim3(256), 0, st, sums_dev, reinterpret_cast<const long long *>(counts_dev), k, c,
                       means_dev);
    PXSOM_LAUNCH_CHECK("tables_to_means_kernel");
    return PXSOM_OK;
}
