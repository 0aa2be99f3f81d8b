// pxsom_metric_step.hip -- labels AND batch statistics in one pass over the rows for FlowSOM's other distances (distf 1
// Manhattan, 3 Chebyshev, 4 cosine): pxsom_assign_sums_metric (include/pxsom.h; DESIGN.md "K6m").  The accumulation half of
// a batch step under these metrics (pxsom_batch_train_sched_metric, pxsom_batch_train.hip) and the pipeline's one-pass
// labelling.
//
// The search is pxsom_assign_metric's (pxsom_metric_bmu.h: prepared codebook, one lane per row, every pair in binary64), so the
// labels are its labels bit for bit.  It costs about 2 k c binary64 VALU operations per row; the statistics cost c + 1 adds per
// row, so they ride along: a labelled row's lane adds its row (rounded to the run's quantum: qround) and a 1 to a
// workgroup table [k*c sums | k counts] in LDS with binary64 LDS adds.  The grid is sized to the CUs, not to the rows, and
// loops over them; at the end every workgroup adds the non-zero entries of its table to the caller's statistics with global
// binary64 adds (contiguous entries on consecutive lanes).  A table that does not fit the LDS beside the staging slices is not
// built: the lanes add to the caller's statistics directly (what pxsom_cluster_sums does for such tables) -- same results.
// Rows taking part: a window of the row dealing of pxsom_batch_train_sched (row i iff e0 <= i % phases < e1), addressed with
// the rule of pxsom::RowView (window row t -> (t / wd) * phases + e0 + t % wd, wd = e1 - e0).
#include <map>
#include <mutex>

#include "pxsom_assign.h"
#include "pxsom_metric_bmu.h"
#include "pxsom_sums.h"

namespace {

using namespace pxsom_metric;
using pxsom_bmu::qround;

constexpr size_t kLdsMax = 160 * 1024;   // LDS of a gfx950 CU, what one workgroup may take
constexpr int kStageChSmall = 8;         // staged rows beside a table that leaves no room for kStageCh channels per chunk
constexpr int kMaxWgPerCu = 8;             // (K7m's grid: 8 workgroups per CU where registers and LDS allow)

// CX / SCH: bmu_search's (SCH == kStageChSmall sits beside a table that leaves room for one workgroup per CU: no occupancy to
// compile for, and the smaller register budget measured 1.9 x slower there).  nwin rows take part; window row t is row e0 + view.offset(t, rstride) of x.
// table != 0: dynamic LDS = [staging slices (CX == 0)] [k*(c+1) doubles]; table == 0: the staging slices only.
template <int M, typename T, int CX, int SCH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CX == 0 && SCH == kStageCh ? kStagedWavesPerSimd : 1)))
void assign_sums_metric_kernel(const T *__restrict__ x, int64_t nwin, int c, int64_t ldx,
                                                                 pxsom::RowView view, int64_t rstride, int e0,
                                                                 const double *__restrict__ wt, const double *__restrict__ wn,
                                                                 int k, int kp, int32_t *__restrict__ labels,
                                                                 double *__restrict__ stats, double qmagic, int table)
{
    extern __shared__ double step_smem[];
    const int lane = threadIdx.x & 63;
    double *xs = step_smem + (threadIdx.x >> 6) * (SCH * kStageLd);   // this wave's staging slice (CX == 0)
    double *tab = step_smem + (CX > 0 ? 0 : 4 * SCH * kStageLd);     // [k*c sums | k counts] of this workgroup
    const int nstats = k * (c + 1), nw = k * c;
    if (table) {
        for (int e = threadIdx.x; e < nstats; e += 256) tab[e] = 0.0;
        __syncthreads();
    }
    const int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63);
    // wave-uniform loop: the last wave's idle lanes work on the last window row and store nothing
    for (int64_t base = wave0; base < nwin; base += (int64_t)gridDim.x * 256) {
        auto row_of = [&](int r) { return (int64_t)e0 + view.offset(base + r < nwin ? base + r : nwin - 1, rstride); };
        double xr[CX > 0 ? CX : 1], best;
        const int bk = bmu_search<M, T, CX, SCH>(x, ldx, c, row_of, lane, xs, wt, wn, k, kp, xr, &best);
        if (base + lane < nwin) {
            const int64_t row = row_of(lane);
            if (labels) labels[row] = bk + 1;
            if (bk >= 0) {   // (a non-finite value of a labelled row joins the sums like any other)
                if (table) {
                    if constexpr (CX > 0) {
#pragma unroll
                        for (int j = 0; j < CX; j++)
                            if (j < c) atomicAdd(&tab[bk * c + j], qround(xr[j], qmagic));
                    } else {
                        const T *xp = x + row * ldx;
                        for (int j = 0; j < c; j++) atomicAdd(&tab[bk * c + j], qround((double)xp[j], qmagic));
                    }
                    atomicAdd(&tab[nw + bk], 1.0);
                } else {
                    if constexpr (CX > 0) {
#pragma unroll
                        for (int j = 0; j < CX; j++)
                            if (j < c) atomicAdd(&stats[(size_t)bk * c + j], qround(xr[j], qmagic));
                    } else {
                        const T *xp = x + row * ldx;
                        for (int j = 0; j < c; j++) atomicAdd(&stats[(size_t)bk * c + j], qround((double)xp[j], qmagic));
                    }
                    atomicAdd(&stats[nw + bk], 1.0);
                }
            }
        }
    }
    if (table) {
        __syncthreads();
        for (int e = threadIdx.x; e < nstats; e += 256) {
            const double v = tab[e];
            if (v != 0.0) atomicAdd(&stats[e], v);   // (NaN != 0: a non-finite sum is delivered too)
        }
    }
}

struct StepPlan {
    int sch;        // channels per staged chunk (rows wider than kRegChannels)
    int table;      // the workgroup table fits the LDS
    size_t lds;
};

inline StepPlan step_plan(int c, int k)
{
    StepPlan p;
    const bool reg = c <= kRegChannels;
    const size_t tbytes = (size_t)k * (c + 1) * sizeof(double);
    p.sch = kStageCh;
    p.table = 1;
    if (!reg && stage_bytes(kStageCh) + tbytes > kLdsMax) p.sch = kStageChSmall;
    size_t stage = reg ? 0 : stage_bytes(p.sch);
    if (stage + tbytes > kLdsMax) {
        p.table = 0;
        p.sch = kStageCh;
        stage = reg ? 0 : stage_bytes(p.sch);
    }
    p.lds = stage + (p.table ? tbytes : 0);
    return p;
}

// Raises the kernel's dynamic LDS limit where needed and returns in *wg_per_cu how many of its workgroups a CU holds at once (by
// registers and LDS; at most kMaxWgPerCu): the grid is exactly what is resident, so no workgroup waits for a slot while the
// others loop.  Cached per device and LDS size, under the cache's lock.
struct KernelFit {
    std::mutex lock;
    size_t raised = 0;
    std::map<size_t, int> wg_per_cu;
};

template <typename Kernel>
int fit_kernel(Kernel kern, size_t lds, KernelFit *have, int *wg_per_cu)
{
    const std::lock_guard<std::mutex> guard(have->lock);
    if (lds > 48 * 1024 && have->raised < lds) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return pxsom::fail(PXSOM_ERR_HIP, "pxsom_assign_sums_metric: cannot raise the LDS limit to %zu bytes: %s", lds, hipGetErrorString(e));
        have->raised = lds;
    }
    auto it = have->wg_per_cu.find(lds);
    if (it == have->wg_per_cu.end()) {
        int nbk = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbk, kern, 256, lds) != hipSuccess || nbk < 1) nbk = 1;
        it = have->wg_per_cu.emplace(lds, std::min(nbk, kMaxWgPerCu)).first;
    }
    *wg_per_cu = it->second;
    return PXSOM_OK;
}

template <int M, typename T>
int assign_sums_typed(const T *x, int64_t n, int c, int64_t ldx, const double *w, int k, int phases, int e0, int e1,
                      int32_t *labels, int32_t *scratch, double *stats, double qmagic, char *ws, hipStream_t st)
{
    if (sizeof(T) != 8) qmagic = 0.0;
    int wd = e1 - e0;
    if (wd == phases) phases = 1, e0 = 0, wd = 1;   // every row
    const int64_t full = n / phases, rem = n % phases;
    const int64_t nwin = full * wd + std::min<int64_t>(std::max<int64_t>(rem - e0, 0), wd);
    if (nwin == 0) return PXSOM_OK;
    const StepPlan pl = step_plan(c, k);
    // Two launches -- pxsom_assign_metric, then the sums kernels with qmagic -- where one pass measured slower than that pair
    // (DESIGN.md "K6m": cosine on staged rows; every metric when the table does not fit the LDS) and the pair can run: the
    // window is a strided matrix (every row, or one phase) and there is a vector for its labels (the caller's for a window of
    // every row, else `scratch`; a caller that wants the labels of ONE phase at their rows' own indices gets one pass).
    int32_t *lab2 = phases == 1 ? (labels ? labels : scratch) : (labels ? nullptr : scratch);
    if (((M == PXSOM_METRIC_COSINE && c > kRegChannels) || !pl.table) && wd == 1 && lab2) {
        const T *xv = x + (size_t)e0 * ldx;
        const int64_t ldv = ldx * phases;
        const int dt = sizeof(T) == 8 ? PXSOM_F64 : (sizeof(T) == 4 ? PXSOM_F32 : PXSOM_F16);
        int rc2 = pxsom_assign_metric(xv, nwin, c, ldv, dt, w, k, lab2, nullptr, ws, metric_workspace_bytes(c, k), M, st);
        if (rc2) return rc2;
        return pxsom::cluster_sums_typed<T, true>(xv, nwin, c, ldv, lab2, k, stats, reinterpret_cast<int64_t *>(stats + (size_t)k * c), st,
                                                  qmagic);
    }
    Prepared p;
    int rc = launch_metric_prep(w, k, c, M, ws, (unsigned)nwin, st, &p);
    if (rc) return rc;
    // the window as a row view in units of rows: wd consecutive rows out of every `phases` (wd == 1: every phases-th row)
    const pxsom::RowView view = wd > 1 ? pxsom::make_row_view(wd, phases) : pxsom::RowView{};
    const int64_t rstride = wd > 1 ? 1 : phases;
    const bool reg = c <= kRegChannels;
    static pxsom::PerDevice<KernelFit> fits[3];   // (per instantiation of this function: the kernels of one M, T)
    const dim3 block(256);
    const int cus = pxsom::device_cu_count();
    int per_cu = 1;
    auto grid_of = [&]() { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((nwin + 255) / 256, (int64_t)cus * per_cu))); };
    pxsom::Prof *prof = pxsom::current_prof();
    if (reg) {
        auto kern = assign_sums_metric_kernel<M, T, kRegChannels, kStageCh>;
        if ((rc = fit_kernel(kern, pl.lds, &fits[0].here(), &per_cu))) return rc;
        pxsom::prof_mark(prof, st, true, nwin);
        PXSOM_TIMED_LAUNCH(kern, grid_of(), block, pl.lds, st, x, nwin, c, ldx, view, rstride, e0, p.wt, p.wn, k, p.kp, labels, stats, qmagic,
                           pl.table);
    } else if (pl.sch == kStageCh) {
        auto kern = assign_sums_metric_kernel<M, T, 0, kStageCh>;
        if ((rc = fit_kernel(kern, pl.lds, &fits[1].here(), &per_cu))) return rc;
        pxsom::prof_mark(prof, st, true, nwin);
        PXSOM_TIMED_LAUNCH(kern, grid_of(), block, pl.lds, st, x, nwin, c, ldx, view, rstride, e0, p.wt, p.wn, k, p.kp, labels, stats, qmagic,
                           pl.table);
    } else {
        auto kern = assign_sums_metric_kernel<M, T, 0, kStageChSmall>;
        if ((rc = fit_kernel(kern, pl.lds, &fits[2].here(), &per_cu))) return rc;
        pxsom::prof_mark(prof, st, true, nwin);
        PXSOM_TIMED_LAUNCH(kern, grid_of(), block, pl.lds, st, x, nwin, c, ldx, view, rstride, e0, p.wt, p.wn, k, p.kp, labels, stats, qmagic,
                           pl.table);
    }
    pxsom::prof_mark(prof, st, false, nwin);
    PXSOM_LAUNCH_CHECK("assign_sums_metric_kernel");
    return PXSOM_OK;
}

template <int M>
int assign_sums_m(const void *x, int64_t n, int c, int64_t ldx, int dtype, const double *w, int k, int phases, int e0, int e1,
                  int32_t *labels, int32_t *scratch, double *stats, double qmagic, char *ws, hipStream_t st)
{
    PXSOM_DISPATCH_DTYPE(dtype, x, xp, (assign_sums_typed<M, T>(xp, n, c, ldx, w, k, phases, e0, e1, labels, scratch, stats, qmagic, ws, st)));
}

}  // namespace

int pxsom_metric::assign_sums_step(const void *x, int64_t n, int c, int64_t ldx, int dtype, const double *w, int k, int phases,
                                   int e0, int e1, int32_t *labels, int32_t *scratch, double *stats, double qmagic, char *ws,
                                   int metric, hipStream_t st)
{
    switch (metric) {
    case PXSOM_METRIC_MANHATTAN: return assign_sums_m<PXSOM_METRIC_MANHATTAN>(x, n, c, ldx, dtype, w, k, phases, e0, e1, labels, scratch, stats, qmagic, ws, st);
    case PXSOM_METRIC_CHEBYSHEV: return assign_sums_m<PXSOM_METRIC_CHEBYSHEV>(x, n, c, ldx, dtype, w, k, phases, e0, e1, labels, scratch, stats, qmagic, ws, st);
    default: return assign_sums_m<PXSOM_METRIC_COSINE>(x, n, c, ldx, dtype, w, k, phases, e0, e1, labels, scratch, stats, qmagic, ws, st);
    }
}

PXSOM_EXPORT size_t pxsom_metric_step_workspace_bytes(int c, int k, int metric)
{
    if (!metric_known(metric) || metric == PXSOM_METRIC_EUCLIDEAN || c < 1 || c > PXSOM_MAX_CHANNELS || k < 1 || k > PXSOM_MAX_NODES)
        return 0;
    return metric_workspace_bytes(c, k);
}

PXSOM_EXPORT int pxsom_assign_sums_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                                          int phases, int e0, int e1, int32_t *labels_dev, double *stats_dev, double sum_quantum,
                                          void *workspace_dev, size_t workspace_bytes, int metric, void *stream)
{
    if (!metric_known(metric))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG,
                           "pxsom_assign_sums_metric: unknown metric %d (FlowSOM distf: 1 Manhattan, 2 Euclidean, 3 Chebyshev, "
                           "4 cosine)", metric);
    if (metric == PXSOM_METRIC_EUCLIDEAN)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED,
                           "pxsom_assign_sums_metric: metric 2 (Euclidean) has its own entries: pxsom_assign_sums / "
                           "pxsom_batch_accumulate");
    if (n < 0 || n > 0x7fffffffLL)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_sums_metric: n=%lld outside [0, 2^31)", (long long)n);
    if (c < 1 || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_sums_metric: c=%d outside [1, %d]", c, PXSOM_MAX_CHANNELS);
    if (k < 1 || k > PXSOM_MAX_NODES)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_sums_metric: k=%d outside [1, %d]", k, PXSOM_MAX_NODES);
    if (ldx < c) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_sums_metric: ldx=%lld < c=%d", (long long)ldx, c);
    if (!pxsom::dtype_ok(dtype)) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_sums_metric: dtype %d", dtype);
    if (!w_dev || !stats_dev || (n > 0 && !x_dev))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_sums_metric: null pointer");
    if (phases < 1 || e0 < 0 || e1 <= e0 || e1 > phases)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_sums_metric: window needs 0 <= e0 < e1 <= phases, got [%d, %d) of %d",
                           e0, e1, phases);
    int qe = 0;
    if (!(sum_quantum >= 0.0) || (sum_quantum > 0.0 && frexp(sum_quantum, &qe) != 0.5))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_sums_metric: sum_quantum must be 0 or a power of two");
    const size_t need = metric_workspace_bytes(c, k);
    if (!workspace_dev || workspace_bytes < need)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "pxsom_assign_sums_metric: workspace %zu < %zu bytes", workspace_bytes, need);
    if (pxsom::row_view_active())
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_sums_metric: the metric kernels do not take row views");
    if (n == 0) return PXSOM_OK;
    const double qmagic = (dtype == PXSOM_F64 && sum_quantum > 0.0) ? 6755399441055744.0 /* 1.5 * 2^52 */ * sum_quantum : 0.0;
    return pxsom_metric::assign_sums_step(x_dev, n, c, ldx, dtype, w_dev, k, phases, e0, e1, labels_dev, nullptr, stats_dev, qmagic,
                                          reinterpret_cast<char *>(workspace_dev), metric, reinterpret_cast<hipStream_t>(stream));
}
