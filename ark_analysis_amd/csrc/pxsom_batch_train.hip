// pxsom_batch_train.hip -- the batch rule on gfx950: codebook update, accumulation, and the training pass driven from one call.
//
//   pxsom_batch_update       the batch rule's codebook update (oracle of record: orc_batch_update)
//   pxsom_batch_accumulate   a mini-batch step's accumulation half (BMU of every row, per-BMU sums)
//   pxsom_batch_train_*      the host loop over the mini-batch steps of a pass
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "pxsom_assign.h"
#include "pxsom_codebook_rules.h"
#include "pxsom_common.h"
#include "pxsom_metric_step.h"
#include "pxsom_sums.h"
#include "pxsom_wave.h"
#include "pxsom_xch.h"

namespace {

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// batch update: one workgroup per node k, thread <-> channel.  Only the Chebyshev window of k is
// visited, in the oracle's separable summation order (orc_batch_update: per grid row, then over the rows).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void batch_update_kernel(double *w, int xdim, int ydim, int c,
                                                           const double *__restrict__ sums,
                                                           const double *__restrict__ counts,
                                                           double thr, double q, double sat, int stage,
                                                           double *__restrict__ zero_out, int zero_count,
                                                           const double *w_src = nullptr)
{
    if (!w_src) w_src = w;   // (w_src != w: the updated codebook goes to w, the source stays as it is -- no copy launch)
    extern __shared__ __attribute__((aligned(16))) char upd_smem[];
    const int k = blockIdx.x, tid = threadIdx.x;
    // the OTHER statistics buffer (the next accumulate's target) is cleared here, a slice per workgroup
    // (R10 clear_stats_slice in unsigned arithmetic, written out: through the rule this kernel comes out with other instructions)
    if (zero_count > 0) {
        const int per = (zero_count + gridDim.x - 1) / gridDim.x;
        for (int e = k * per + tid; e < min((k + 1) * per, zero_count); e += 256) zero_out[e] = 0.0;
    }
    const int kx = k / ydim, ky = k % ydim;
    const int r = pxsom_bmu::window_radius(thr);
    const int x0 = kx - r < 0 ? 0 : kx - r, x1 = kx + r > xdim - 1 ? xdim - 1 : kx + r;
    const int y0 = ky - r < 0 ? 0 : ky - r, y1 = ky + r > ydim - 1 ? ydim - 1 : ky + r;
    // The window rows x0..x1 are contiguous in node order: stage their statistics in LDS with every
    // thread of the workgroup loading (8 in flight each) -- a loop of dependent L2 round trips per window
    // node costs 5-10 us at radius 6 -- then sum from LDS in the oracle's order.
    const int b_lo = x0 * ydim, b_hi = (x1 + 1) * ydim;  // node range [b_lo, b_hi)
    const double *ls = sums, *lc = counts;
    int boff = 0;
    if (stage) {
        double *ss = reinterpret_cast<double *>(upd_smem);  // [(b_hi - b_lo) * c] sums, then counts
        const int ne = (b_hi - b_lo) * c, nc = b_hi - b_lo;
        const double *gs = sums + (size_t)b_lo * c, *gc = counts + b_lo;
        for (int e0 = tid; e0 < ne + nc; e0 += 8 * 256) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int e = e0 + u * 256;
                v[u] = e < ne ? gs[e] : (e < ne + nc ? gc[e - ne] : 0.0);
            }
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (e0 + u * 256 < ne + nc) ss[e0 + u * 256] = v[u];
        }
        __syncthreads();
        ls = ss;
        lc = ss + ne;
        boff = b_lo;
    }
    for (int j = tid; j < c; j += 256) {   // (wide rows: more channels than threads)
        const double wv = w_src[(size_t)k * c + j];
        // separable order of orc_batch_update: T[bx] = sum over the window's by (ascending), num = sum of T[bx]
        double num = 0.0, den = 0.0;
        for (int bx = x0; bx <= x1; bx++) {
            double tn = 0.0, td = 0.0;
#pragma unroll 4
            for (int by = y0; by <= y1; by++) {
                const int b = bx * ydim + by - boff;
                td += lc[b];
                tn += ls[(size_t)b * c + j];
            }
            den += td;
            num += tn;
        }
        if (den > 0.0) {
            // 1 - (1-alpha)^den by binary exponentiation, 1 - alpha formed on the host (batch_gain; orc_batch_update)
            const double gain = pxsom_bmu::batch_gain(den, q, sat), inv = 1.0 / den;
            w[(size_t)k * c + j] = pxsom_bmu::node_update(wv, gain, num * inv);
        } else if (w_src != w) {
            w[(size_t)k * c + j] = wv;
        }
    }
}

#pragma clang fp contract(fast)

// w = update of w_src (NULL: of w itself, in place) from [sums | counts]; zero_count > 0: zero_out cleared by the same launch
int launch_batch_update(double *w, const double *w_src, int xdim, int ydim, int c, const double *sums, const double *counts,
                        double thr, double alpha, double *zero_out, int zero_count, hipStream_t st)
{
    const int k = xdim * ydim;
    // statistics of the widest window (the whole grid) staged in LDS when they fit
    const size_t stage_bytes = (size_t)k * (c + 1) * sizeof(double);
    const int stage = stage_bytes <= 60 * 1024;
    hipLaunchKernelGGL(batch_update_kernel, dim3(k), dim3(256), stage ? stage_bytes : 0, st, w, xdim, ydim, c, sums, counts, thr,
                       1.0 - alpha, pxsom_bmu::batch_gain_saturation(1.0 - alpha), stage, zero_out, zero_count, w_src);
    PXSOM_LAUNCH_CHECK("batch_update_kernel");
    return PXSOM_OK;
}

}  // namespace

PXSOM_EXPORT int pxsom_batch_update(double *w_dev, int xdim, int ydim, int c, const double *sums_dev,
                                    const double *counts_dev, double thr, double alpha, void *stream)
{
    if (xdim < 1 || ydim < 1 || (int64_t)xdim * ydim > PXSOM_MAX_NODES || c < 1 || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_batch_update: shape %dx%d x %d", xdim, ydim, c);
    if (!w_dev || !sums_dev || !counts_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_update: null pointer");
    return launch_batch_update(w_dev, nullptr, xdim, ydim, c, sums_dev, counts_dev, thr, alpha, nullptr, 0,
                               reinterpret_cast<hipStream_t>(stream));
}

// codebooks the accumulating filter prepares for itself inside its own launch (register-resident shapes)
static bool self_preparing_shape(int c, int k)
{
    const pxsom_bmu::Layout L = pxsom_bmu::make_layout(0, c, k);
    return c % 2 == 0 && L.nch == 1 && L.nb == 7 && (k - 16 * (L.nb - 1) + 3) / 4 == 1;
}

// One mini-batch step's accumulation half: zero the statistics, BMU of every row, per-BMU sums.
// stats_dev = [k*c sums | k counts], all binary64 (counts are exact integers below 2^53), so the
// multi-GPU all-reduce is a single sum over one buffer.
// flags & PXSOM_ACC_PREPARED: pxsom_batch_update_prepare already cleared stats_dev (and prepared the workspace
// for w_dev where the shape needs one).
static int batch_accumulate_impl(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                                 int32_t *labels_dev, double *stats_dev, void *workspace_dev, size_t workspace_bytes, int flags,
                                 void *stream, double qmagic);

PXSOM_EXPORT int pxsom_batch_accumulate(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype,
                                        const double *w_dev, int k, int32_t *labels_dev, double *stats_dev,
                                        void *workspace_dev, size_t workspace_bytes, int flags, void *stream)
{
    return batch_accumulate_impl(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, stats_dev, workspace_dev, workspace_bytes, flags,
                                 stream, 0.0);
}

// qmagic != 0: binary64 rows rounded to the run's quantum as they join the statistics (the one-launch accumulating filter
// does not know the rounding: search and sums run as two kernels then)
static int batch_accumulate_impl(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                                 int32_t *labels_dev, double *stats_dev, void *workspace_dev, size_t workspace_bytes, int flags,
                                 void *stream, double qmagic)
{
    if (dtype != PXSOM_F64) qmagic = 0.0;
    if (!stats_dev || k < 1 || k > PXSOM_MAX_NODES || c < 1 || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_accumulate: bad statistics buffer / shape");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool cleared = (flags & PXSOM_ACC_PREPARED) != 0;
    if (!cleared) PXSOM_HIP_TRY(hipMemsetAsync(stats_dev, 0, (size_t)k * (c + 1) * sizeof(double), st));
    // fused route (register-resident filter shapes): ONE launch prepares the codebook, labels every row,
    // settles the listed rows and accumulates -- one pass over x
    bool fused = false;
    int rc = PXSOM_OK;
    if (qmagic == 0.0)
        rc = pxsom_bmu::assign_accumulate(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, stats_dev, workspace_dev,
                                          workspace_bytes, st, &fused);
    if (fused) return rc;
    if (n == 0) return PXSOM_OK;
    rc = pxsom::check_matrix("pxsom_batch_accumulate", x_dev, n, c, ldx, dtype);
    if (rc) return rc;
    // a workspace prepared by update_prepare exists only for shapes that are not self-preparing
    if (cleared && !self_preparing_shape(c, k)) {
        if (!w_dev || !labels_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_accumulate: null pointer");
        rc = pxsom_bmu::assign_prepared(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, workspace_dev, workspace_bytes, st);
    } else {
        rc = pxsom_assign(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, nullptr, workspace_dev, workspace_bytes, stream);
    }
    if (rc) return rc;
    double *sums = stats_dev;
    int64_t *counts = reinterpret_cast<int64_t *>(stats_dev + (size_t)k * c);
    PXSOM_DISPATCH_DTYPE(dtype, x_dev, xp, (pxsom::cluster_sums_typed<T, true>(xp, n, c, ldx, labels_dev, k, sums, counts, st, qmagic)));
}

// The update half of a mini-batch step plus what the NEXT pxsom_batch_accumulate(PXSOM_ACC_PREPARED) relies on:
// codebook update from the (all-reduced) statistics in stats_dev; stats_next_dev -- the buffer the next
// accumulate will fill -- cleared by the same launch (pass the other one of two alternating buffers; with
// stats_next_dev == stats_dev or NULL the buffer is cleared by a separate fill); and, for codebook shapes the
// accumulating filter does not prepare itself, the workspace prepared for the new codebook.
// (A single-workgroup fusion of update and prep was measured slower: its window sums are LDS-bandwidth bound
// on one CU, 9-14 us at radius 6; so was a last-workgroup-runs-prep variant.)
PXSOM_EXPORT int pxsom_batch_update_prepare(double *w_dev, int xdim, int ydim, int c, double *stats_dev,
                                            double *stats_next_dev, double thr, double alpha,
                                            void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (xdim < 1 || ydim < 1 || (int64_t)xdim * ydim > PXSOM_MAX_NODES || c < 1 || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_batch_update_prepare: shape %dx%d x %d", xdim, ydim, c);
    if (!w_dev || !stats_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_update_prepare: null pointer");
    const int k = xdim * ydim;
    const bool needs_ws = !self_preparing_shape(c, k);
    if (needs_ws && (!workspace_dev || workspace_bytes < pxsom_assign_workspace_bytes(0, c, k)))
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "pxsom_batch_update_prepare: workspace %zu bytes too small",
                           workspace_bytes);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nstats = k * (c + 1);
    const bool other = stats_next_dev && stats_next_dev != stats_dev;
    int rc = launch_batch_update(w_dev, nullptr, xdim, ydim, c, stats_dev, stats_dev + (size_t)k * c, thr, alpha,
                                 other ? stats_next_dev : nullptr, other ? nstats : 0, st);
    if (rc) return rc;
    if (!other) PXSOM_HIP_TRY(hipMemsetAsync(stats_dev, 0, (size_t)nstats * sizeof(double), st));
    if (!needs_ws) return PXSOM_OK;
    return pxsom_bmu::prepare_only(w_dev, c, k, workspace_dev, workspace_bytes, nullptr, st);
}

// ------------------------------------------------------------------------------------------------
// Batch training pass driven from ONE call (pxsom_batch_train_steps): the host loop over the mini-batch steps
// lives here, not in Python.  Register-resident shapes on a 10 x 10 grid take one launch per step (batch_step_kernel,
// pxsom_batch_step.hip: pending update + prep + filter + table + flush); other shapes run update-and-prepare /
// filter / exact / cluster sums per step.  Both keep the same state:
//   wbuf[g % 2]        W_g, the codebook step g searches with          (two buffers alternate)
//   ring[g % 3]        statistics of step g; ring[(g+1) % 3] is cleared by step g
// so a multi-rank run all-reduces ring[g % 3] right behind step g (comm != NULL: enqueued here, pxsom_comm.hip; or the
// caller runs one step per call and all-reduces in between).
// ------------------------------------------------------------------------------------------------
namespace {

// (thr, alpha) of the online schedule at position pos / span of the run (pos = rows presented before the step, in
// phases: orc_som_batch_sched)
inline void batch_schedule(int64_t pos, int64_t span, double a0, double a1, double r0, double r1, double *thr, double *alpha)
{
    double t = r0 - (r0 - r1) * (double)pos / (double)span;
    if (t < 1.0) t = 0.5;
    *thr = t;
    *alpha = a0 - (a0 - a1) * (double)pos / (double)span;
}

// A pass's schedule: row i belongs to phase i % phases, step g takes the phases [edges[g], edges[g+1]).
struct Sched {
    int phases, steps;
    const int32_t *edges;   // host, [steps + 1]
    int e0(int g) const { return edges[g]; }
    int width(int g) const { return edges[g + 1] - edges[g]; }
    int64_t rows(int64_t n, int g) const
    {
        const int64_t full = n / phases, rem = n % phases;
        const int64_t part = std::min<int64_t>(std::max<int64_t>(rem - e0(g), 0), width(g));
        return full * width(g) + part;
    }
    int64_t offset(int64_t n, int g) const   // rows of the steps before g
    {
        const int64_t full = n / phases, rem = n % phases;
        return full * e0(g) + std::min<int64_t>(e0(g), rem);
    }
    int64_t rows_max(int64_t n) const
    {
        int64_t m = 0;
        for (int g = 0; g < steps; g++) m = std::max(m, rows(n, g));
        return m;
    }
    bool any_wide() const
    {
        for (int g = 0; g < steps; g++)
            if (width(g) > 1) return true;
        return false;
    }
    int64_t pos(int gg) const { return (int64_t)(gg / steps) * phases + e0(gg % steps); }   // of global step gg
};

int check_sched(const char *fn, int phases, const int32_t *edges, int steps)
{
    if (phases < 1 || steps < 1 || steps > PXSOM_MAX_SCHED_STEPS || !edges || edges[0] != 0 || edges[steps] != phases)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: schedule needs 1 <= steps <= %d, edges[0] == 0, edges[steps] == phases", fn,
                           PXSOM_MAX_SCHED_STEPS);
    for (int g = 0; g < steps; g++)
        if (edges[g + 1] < edges[g]) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: schedule edges must not decrease", fn);
    return PXSOM_OK;
}

// Steps that take several phases (width > 1) on shapes outside the fused kernel: their rows are gathered ONCE per run
// into step-contiguous order (the generic search / exact / sums kernels take plain strided matrices).  One work item
// per (destination row, 16 / 8 / 4 / 2-byte chunk); the step of a destination row by binary search over the
// closed-form offsets.
struct SchedArg {
    int phases, steps;
    int edges[PXSOM_MAX_SCHED_STEPS + 1];
};

template <typename V>
__global__ __launch_bounds__(256) void gather_steps_kernel(const V *__restrict__ x, int64_t n, int cpr, int64_t ldx_v,
                                                           V *__restrict__ out, SchedArg s)
{
    const int64_t full = n / s.phases, rem = n % s.phases;
    auto off = [&](int g) { return full * s.edges[g] + min((int64_t)s.edges[g], rem); };
    const int64_t items = n * cpr;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
        const int64_t d = it / cpr;
        const int ch = (int)(it - d * cpr);
        int lo = 0, hi = s.steps;   // the step with off(lo) <= d < off(lo + 1)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off(mid) <= d) lo = mid;
            else hi = mid;
        }
        const int64_t r = d - off(lo);
        const int w = s.edges[lo + 1] - s.edges[lo];
        const int64_t src = (r / w) * s.phases + s.edges[lo] + (r % w);
        out[d * cpr + ch] = x[src * ldx_v + ch];
    }
}

template <typename T>
int launch_gather(const T *x, int64_t n, int c, int64_t ldx, T *out, const Sched &sc, hipStream_t st)
{
    SchedArg a;
    a.phases = sc.phases;
    a.steps = sc.steps;
    for (int g = 0; g <= sc.steps; g++) a.edges[g] = sc.edges[g];
    const size_t rb = (size_t)c * sizeof(T), lb = (size_t)ldx * sizeof(T);
    const uintptr_t ax = reinterpret_cast<uintptr_t>(x), ao = reinterpret_cast<uintptr_t>(out);
    const int64_t grid_max = (int64_t)pxsom::device_cu_count() * 16;
    auto go = [&](auto tag) {
        typedef decltype(tag) V;
        const int cpr = (int)(rb / sizeof(V));
        const int64_t grid = std::min<int64_t>((n * cpr + 255) / 256, grid_max);
        hipLaunchKernelGGL(gather_steps_kernel<V>, dim3((unsigned)std::max<int64_t>(grid, 1)), dim3(256), 0, st,
                           reinterpret_cast<const V *>(x), n, cpr, (int64_t)(lb / sizeof(V)), reinterpret_cast<V *>(out), a);
    };
    if (rb % 16 == 0 && lb % 16 == 0 && ax % 16 == 0 && ao % 16 == 0) go(uint4{});
    else if (rb % 8 == 0 && lb % 8 == 0 && ax % 8 == 0 && ao % 8 == 0) go(uint2{});
    else if (rb % 4 == 0 && lb % 4 == 0 && ax % 4 == 0 && ao % 4 == 0) go((unsigned)0);
    else go((unsigned short)0);
    PXSOM_LAUNCH_CHECK("gather_steps_kernel");
    return PXSOM_OK;
}

// The run's centring vector for the one-launch step's filter (AssignHdr::mu_s, DESIGN.md "K7 centring"): the mean of the
// codebook the run starts from, per channel, in binary32.  Any vector keeps the search exact; this one stays close to the
// nodes' mean for the whole run (they follow the data), so the steps need no reduction of their own for it.
__global__ __launch_bounds__(1024) void centring_vector_kernel(const double *__restrict__ w, int k, int c, float *__restrict__ mu32,
                                                               double *__restrict__ zero_out, int zero_count, double *__restrict__ copy_out)
{
    // 1024 threads clear and copy (a 100 x 100 codebook on 256 threads was 40 dependent load -> store trips: 22 us of config 4's
    // pass), the first 256 form the means
    for (int e = threadIdx.x; e < zero_count; e += 1024) zero_out[e] = 0.0;   // the first step's statistics buffer (no memset launch)
    if (copy_out) {   // W_0 handed over by the caller: into the run's codebook buffer (no copy launch in front of the pass)
        for (int e0 = threadIdx.x; e0 < k * c; e0 += 4 * 1024) {
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = w[e0 + u * 1024 < k * c ? e0 + u * 1024 : 0];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (e0 + u * 1024 < k * c) copy_out[e0 + u * 1024] = v[u];
        }
    }
    __shared__ float s_m[pxsom_bmu::kFilterMaxChannels];
    if (threadIdx.x < pxsom_bmu::kFilterMaxChannels) s_m[threadIdx.x] = 0.f;
    __syncthreads();
    // `parts` adjacent lanes share a channel (8 for c <= 32, 2 for c <= 128): each sums every parts-th node with its loads in
    // flight eight at a time -- a lane walking 50 nodes one L2 round trip after the other made this launch 16 us
    if (threadIdx.x < 256) {
        const int cp = c <= 32 ? 32 : (c <= 64 ? 64 : 128), parts = 256 / cp;
        const int j = threadIdx.x / parts, part = threadIdx.x % parts;
        double sum = 0.0;
        if (j < c) {
            for (int n0 = part; n0 < k; n0 += 8 * parts) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = n0 + u * parts < k ? w[(size_t)(n0 + u * parts) * c + j] : 0.0;
#pragma unroll
                for (int u = 0; u < 8; u++) sum += v[u];
            }
        }
        for (int d = 1; d < parts; d *= 2) sum += __shfl_xor(sum, d);
        float m = (float)(sum / (double)k);
        if (!(j < c && fabsf(m) <= 3.0e38f)) m = 0.f;   // a non-finite codebook: not centred (every row is listed anyway)
        if (part == 0 && j < pxsom_bmu::kFilterMaxChannels) {
            mu32[j] = m;
            s_m[j] = m;
        }
    }
    __syncthreads();
    // word 128: the vector's norm (the steps cap their power-of-two scale with it: pxsom_batch_step.hip)
    if (threadIdx.x < 64) {
        const double a = (double)s_m[threadIdx.x], b = (double)s_m[threadIdx.x + 64];
        double n2 = a * a + b * b;
        for (int d = 1; d < 64; d *= 2) n2 += __shfl_xor(n2, d);
        if (threadIdx.x == 0) mu32[pxsom_bmu::kFilterMaxChannels] = (float)sqrt(n2);
    }
}

struct TrainWs {
    size_t assign_ws, off_labels, off_mu, off_gather, total;
};
inline TrainWs train_ws(int64_t n, int c, int k, size_t esize, const Sched &sc)
{
    TrainWs w;
    const int64_t rmax = sc.rows_max(n);
    w.assign_ws = pxsom_assign_workspace_bytes(rmax, c, k);
    w.off_labels = pxsom::align_up(w.assign_ws, 256);
    w.off_mu = w.off_labels + pxsom::align_up((size_t)(rmax > 0 ? rmax : 1) * sizeof(int32_t), 256);
    w.off_gather = w.off_mu + 1024;   // 129 floats: the run's centring vector (c <= 128) and its norm
    w.total = w.off_gather + (sc.any_wide() ? pxsom::align_up((size_t)(n > 0 ? n : 1) * c * esize, 256) : 0);
    return w;
}
}  // namespace
namespace pxsom {
int comm_allreduce_sum_f64(pxsom_comm *c, double *buf, size_t count, hipStream_t st);   // pxsom_comm.hip
}
namespace {

constexpr int64_t kWideWindowedMaxRows = 4096;   // rows of a windowed step the wide one-launch kernel takes

template <typename T>
int train_steps_typed(const T *x, int64_t n, int c, int64_t ldx, int dtype, double *wbuf, double *ring, int xdim,
                      int ydim, const Sched &sc, int g_begin, int g_end, int num_passes, double a0, double a1, double r0,
                      double r1, double sum_quantum, char *ws, int flags, pxsom_comm *comm, hipStream_t st,
                      const double *w0 = nullptr)
{
    // binary64 rows of a reproducible run: (v + qmagic) - qmagic rounds v to a multiple of the quantum
    const double qmagic = (sizeof(T) == 8 && sum_quantum > 0.0) ? 6755399441055744.0 /* 1.5 * 2^52 */ * sum_quantum : 0.0;
    const int k = xdim * ydim;
    const size_t nstats = (size_t)k * (c + 1), nw = (size_t)k * c;
    const TrainWs tw = train_ws(n, c, k, sizeof(T), sc);
    const size_t assign_ws = tw.assign_ws;
    int32_t *labels = reinterpret_cast<int32_t *>(ws + tw.off_labels);
    T *xg = reinterpret_cast<T *>(ws + tw.off_gather);
    const int64_t span = (int64_t)num_passes * sc.phases;
    // which route a step takes (one decision per run: every step of a shape shares it, and so do all ranks -- the fused
    // kernel needs rows >= 1, which a rank with a short shard may not have, so empty steps are allowed there)
    const bool fused_shape = !(flags & PXSOM_TRAIN_UNFUSED) &&
                             pxsom_bmu::step_fused_shape<T>(x, 1, c, ldx, xdim, ydim, (int64_t)sc.phases * ldx);
    float *mu32 = reinterpret_cast<float *>(ws + tw.off_mu);
    // rows of 2-byte floats on the generic route keep the uncentred two-term split (pxsom_assign_filter.hip)
    const bool centred_run = fused_shape || (sizeof(T) != 2 && c <= pxsom_bmu::kFilterMaxChannels && !(flags & PXSOM_TRAIN_UNFUSED));
    if (g_begin == 0) {   // the first step's statistics buffer; every later one is cleared by the step before it
        // (w0: the codebook the run starts from, where the caller holds it -- copied into wbuf[0] by the launch that is there anyway)
        if (centred_run) {
            hipLaunchKernelGGL(centring_vector_kernel, dim3(1), dim3(1024), 0, st, w0 ? w0 : wbuf, k, c, mu32, ring, (int)nstats,
                               w0 ? wbuf : (double *)nullptr);
            PXSOM_LAUNCH_CHECK("centring_vector_kernel");
        } else {
            if (w0) PXSOM_HIP_TRY(hipMemcpyAsync(wbuf, w0, nw * sizeof(double), hipMemcpyDeviceToDevice, st));
            PXSOM_HIP_TRY(hipMemsetAsync(ring, 0, nstats * sizeof(double), st));
        }
    }
    // Round 6: where every kernel of the generic route takes row views (pxsom_common.h RowView: more than 64 channels of binary32 /
    // binary16 rows, contiguous in the caller's matrix) the steps read their rows where they lie -- no gathered copy of the matrix
    // at the head of every pass (config 4: 217 us of 2.0 ms, 800 MB of traffic)
    const bool viewed = !fused_shape && sc.any_wide() && c > 32 && c <= pxsom_bmu::kFilterMaxChannels && pxsom::sums_take_views<T>(x, c, ldx, k);
    const bool gathered = !fused_shape && sc.any_wide() && !viewed;
    if (gathered && g_begin == 0 && n > 0) {
        int rc = launch_gather<T>(x, n, c, ldx, xg, sc, st);
        if (rc) return rc;
    }
    // The exchange inside the step launches (round 5; a peer-to-peer communicator with pxsom_comm_p2p_set_fused, the fused 10 x 10 step):
    // step gg's last workgroup hands this rank's statistics to every rank, step gg + 1 adds the ranks' slots in rank order while
    // it applies the pending update -- no all-reduce launch between two steps.  The last step of the call keeps the separate
    // all-reduce: the next call (or the final update) reads the ring.  Every rank takes the same decision (same environment,
    // same communicator kind, agreed route).
    pxsom::FusedXch fxch;
    bool fused_xch = false;
    if (comm && fused_shape && g_end - g_begin >= 2)   // (false unless the communicator is peer-to-peer with its fused switch on)
        fused_xch = pxsom::comm_fused_begin(comm, g_end - g_begin - 1, nstats, &fxch);
    for (int gg = g_begin; gg < g_end; gg++) {
        const int g = gg % sc.steps;
        const int64_t rows = sc.rows(n, g);
        const int wd = sc.width(g);
        // the step's rows as a strided matrix: phase view (one phase), or its slice of the gathered copy
        const T *xv = gathered ? xg + (size_t)sc.offset(n, g) * c : x + (size_t)sc.e0(g) * ldx;
        const int64_t ldv = gathered ? c : ((viewed && wd > 1) ? ldx : ldx * sc.phases);
        const pxsom::RowViewScope view_scope((viewed && wd > 1) ? pxsom::make_row_view(wd, (int64_t)sc.phases * ldx) : pxsom::RowView{});
        if (rows >= (int64_t)1 << 31) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_batch_train: a step of %lld rows", (long long)rows);
        double *w_prev = wbuf + (size_t)((gg + 1) % 2) * nw, *w_cur = wbuf + (size_t)(gg % 2) * nw;
        double *s_prev = ring + (size_t)((gg + 2) % 3) * nstats, *s_cur = ring + (size_t)(gg % 3) * nstats,
               *s_next = ring + (size_t)((gg + 1) % 3) * nstats;
        double thr = 0.0, alpha = 0.0;
        if (gg > 0) batch_schedule(sc.pos(gg - 1), span, a0, a1, r0, r1, &thr, &alpha);
        // What the three one-launch routes below hand their kernels alike: the pending update of step gg - 1 and the step's
        // housekeeping.  Each route adds what is its own: where W_g goes, the centring vector, the relative tolerance of its
        // filter (filter_tol_rel, pxsom_assign.h: DESIGN.md "K7 error bound"), the quantum of a reproducible run, its row view.
        pxsom_bmu::StepArgs base{};
        base.w_in = gg > 0 ? w_prev : w_cur;
        base.stats_prev = s_prev;
        base.stats_zero = s_next;
        base.zero_count = (int)nstats;
        base.has_update = gg > 0 ? 1 : 0;
        base.thr = thr;
        base.q = 1.0 - alpha;
        base.sat = pxsom_bmu::batch_gain_saturation(base.q);
        base.tol_abs = (float)pxsom_bmu::filter_tol_abs(c);
        if (fused_shape) {
            pxsom_bmu::StepArgs sa = base;
            sa.w_out = w_cur;
            sa.mu32 = mu32;
            // (5 index bits in the scores: the lane group travels beside them; single accumulation chain, centred rows)
            sa.tol_rel = pxsom_bmu::filter_tol_rel(5, pxsom_bmu::filter_accum_units(c, 3), true);
            sa.qmagic = qmagic;
            sa.group_w = wd > 1 ? wd : 1;
            sa.group_stride = (int64_t)sc.phases * ldx;
            sa.dup_small = (flags & PXSOM_TRAIN_SMALL_DUP_TABLES) ? 1 : 0;
            if (fused_xch) {
                const int i = gg - g_begin;                       // the exchange behind step gg has epoch base + i + 1
                sa.xch_peers = fxch.peers;
                sa.xch_ticket = fxch.ticket;
                sa.xch_nranks = fxch.nranks;
                sa.xch_rank = fxch.rank;
                sa.xch_max_count = fxch.max_count;
                sa.xch_wait = i > 0 ? fxch.epoch_base + (unsigned long long)i : 0ull;
                sa.xch_signal = gg + 1 < g_end ? fxch.epoch_base + (unsigned long long)i + 1ull : 0ull;
            }
            // (an empty step -- a rank whose shard is shorter than the schedule -- still launches: the update, the
            // clearing of the next buffer and W_g are the kernel's, and every rank must take the same route)
            int rc = pxsom_bmu::launch_batch_step<T>(x + (size_t)sc.e0(g) * ldx, rows, c, wd > 1 ? ldx : ldx * sc.phases, s_cur, sa,
                                                     0 /* 16-row tiles per wave: by step size (launch_step) */, st);
            if (rc) return rc;
            if (comm && (!fused_xch || gg + 1 == g_end) && (rc = pxsom::comm_allreduce_sum_f64(comm, s_cur, nstats, st))) return rc;
            continue;
        }
        // small steps (<= 16 K rows) of codebooks up to 256 nodes x 128 channels: ONE launch (update, fragments, search, exact
        // settle, statistics: pxsom_batch_step_wide.hip) instead of the four or five below -- the BMU-only steps (threshold
        // pinned at 0.5) on any grid, the windowed ones on grids up to 16 x 16
        if constexpr (sizeof(T) >= 4) {
            const bool bmu_only = gg > 0 && thr == 0.5;
            if (!(flags & PXSOM_TRAIN_UNFUSED) && rows <= pxsom_bmu::step_wide_max_rows() && pxsom_bmu::step_wide_shape<T>(c, k) &&
                (bmu_only || (rows <= kWideWindowedMaxRows && pxsom_bmu::step_wide_windowed(xdim, ydim, c)))) {
                pxsom_bmu::StepArgs sa = base;
                sa.w_out = gg > 0 ? w_cur : nullptr;
                sa.mu32 = centred_run ? mu32 : nullptr;
                // (5 index bits in the scores -- 6 from 129 nodes on --, three-term split, centred rows)
                sa.tol_rel = pxsom_bmu::filter_tol_rel(k > 128 ? 6 : 5, pxsom_bmu::filter_accum_units_split(c, 3), true);
                sa.qmagic = qmagic;
                int rc = pxsom_bmu::launch_batch_step_wide<T>(xv, rows, c, ldv, xdim, ydim, s_cur, sa, st);
                if (rc) return rc;
                if (comm && (rc = pxsom::comm_allreduce_sum_f64(comm, s_cur, nstats, st))) return rc;
                continue;
            }
        }
        // codebooks the all-in-one kernel cannot hold (K = 400, or C > 32): ONE launch applies the pending update and
        // prepares the assign workspace for W_g (copy + update + clears + prep before), then search / exact / sums
        if (!(flags & PXSOM_TRAIN_UNFUSED)) {
            const int npk = pxsom_bmu::packed_rows_ok<T>(xv, ldv) ? pxsom_bmu::packed_k(c, k, sizeof(T) == 2) : 0;
            const pxsom_bmu::Layout L = pxsom_bmu::make_layout(rows, c, k, npk);
            pxsom_bmu::StepArgs sa = base;
            sa.w_out = gg > 0 ? w_cur : nullptr;
            // the generic filter is centred on the run's vector too (binary32 / binary64 rows)
            sa.mu32 = (centred_run && npk == 0) ? mu32 : nullptr;
            sa.tol_rel = pxsom_bmu::filter_tol_rel(L.idx_bits, pxsom_bmu::filter_accum_units_for(c, 3, npk), sa.mu32 != nullptr);
            // (no sa.qmagic here: this launch adds no rows; the quantum goes to the sums kernel below)
            int rc = PXSOM_OK;
            if (pxsom_bmu::launch_update_prepare(sa, xdim, ydim, c, ws, L, st, &rc)) {
                if (rc) return rc;
                if (rows > 0) {
                    rc = pxsom_bmu::assign_prepared(xv, rows, c, ldv, dtype, w_cur, k, labels, ws, assign_ws, st, npk);
                    if (rc) return rc;
                    rc = pxsom::cluster_sums_typed<T, true>(xv, rows, c, ldv, labels, k, s_cur, reinterpret_cast<int64_t *>(s_cur + nw), st, qmagic);
                    if (rc) return rc;
                }
                if (comm && (rc = pxsom::comm_allreduce_sum_f64(comm, s_cur, nstats, st))) return rc;
                continue;
            }
        }
        if (gg > 0) {
            PXSOM_HIP_TRY(hipMemcpyAsync(w_cur, w_prev, nw * sizeof(double), hipMemcpyDeviceToDevice, st));
            int rc = pxsom_batch_update(w_cur, xdim, ydim, c, s_prev, s_prev + nw, thr, alpha, st);
            if (rc) return rc;
        }
        PXSOM_HIP_TRY(hipMemsetAsync(s_next, 0, nstats * sizeof(double), st));
        int rc = batch_accumulate_impl(xv, rows, c, ldv, dtype, w_cur, k, labels, s_cur, ws, assign_ws, 0, st, qmagic);
        if (rc) return rc;
        if (comm && (rc = pxsom::comm_allreduce_sum_f64(comm, s_cur, nstats, st))) return rc;
    }
    return PXSOM_OK;
}

inline std::vector<int32_t> equal_edges(int m)
{
    std::vector<int32_t> e((size_t)m + 1);
    for (int t = 0; t <= m; t++) e[(size_t)t] = t;
    return e;
}

}  // namespace

PXSOM_EXPORT size_t pxsom_batch_train_sched_workspace_bytes(int64_t n, int c, int k, int dtype, int phases,
                                                            const int32_t *edges, int steps_per_pass)
{
    if (n < 0 || c < 1 || c > PXSOM_MAX_CHANNELS || k < 1 || k > PXSOM_MAX_NODES || !pxsom::dtype_ok(dtype)) return 0;
    if (check_sched("pxsom_batch_train_sched_workspace_bytes", phases, edges, steps_per_pass)) return 0;
    const Sched sc{phases, steps_per_pass, edges};
    return train_ws(n, c, k, dtype == PXSOM_F64 ? 8 : (dtype == PXSOM_F32 ? 4 : 2), sc).total;
}

PXSOM_EXPORT size_t pxsom_batch_train_workspace_bytes(int64_t n, int batch_steps, int c, int k)
{
    if (batch_steps < 1 || batch_steps > PXSOM_MAX_SCHED_STEPS) return 0;
    const std::vector<int32_t> e = equal_edges(batch_steps);
    return pxsom_batch_train_sched_workspace_bytes(n, c, k, PXSOM_F64, batch_steps, e.data(), batch_steps);
}

PXSOM_EXPORT int pxsom_batch_train_sched(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *wbuf_dev,
                                         double *stats_ring_dev, int xdim, int ydim, int phases, const int32_t *edges,
                                         int steps_per_pass, int g_begin, int g_end, int num_passes, double a0, double a1,
                                         double r0, double r1, double sum_quantum, void *workspace_dev, size_t workspace_bytes,
                                         int flags, pxsom_comm *comm, void *stream)
{
    return pxsom_batch_train_sched_from(x_dev, n, c, ldx, dtype, nullptr, wbuf_dev, stats_ring_dev, xdim, ydim, phases, edges, steps_per_pass,
                                        g_begin, g_end, num_passes, a0, a1, r0, r1, sum_quantum, workspace_dev, workspace_bytes, flags, comm,
                                        stream);
}

PXSOM_EXPORT int pxsom_batch_train_sched_from(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w0_dev,
                                              double *wbuf_dev, double *stats_ring_dev, int xdim, int ydim, int phases,
                                              const int32_t *edges, int steps_per_pass, int g_begin, int g_end, int num_passes,
                                              double a0, double a1, double r0, double r1, double sum_quantum, void *workspace_dev,
                                              size_t workspace_bytes, int flags, pxsom_comm *comm, void *stream)
{
    int rc = pxsom::check_matrix("pxsom_batch_train_sched", x_dev, n, c, ldx, dtype);
    if (rc) return rc;
    int qe = 0;
    if (!(sum_quantum >= 0.0) || (sum_quantum > 0.0 && frexp(sum_quantum, &qe) != 0.5))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_sched: sum_quantum must be 0 or a power of two");
    if (xdim < 1 || ydim < 1 || (int64_t)xdim * ydim > PXSOM_MAX_NODES)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_batch_train_sched: grid %dx%d outside [1, %d] nodes", xdim, ydim,
                           PXSOM_MAX_NODES);
    if ((rc = check_sched("pxsom_batch_train_sched", phases, edges, steps_per_pass))) return rc;
    if (num_passes < 1 || g_begin < 0 || g_end < g_begin || (int64_t)g_end > (int64_t)num_passes * steps_per_pass)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_sched: steps [%d, %d) of %d passes x %d", g_begin, g_end,
                           num_passes, steps_per_pass);
    if (!wbuf_dev || !stats_ring_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_sched: null pointer");
    const size_t need = pxsom_batch_train_sched_workspace_bytes(n, c, xdim * ydim, dtype, phases, edges, steps_per_pass);
    if (!workspace_dev || workspace_bytes < need)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "pxsom_batch_train_sched: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Sched sc{phases, steps_per_pass, edges};
    PXSOM_DISPATCH_DTYPE(dtype, x_dev, xp,
                         train_steps_typed<T>(xp, n, c, ldx, dtype, wbuf_dev, stats_ring_dev, xdim, ydim, sc, g_begin, g_end,
                                              num_passes, a0, a1, r0, r1, sum_quantum, reinterpret_cast<char *>(workspace_dev),
                                              flags, comm, st, g_begin == 0 ? w0_dev : nullptr));
}

// ---- the same run under FlowSOM's other distances (distf 1, 3, 4; DESIGN.md "K6m") ----------------------------------------
// Same state conventions and schedule; a step is the pending update (launch_batch_update, which also clears the next
// statistics buffer) followed by the prep + one-pass search-and-statistics launch of pxsom_metric_step.hip on the step's window
// of the row dealing -- the rows are read where they lie, whatever the step's width.
PXSOM_EXPORT size_t pxsom_batch_train_sched_metric_workspace_bytes(int64_t n, int c, int k, int dtype, int phases,
                                                                   const int32_t *edges, int steps_per_pass, int metric)
{
    if (n < 0 || !pxsom::dtype_ok(dtype)) return 0;
    if (check_sched("pxsom_batch_train_sched_metric_workspace_bytes", phases, edges, steps_per_pass)) return 0;
    const size_t step = pxsom_metric_step_workspace_bytes(c, k, metric);
    if (!step) return 0;
    // behind the prepared codebook: the labels of a step's rows (the steps that take two launches: pxsom_metric_step.h)
    const Sched sc{phases, steps_per_pass, edges};
    return pxsom::align_up(step, 256) + (size_t)std::max<int64_t>(sc.rows_max(n), 1) * sizeof(int32_t);
}

PXSOM_EXPORT int pxsom_batch_train_sched_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w0_dev,
                                                double *wbuf_dev, double *stats_ring_dev, int xdim, int ydim, int phases,
                                                const int32_t *edges, int steps_per_pass, int g_begin, int g_end, int num_passes,
                                                double a0, double a1, double r0, double r1, double sum_quantum, void *workspace_dev,
                                                size_t workspace_bytes, int flags, pxsom_comm *comm, int metric, void *stream)
{
    (void)flags;   // (the routes the flags choose among are the Euclidean ones)
    if (!pxsom_metric::metric_known(metric))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG,
                           "pxsom_batch_train_sched_metric: unknown metric %d (FlowSOM distf: 1 Manhattan, 2 Euclidean, 3 Chebyshev, "
                           "4 cosine)", metric);
    if (metric == PXSOM_METRIC_EUCLIDEAN)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED,
                           "pxsom_batch_train_sched_metric: metric 2 (Euclidean) has its own entry: pxsom_batch_train_sched_from");
    if (comm)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED,
                           "pxsom_batch_train_sched_metric: no exchange inside the library under this metric (run one step per "
                           "call and all-reduce ring[g % 3] in between)");
    int rc = pxsom::check_matrix("pxsom_batch_train_sched_metric", x_dev, n, c, ldx, dtype);
    if (rc) return rc;
    if (n > 0x7fffffffLL)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_sched_metric: n=%lld outside [0, 2^31)", (long long)n);
    int qe = 0;
    if (!(sum_quantum >= 0.0) || (sum_quantum > 0.0 && frexp(sum_quantum, &qe) != 0.5))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_sched_metric: sum_quantum must be 0 or a power of two");
    if (xdim < 1 || ydim < 1 || (int64_t)xdim * ydim > PXSOM_MAX_NODES)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_batch_train_sched_metric: grid %dx%d outside [1, %d] nodes", xdim, ydim,
                           PXSOM_MAX_NODES);
    if ((rc = check_sched("pxsom_batch_train_sched_metric", phases, edges, steps_per_pass))) return rc;
    if (num_passes < 1 || g_begin < 0 || g_end < g_begin || (int64_t)g_end > (int64_t)num_passes * steps_per_pass)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_sched_metric: steps [%d, %d) of %d passes x %d", g_begin, g_end,
                           num_passes, steps_per_pass);
    if (!wbuf_dev || !stats_ring_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_sched_metric: null pointer");
    const int k = xdim * ydim;
    const size_t need = pxsom_batch_train_sched_metric_workspace_bytes(n, c, k, dtype, phases, edges, steps_per_pass, metric);
    if (!workspace_dev || workspace_bytes < need)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "pxsom_batch_train_sched_metric: workspace %zu < %zu bytes", workspace_bytes, need);
    int32_t *step_labels = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(workspace_dev) +
                                                       pxsom::align_up(pxsom_metric_step_workspace_bytes(c, k, metric), 256));
    if (pxsom::row_view_active())
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_batch_train_sched_metric: the metric kernels do not take row views");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Sched sc{phases, steps_per_pass, edges};
    const size_t nstats = (size_t)k * (c + 1), nw = (size_t)k * c;
    const int64_t span = (int64_t)num_passes * sc.phases;
    const double qmagic = (dtype == PXSOM_F64 && sum_quantum > 0.0) ? 6755399441055744.0 /* 1.5 * 2^52 */ * sum_quantum : 0.0;
    double *wbuf = wbuf_dev, *ring = stats_ring_dev;
    for (int gg = g_begin; gg < g_end; gg++) {
        const int g = gg % sc.steps;
        double *w_prev = wbuf + (size_t)((gg + 1) % 2) * nw, *w_cur = wbuf + (size_t)(gg % 2) * nw;
        double *s_prev = ring + (size_t)((gg + 2) % 3) * nstats, *s_cur = ring + (size_t)(gg % 3) * nstats,
               *s_next = ring + (size_t)((gg + 1) % 3) * nstats;
        if (gg == 0) {   // the run's first codebook; ring[0] (this step's statistics) and ring[1] (the next step's) are adjacent
            if (w0_dev && w0_dev != wbuf) PXSOM_HIP_TRY(hipMemcpyAsync(wbuf, w0_dev, nw * sizeof(double), hipMemcpyDeviceToDevice, st));
            PXSOM_HIP_TRY(hipMemsetAsync(ring, 0, 2 * nstats * sizeof(double), st));
        } else {         // W_g from W_{g-1} and the (all-reduced) statistics of step g - 1; the same launch clears ring[(g+1) % 3]
            double thr = 0.0, alpha = 0.0;
            batch_schedule(sc.pos(gg - 1), span, a0, a1, r0, r1, &thr, &alpha);
            rc = launch_batch_update(w_cur, w_prev, xdim, ydim, c, s_prev, s_prev + nw, thr, alpha, s_next, (int)nstats, st);
            if (rc) return rc;
        }
        if (sc.width(g) < 1 || n == 0) continue;   // an empty step
        rc = pxsom_metric::assign_sums_step(x_dev, n, c, ldx, dtype, w_cur, k, sc.phases, sc.e0(g), sc.e0(g) + sc.width(g), nullptr,
                                            step_labels, s_cur, qmagic, reinterpret_cast<char *>(workspace_dev), metric, st);
        if (rc) return rc;
    }
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_batch_train_steps(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *wbuf_dev,
                                         double *stats_ring_dev, int xdim, int ydim, int batch_steps, int g_begin,
                                         int g_end, int total_steps, double a0, double a1, double r0, double r1,
                                         void *workspace_dev, size_t workspace_bytes, int flags, void *stream)
{
    return pxsom_batch_train_steps_sharded(x_dev, n, c, ldx, dtype, wbuf_dev, stats_ring_dev, xdim, ydim, batch_steps,
                                           g_begin, g_end, total_steps, a0, a1, r0, r1, workspace_dev, workspace_bytes,
                                           flags, nullptr, stream);
}

// equal steps (the round-1/2 entry points): total_steps = num_passes * batch_steps
PXSOM_EXPORT int pxsom_batch_train_steps_sharded(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype,
                                                 double *wbuf_dev, double *stats_ring_dev, int xdim, int ydim,
                                                 int batch_steps, int g_begin, int g_end, int total_steps, double a0,
                                                 double a1, double r0, double r1, void *workspace_dev,
                                                 size_t workspace_bytes, int flags, pxsom_comm *comm, void *stream)
{
    if (batch_steps < 1 || batch_steps > PXSOM_MAX_SCHED_STEPS || total_steps < 1 || total_steps % batch_steps != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_steps: steps [%d, %d) of %d, %d per pass (1..%d, whole passes)",
                           g_begin, g_end, total_steps, batch_steps, PXSOM_MAX_SCHED_STEPS);
    const std::vector<int32_t> e = equal_edges(batch_steps);
    return pxsom_batch_train_sched(x_dev, n, c, ldx, dtype, wbuf_dev, stats_ring_dev, xdim, ydim, batch_steps, e.data(),
                                   batch_steps, g_begin, g_end, total_steps / batch_steps, a0, a1, r0, r1, 0.0, workspace_dev,
                                   workspace_bytes, flags, comm, stream);
}

namespace {
int finish_at(const double *wbuf_dev, const double *stats_ring_dev, int xdim, int ydim, int c, int steps_done, int64_t pos,
              int64_t span, double a0, double a1, double r0, double r1, double *w_out_dev, void *stream)
{
    const int k = xdim * ydim, g = steps_done - 1;
    const size_t nw = (size_t)k * c, nstats = (size_t)k * (c + 1);
    const double *w_last = wbuf_dev + (size_t)(g % 2) * nw, *s_last = stats_ring_dev + (size_t)(g % 3) * nstats;
    double thr, alpha;
    batch_schedule(pos, span, a0, a1, r0, r1, &thr, &alpha);
    // one launch: the update reads W of the last step where it lies and writes the result to w_out (no copy in front)
    return launch_batch_update(w_out_dev, w_last, xdim, ydim, c, s_last, s_last + nw, thr, alpha, nullptr, 0,
                               reinterpret_cast<hipStream_t>(stream));
}
}  // namespace

PXSOM_EXPORT int pxsom_batch_train_sched_finish(const double *wbuf_dev, const double *stats_ring_dev, int xdim, int ydim,
                                                int c, int phases, const int32_t *edges, int steps_per_pass, int steps_done,
                                                int num_passes, double a0, double a1, double r0, double r1,
                                                double *w_out_dev, void *stream)
{
    if (xdim < 1 || ydim < 1 || (int64_t)xdim * ydim > PXSOM_MAX_NODES || c < 1 || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_batch_train_finish: shape %dx%d x %d", xdim, ydim, c);
    int rc = check_sched("pxsom_batch_train_finish", phases, edges, steps_per_pass);
    if (rc) return rc;
    if (!wbuf_dev || !stats_ring_dev || !w_out_dev || num_passes < 1 || steps_done < 1 ||
        (int64_t)steps_done > (int64_t)num_passes * steps_per_pass)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_finish: bad arguments");
    const Sched sc{phases, steps_per_pass, edges};
    return finish_at(wbuf_dev, stats_ring_dev, xdim, ydim, c, steps_done, sc.pos(steps_done - 1), (int64_t)num_passes * phases,
                     a0, a1, r0, r1, w_out_dev, stream);
}

// equal steps: the position of step g of total_steps is g / total_steps whatever the steps per pass
PXSOM_EXPORT int pxsom_batch_train_finish(const double *wbuf_dev, const double *stats_ring_dev, int xdim, int ydim, int c,
                                          int steps_done, int total_steps, double a0, double a1, double r0, double r1,
                                          double *w_out_dev, void *stream)
{
    if (xdim < 1 || ydim < 1 || (int64_t)xdim * ydim > PXSOM_MAX_NODES || c < 1 || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_batch_train_finish: shape %dx%d x %d", xdim, ydim, c);
    if (!wbuf_dev || !stats_ring_dev || !w_out_dev || steps_done < 1 || steps_done > total_steps)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_batch_train_finish: bad arguments");
    return finish_at(wbuf_dev, stats_ring_dev, xdim, ydim, c, steps_done, steps_done - 1, total_steps, a0, a1, r0, r1, w_out_dev,
                     stream);
}

// 1: the steps of this (matrix, shape, schedule) take the one-launch fused kernel; 0: the launch-per-phase route.  A
// multi-rank job agrees on the route before it starts (MIN over the ranks; PXSOM_TRAIN_UNFUSED for everyone otherwise):
// the two routes produce the same statistics but round the codebook's last bits differently.
PXSOM_EXPORT int pxsom_batch_train_fused_route(const void *x_dev, int c, int64_t ldx, int dtype, int xdim, int ydim, int phases)
{
    if (!pxsom::dtype_ok(dtype) || phases < 1) return 0;
    const int64_t gs = (int64_t)phases * ldx;
    PXSOM_DISPATCH_DTYPE(dtype, x_dev, xp, pxsom_bmu::step_fused_shape<T>(xp, 1, c, ldx, xdim, ydim, gs));
}

// ---- reproducible statistics for binary64 rows (include/pxsom.h) ----------------------------------------------------
PXSOM_EXPORT double pxsom_exact_sum_quantum(double value_bound, int64_t rows_bound)
{
    if (!(value_bound > 0.0) || !(value_bound <= DBL_MAX)) return 0.0;   // all-zero / unbounded data: nothing to round to
    if (rows_bound < 2) rows_bound = 2;
    // sums stay below rows * bound < 2^e; with q = 2^(e - 52) they are multiples of q below 2^52 q: exactly representable,
    // and so is every partial sum in any order
    int e = 0;
    frexp(value_bound, &e);                    // value_bound < 2^e
    int r = 0;
    while (((int64_t)1 << r) < rows_bound && r < 62) r++;
    return ldexp(1.0, e + r - 52);
}

namespace {
template <typename T>
__global__ __launch_bounds__(256) void absmax_kernel(const T *__restrict__ x, int64_t n, int c, int64_t ldx,
                                                     unsigned long long *out)
{
    double m = 0.0;
    const int64_t total = n * c;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / c;
        const double v = fabs((double)x[row * ldx + (e - row * c)]);
        if (v <= DBL_MAX && v > m) m = v;      // (NaN and Inf fail the first test)
    }
    m = -pxsom::wave_min_f64(-m);
    // non-negative binary64 numbers order like their bit patterns
    if ((threadIdx.x & 63) == 0 && m > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(m));
}
}  // namespace

PXSOM_EXPORT int pxsom_absmax(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *out_dev, void *stream)
{
    int rc = pxsom::check_matrix("pxsom_absmax", x_dev, n, c, ldx, dtype);
    if (rc) return rc;
    if (!out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_absmax: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(double), st));
    if (n == 0) return PXSOM_OK;
    const int64_t grid = std::min<int64_t>((n * c + 255) / 256, (int64_t)pxsom::device_cu_count() * 8);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(out_dev);
    if (dtype == PXSOM_F32)
        hipLaunchKernelGGL(absmax_kernel<float>, dim3((unsigned)grid), dim3(256), 0, st, static_cast<const float *>(x_dev), n, c, ldx, out);
    else if (dtype == PXSOM_F16)
        hipLaunchKernelGGL(absmax_kernel<_Float16>, dim3((unsigned)grid), dim3(256), 0, st, static_cast<const _Float16 *>(x_dev), n, c, ldx, out);
    else
        hipLaunchKernelGGL(absmax_kernel<double>, dim3((unsigned)grid), dim3(256), 0, st, static_cast<const double *>(x_dev), n, c, ldx, out);
    PXSOM_LAUNCH_CHECK("absmax_kernel");
    return PXSOM_OK;
}
