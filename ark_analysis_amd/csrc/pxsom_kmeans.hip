// pxsom_kmeans.hip -- Lloyd's k-means over the rows of one matrix for P independent problems at once (K19).
//
// reference: sklearn.cluster.KMeans(algorithm="lloyd") as ark/analysis/spatial_analysis_utils.py fits it, once per k of a
// sweep (compute_kmeans_inertia, compute_kmeans_silhouette) or with ten restarts (generate_cluster_labels).  Here every
// (k, restart) is one problem: its own centres [k_p, d], tolerance and iteration limit over the shared rows x[n, d]
// (binary64, d <= 64, k_p <= 32).  One iteration is one pass over the rows per group of still-active problems.
//
// The assignment.  dist(x, c) = sum_j (x_j - c_j)^2 in binary64 with j ascending, every difference, product and sum
// rounded on its own (this file is compiled with floating-point contraction off: no fused multiply-add); the centres are
// tried in ascending order and only a strictly smaller distance replaces the best, so the first minimum wins.  A thread
// owns one row, held in DMAX registers under static indices (DMAX = 8, 16, 32 or 64, as K15); the centres of the group sit
// in LDS padded with zeros to a multiple of four columns and are read as broadcasts.
//
// The sums.  Rows are cut into fixed blocks of 256 (block b = rows [256 b, 256 b + 256), whatever the grid); a workgroup
// takes blocks b = blockIdx.x, blockIdx.x + gridDim.x, ...  For a block the 256 labels of every problem are kept in LDS
// (one byte each) and one thread per (centre, column) adds the block's rows of that centre in row order into a register,
// then stores the partial table entry partial[b, centre, column] (the count rides in column d).  The winning distances
// of a block are added per problem by a fixed butterfly over each wave, then over the four waves in order.  A second
// kernel folds the partial tables in block order (one thread per entry, b ascending).  No floating-point atomic
// anywhere: the order of every sum is a function of n alone, so the bits do not depend on the number of workgroups, on
// which problems share a group, or on the run.  (The other choice, the batch trainer's fixed-point quantum, would
// round the rows that enter the sums; the blocks leave them as they are.)
//
// The grouping rule.  A group's LDS holds, for its problems g with K = sum k_g centres and dp = d rounded up to 4:
//     K * dp * 8     the centres
//   + |g| * 4 * 8    the per-wave sums of the winning distances
//   + |g| * 256      the block's labels
//   + K * 6          which problem, which centre and which row of the centre table a group-wide centre index is
// bytes, and must stay within 65536 (two workgroups per CU of the 160 KiB, no partial table in LDS: those live in
// registers).  The active problems are taken in order and a group is closed when the next problem would not fit or it
// holds 32.  One problem at k = 32, d = 64 takes 16864 bytes, so ten such restarts are four groups (3 + 3 + 3 + 1) and
// four passes per iteration; the sweep k = 2 .. 10 at d = 20 (54 centres) is one.  Which group a problem is in changes
// nothing it computes.
//
// The update (one workgroup per problem, after the fold), scikit-learn's Lloyd iteration as documented:
//   - an empty cluster takes the row that is currently farthest from its own centre (ties: the lower row); several empty
//     clusters, in ascending order, take the farthest rows in that order; the row leaves the sum and count of the
//     cluster it was assigned to;
//   - centre = sum / count (a cluster left with count 0 keeps its centre);
//   - shift = sum_c (sum_j (new - old)^2), j ascending inside c ascending, every operation rounded on its own.
// The host loop reads (labels changed?, shift, inertia) per problem after every iteration: a problem stops when no label
// changed (its inertia is that assignment's), or goes to one closing assignment pass (labels and inertia only) when
// shift <= tol or the iteration limit is reached.  Stopped problems are in no later group.
//
// Memory safety does not depend on the rows: a NaN distance is never smaller, so a label stays in [0, k_p) and indexes
// nothing outside the tables; the farthest-row search skips NaN and yields a row in [0, n) or nothing.
#include <vector>

#include "pxsom_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;        // threads per workgroup = rows per block
constexpr int kWaves = kBlock / 64;
constexpr int kMaxD = 64;
constexpr int kMaxK = 32;
constexpr int kMaxGroup = 32;      // problems per group
constexpr int kMaxProblems = 4096;
constexpr size_t kLdsBudget = 65536;
constexpr int kSumLd = kMaxD + 1;  // the update kernel's LDS table: d sums and the count per centre
constexpr int kStatus = 4;         // doubles per problem the host reads back: shift, inertia, changed, spare

struct Group {
    int np, sumk;
    int pid[kMaxGroup], k[kMaxGroup], coff[kMaxGroup];   // problem, its k, its first row in the centre table
};

struct Ctl {   // one active problem of an iteration, for the update kernel
    int pid, k, coff, final_pass;
    double tol;
};

inline int pad4(int d) { return (d + 3) / 4 * 4; }

inline size_t group_lds_bytes(int sumk, int np, int d)
{
    return (size_t)sumk * pad4(d) * 8 + (size_t)np * kWaves * 8 + (size_t)np * kBlock + (size_t)sumk * 6;
}

template <int DMAX>
__global__ __launch_bounds__(kBlock) void kmeans_assign_kernel(const double *__restrict__ x, int64_t n, int d, Group g,
                                                               const double *__restrict__ centres,
                                                               int32_t *__restrict__ labels, double *__restrict__ dist,
                                                               int32_t *__restrict__ changed,
                                                               double *__restrict__ partial, double *__restrict__ ipart,
                                                               int total_k, int n_problems, int64_t nblocks)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int dp = (d + 3) / 4 * 4;
    double *cen = smem;                                       // [sumk, dp]
    double *wpart = cen + (size_t)g.sumk * dp;                // [np, kWaves]
    int32_t *own_row = reinterpret_cast<int32_t *>(wpart + g.np * kWaves);   // [sumk]
    uint8_t *lab = reinterpret_cast<uint8_t *>(own_row + g.sumk);           // [np, kBlock]
    uint8_t *own_p = lab + g.np * kBlock;                     // [sumk]
    uint8_t *own_c = own_p + g.sumk;                          // [sumk]

    const int tid = threadIdx.x;
    {
        int loff = 0;
        for (int p = 0; p < g.np; ++p) {
            const int kp = g.k[p];
            for (int idx = tid; idx < kp * dp; idx += kBlock) {
                const int c = idx / dp, t = idx - c * dp;
                cen[(size_t)(loff + c) * dp + t] = t < d ? centres[(int64_t)(g.coff[p] + c) * d + t] : 0.0;
            }
            for (int c = tid; c < kp; c += kBlock) {
                own_p[loff + c] = (uint8_t)p;
                own_c[loff + c] = (uint8_t)c;
                own_row[loff + c] = g.coff[p] + c;
            }
            loff += kp;
        }
    }
    __syncthreads();

    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int64_t base = b * kBlock;
        const int64_t i = base + tid;
        const bool has_row = i < n;
        const int rows_here = n - base < kBlock ? (int)(n - base) : kBlock;

        double xi[DMAX];
#pragma unroll
        for (int t = 0; t < DMAX; ++t) xi[t] = (has_row && t < d) ? x[i * d + t] : 0.0;

        int loff = 0;
        for (int p = 0; p < g.np; ++p) {
            const int kp = g.k[p];
            const double *cp = cen + (size_t)loff * dp;
            double best = __builtin_inf();
            int bi = 0;
            for (int c = 0; c < kp; ++c) {
                const double *cc = cp + c * dp;
                double s = 0.0;
#pragma unroll
                for (int t0 = 0; t0 < DMAX; t0 += 4) {
                    if (t0 < d) {
#pragma unroll
                        for (int t = t0; t < t0 + 4; ++t) {
                            const double diff = xi[t] - cc[t];
                            const double sq = diff * diff;
                            s = s + sq;      // a padded column adds (0 - 0)^2 = +0: the sum is unchanged
                        }
                    }
                }
                if (s < best) {
                    best = s;
                    bi = c;
                }
            }
            const int pid = g.pid[p];
            if (has_row) {
                const int64_t at = (int64_t)pid * n + i;
                if (labels[at] != bi) changed[pid] = 1;     // an integer flag: every writer stores the same 1
                labels[at] = bi;
                dist[at] = best;
            }
            lab[p * kBlock + tid] = has_row ? (uint8_t)bi : (uint8_t)255;
            double v = has_row ? best : 0.0;
            for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
            if ((tid & 63) == 0) wpart[p * kWaves + (tid >> 6)] = v;
            loff += kp;
        }
        __syncthreads();

        for (int idx = tid; idx < g.sumk * d; idx += kBlock) {
            const int gc = idx / d, j = idx - gc * d;
            const int p = own_p[gc];
            const uint8_t c = own_c[gc];
            const uint8_t *lp = lab + p * kBlock;
            const double *xp = x + base * d + j;
            double acc = 0.0;
            int cnt = 0;
            for (int r = 0; r < rows_here; ++r) {
                const bool mine = lp[r] == c;
                const double v = xp[(int64_t)r * d];
                acc = acc + (mine ? v : 0.0);
                cnt += mine ? 1 : 0;
            }
            double *out = partial + ((int64_t)b * total_k + own_row[gc]) * (d + 1);
            out[j] = acc;
            if (j == 0) out[d] = (double)cnt;
        }
        if (tid < g.np) {
            const double *w = wpart + tid * kWaves;
            ipart[(int64_t)b * n_problems + g.pid[tid]] = ((w[0] + w[1]) + w[2]) + w[3];
        }
        __syncthreads();   // lab and wpart are free for the next block
    }
}

__global__ __launch_bounds__(kBlock) void kmeans_update_kernel(const double *__restrict__ x, int64_t n, int d,
                                                               const Ctl *__restrict__ ctl, double *__restrict__ centres,
                                                               const int32_t *__restrict__ labels,
                                                               const double *__restrict__ dist,
                                                               int32_t *__restrict__ changed,
                                                               const double *__restrict__ partial,
                                                               const double *__restrict__ ipart, int total_k,
                                                               int n_problems, int64_t nblocks, double *__restrict__ status)
{
    __shared__ double sums[kMaxK * kSumLd];
    __shared__ double shiftc[kMaxK];
    __shared__ double red_v[kBlock];
    __shared__ int64_t red_i[kBlock];
    __shared__ int64_t taken[kMaxK];
    __shared__ int empties[kMaxK];
    __shared__ int n_empty;

    const int tid = threadIdx.x;
    const Ctl me = ctl[blockIdx.x];
    const int k = me.k, ld = d + 1;

    // the fold: entry (c, j) of the problem's table over the blocks in order; one more entry is the inertia
    for (int idx = tid; idx <= k * ld; idx += kBlock) {
        double acc = 0.0;
        if (idx < k * ld) {
            const double *src = partial + (int64_t)me.coff * ld + idx;
            for (int64_t b = 0; b < nblocks; ++b) acc = acc + src[b * total_k * ld];
            sums[(idx / ld) * kSumLd + idx % ld] = acc;
        } else {
            for (int64_t b = 0; b < nblocks; ++b) acc = acc + ipart[b * n_problems + me.pid];
            status[me.pid * kStatus + 1] = acc;
        }
    }
    if (tid == 0) {
        status[me.pid * kStatus + 2] = changed[me.pid] ? 1.0 : 0.0;
        changed[me.pid] = 0;
        if (me.final_pass) status[me.pid * kStatus + 0] = 0.0;
    }
    if (me.final_pass) return;   // the closing pass: labels and inertia only
    __syncthreads();

    if (tid == 0) {
        int m = 0;
        for (int c = 0; c < k; ++c)
            if (sums[c * kSumLd + d] == 0.0) empties[m++] = c;
        n_empty = m;
    }
    __syncthreads();

    const double *dp = dist + (int64_t)me.pid * n;
    const int m_empty = n_empty;
    for (int e = 0; e < m_empty; ++e) {
        // the farthest row not yet taken: the larger distance, on a tie the lower row
        double bv = -1.0;
        int64_t bi = -1;
        for (int64_t i = tid; i < n; i += kBlock) {
            const double v = dp[i];
            bool free_row = true;
            for (int u = 0; u < e; ++u) free_row = free_row && taken[u] != i;
            if (free_row && v > bv) {
                bv = v;
                bi = i;
            }
        }
        red_v[tid] = bv;
        red_i[tid] = bi;
        __syncthreads();
        for (int w = kBlock / 2; w >= 1; w >>= 1) {
            if (tid < w) {
                const double ov = red_v[tid + w];
                const int64_t oi = red_i[tid + w];
                const bool take = oi >= 0 && (red_i[tid] < 0 || ov > red_v[tid] || (ov == red_v[tid] && oi < red_i[tid]));
                if (take) {
                    red_v[tid] = ov;
                    red_i[tid] = oi;
                }
            }
            __syncthreads();
        }
        const int64_t far = red_i[0];
        if (tid == 0) taken[e] = far;
        if (far >= 0 && far < n) {
            const int into = empties[e];
            int from = labels[(int64_t)me.pid * n + far];
            from = from < 0 ? 0 : (from >= k ? k - 1 : from);
            if (tid < d) {
                const double v = x[far * d + tid];
                sums[from * kSumLd + tid] = sums[from * kSumLd + tid] - v;
                sums[into * kSumLd + tid] = v;
            } else if (tid == d) {
                sums[from * kSumLd + d] = sums[from * kSumLd + d] - 1.0;
                sums[into * kSumLd + d] = 1.0;
            }
        }
        __syncthreads();
    }

    if (tid < k) {
        const double cnt = sums[tid * kSumLd + d];
        double sh = 0.0;
        for (int j = 0; j < d; ++j) {
            const double old = centres[(int64_t)(me.coff + tid) * d + j];
            const double now = cnt > 0.0 ? sums[tid * kSumLd + j] / cnt : old;
            const double diff = now - old;
            const double sq = diff * diff;
            sh = sh + sq;
            sums[tid * kSumLd + j] = now;
        }
        shiftc[tid] = sh;
    }
    __syncthreads();
    for (int idx = tid; idx < k * d; idx += kBlock)
        centres[(int64_t)me.coff * d + idx] = sums[(idx / d) * kSumLd + idx % d];
    if (tid == 0) {
        double tot = 0.0;
        for (int c = 0; c < k; ++c) tot = tot + shiftc[c];
        status[me.pid * kStatus + 0] = tot;
    }
}

template <int DMAX>
void launch_assign(unsigned grid, size_t lds, hipStream_t st, const double *x, int64_t n, int d, const Group &g,
                   const double *centres, int32_t *labels, double *dist, int32_t *changed, double *partial, double *ipart,
                   int total_k, int n_problems, int64_t nblocks)
{
    hipLaunchKernelGGL(kmeans_assign_kernel<DMAX>, dim3(grid), dim3(kBlock), lds, st, x, n, d, g, centres, labels, dist,
                       changed, partial, ipart, total_k, n_problems, nblocks);
}

// the workspace: dist [P, n], partial [nblocks, total_k, d + 1], ipart [nblocks, P], status [P, 4] (doubles), then
// ctl [P] and changed [P]
struct Layout {
    size_t dist, partial, ipart, status, ctl, changed, total;
};

Layout make_layout(int64_t n, int d, int n_problems, int total_k)
{
    const size_t nblocks = (size_t)((n + kBlock - 1) / kBlock);
    Layout l;
    size_t at = 0;
    l.dist = at;
    at += pxsom::align_up((size_t)n_problems * (size_t)n * 8, 256);
    l.partial = at;
    at += pxsom::align_up(nblocks * (size_t)total_k * (size_t)(d + 1) * 8, 256);
    l.ipart = at;
    at += pxsom::align_up(nblocks * (size_t)n_problems * 8, 256);
    l.status = at;
    at += pxsom::align_up((size_t)n_problems * kStatus * 8, 256);
    l.ctl = at;
    at += pxsom::align_up((size_t)n_problems * sizeof(Ctl), 256);
    l.changed = at;
    at += pxsom::align_up((size_t)n_problems * 4, 256);
    l.total = at;
    return l;
}

int check_sizes(const char *fn, int64_t n, int d, int n_problems, const int32_t *k_host, int *total_k)
{
    if (d < 1 || d > kMaxD)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: d=%d is outside 1 .. %d, the device route's limit", fn, d, kMaxD);
    if (n < 0 || n > 0x7fffffff)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld is outside 0 .. 2^31 - 1", fn, (long long)n);
    if (n_problems < 1 || n_problems > kMaxProblems)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_problems=%d is outside 1 .. %d", fn, n_problems, kMaxProblems);
    if (!k_host) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null k_host", fn);
    int sum = 0;
    for (int p = 0; p < n_problems; ++p) {
        if (k_host[p] < 1 || k_host[p] > kMaxK)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: k=%d (problem %d) is outside 1 .. %d, the device route's limit",
                               fn, k_host[p], p, kMaxK);
        sum += k_host[p];
    }
    *total_k = sum;
    return PXSOM_OK;
}

// the groups of the listed problems, by the rule of the header: calls emit(group) for each and returns their number
template <typename F>
int for_each_group(int d, const std::vector<int> &active, const int32_t *k_host, const std::vector<int> &coff, F emit)
{
    int groups = 0;
    Group g = {};
    for (size_t a = 0; a < active.size(); ++a) {
        const int p = active[a];
        if (g.np > 0 && (g.np == kMaxGroup || group_lds_bytes(g.sumk + k_host[p], g.np + 1, d) > kLdsBudget)) {
            emit(g);
            ++groups;
            g = Group{};
        }
        g.pid[g.np] = p;
        g.k[g.np] = k_host[p];
        g.coff[g.np] = coff[p];
        g.sumk += k_host[p];
        ++g.np;
    }
    if (g.np > 0) {
        emit(g);
        ++groups;
    }
    return groups;
}

std::vector<int> centre_offsets(int n_problems, const int32_t *k_host)
{
    std::vector<int> coff(n_problems);
    int at = 0;
    for (int p = 0; p < n_problems; ++p) {
        coff[p] = at;
        at += k_host[p];
    }
    return coff;
}

}  // namespace

PXSOM_EXPORT size_t pxsom_kmeans_workspace_bytes(int64_t n, int d, int n_problems, const int32_t *k_host)
{
    int total_k = 0;
    if (check_sizes("pxsom_kmeans_workspace_bytes", n, d, n_problems, k_host, &total_k) != PXSOM_OK) return 0;
    return make_layout(n, d, n_problems, total_k).total;
}

PXSOM_EXPORT int pxsom_kmeans_group_count(int d, int n_problems, const int32_t *k_host)
{
    int total_k = 0;
    const int rc = check_sizes("pxsom_kmeans_group_count", 0, d, n_problems, k_host, &total_k);
    if (rc != PXSOM_OK) return rc;
    std::vector<int> all(n_problems);
    for (int p = 0; p < n_problems; ++p) all[p] = p;
    return for_each_group(d, all, k_host, centre_offsets(n_problems, k_host), [](const Group &) {});
}

PXSOM_EXPORT int pxsom_kmeans_lloyd(const double *x_dev, int64_t n, int d, int n_problems, const int32_t *k_host,
                                    double *centres_dev, const double *tol_host, const int32_t *max_iter_host,
                                    int32_t *labels_dev, double *inertia_host, int32_t *iters_host, void *workspace_dev,
                                    size_t workspace_bytes, int workgroups, void *stream)
{
    const char *fn = "pxsom_kmeans_lloyd";
    int total_k = 0;
    const int rc = check_sizes(fn, n, d, n_problems, k_host, &total_k);
    if (rc != PXSOM_OK) return rc;
    if (!tol_host || !max_iter_host || !inertia_host || !iters_host)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null host array", fn);
    if (workgroups < 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workgroups=%d < 0", fn, workgroups);
    for (int p = 0; p < n_problems; ++p) {
        inertia_host[p] = 0.0;
        iters_host[p] = 0;
    }
    if (n == 0) return PXSOM_OK;
    for (int p = 0; p < n_problems; ++p) {
        if (k_host[p] > n)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: k=%d (problem %d) exceeds the n=%lld rows", fn, k_host[p], p,
                               (long long)n);
        if (max_iter_host[p] < 1)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: max_iter=%d (problem %d) < 1", fn, max_iter_host[p], p);
        if (!(tol_host[p] >= 0.0))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: tol (problem %d) is negative or NaN", fn, p);
    }
    if (!x_dev || !centres_dev || !labels_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
    const Layout lay = make_layout(n, d, n_problems, total_k);
    if (!workspace_dev || workspace_bytes < lay.total)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, lay.total);
    if (reinterpret_cast<uintptr_t>(workspace_dev) % 8 != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workspace not aligned to 8 bytes", fn);

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_dev);
    double *dist = reinterpret_cast<double *>(ws + lay.dist);
    double *partial = reinterpret_cast<double *>(ws + lay.partial);
    double *ipart = reinterpret_cast<double *>(ws + lay.ipart);
    double *status = reinterpret_cast<double *>(ws + lay.status);
    Ctl *ctl = reinterpret_cast<Ctl *>(ws + lay.ctl);
    int32_t *changed = reinterpret_cast<int32_t *>(ws + lay.changed);

    const int64_t nblocks = (n + kBlock - 1) / kBlock;
    const int64_t wanted = workgroups > 0 ? workgroups : 2 * (int64_t)pxsom::device_cu_count();
    const unsigned grid = (unsigned)(wanted < nblocks ? (wanted < 1 ? 1 : wanted) : nblocks);
    const std::vector<int> coff = centre_offsets(n_problems, k_host);

    // no label yet: the first assignment changes every one of them
    PXSOM_HIP_TRY(hipMemsetAsync(labels_dev, 0xff, (size_t)n_problems * (size_t)n * 4, st));
    PXSOM_HIP_TRY(hipMemsetAsync(changed, 0, (size_t)n_problems * 4, st));

    enum { kRun = 0, kClose = 1, kDone = 2 };
    std::vector<int> state(n_problems, kRun), active;
    std::vector<Ctl> ctl_host;
    std::vector<double> status_host((size_t)n_problems * kStatus);
    for (;;) {
        active.clear();
        ctl_host.clear();
        for (int p = 0; p < n_problems; ++p) {
            if (state[p] == kDone) continue;
            active.push_back(p);
            ctl_host.push_back(Ctl{p, k_host[p], coff[p], state[p] == kClose ? 1 : 0, tol_host[p]});
        }
        if (active.empty()) break;
        PXSOM_HIP_TRY(hipMemcpyAsync(ctl, ctl_host.data(), ctl_host.size() * sizeof(Ctl), hipMemcpyHostToDevice, st));
        for_each_group(d, active, k_host, coff, [&](const Group &g) {
            const size_t lds = group_lds_bytes(g.sumk, g.np, d);
            if (d <= 8)
                launch_assign<8>(grid, lds, st, x_dev, n, d, g, centres_dev, labels_dev, dist, changed, partial, ipart,
                                 total_k, n_problems, nblocks);
            else if (d <= 16)
                launch_assign<16>(grid, lds, st, x_dev, n, d, g, centres_dev, labels_dev, dist, changed, partial, ipart,
                                  total_k, n_problems, nblocks);
            else if (d <= 32)
                launch_assign<32>(grid, lds, st, x_dev, n, d, g, centres_dev, labels_dev, dist, changed, partial, ipart,
                                  total_k, n_problems, nblocks);
            else
                launch_assign<64>(grid, lds, st, x_dev, n, d, g, centres_dev, labels_dev, dist, changed, partial, ipart,
                                  total_k, n_problems, nblocks);
        });
        PXSOM_LAUNCH_CHECK("kmeans_assign_kernel");
        hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)active.size()), dim3(kBlock), 0, st, x_dev, n, d, ctl,
                           centres_dev, labels_dev, dist, changed, partial, ipart, total_k, n_problems, nblocks, status);
        PXSOM_LAUNCH_CHECK("kmeans_update_kernel");
        PXSOM_HIP_TRY(hipMemcpyAsync(status_host.data(), status, status_host.size() * 8, hipMemcpyDeviceToHost, st));
        PXSOM_HIP_TRY(hipStreamSynchronize(st));
        for (size_t a = 0; a < active.size(); ++a) {
            const int p = active[a];
            const double *s = &status_host[(size_t)p * kStatus];
            inertia_host[p] = s[1];
            if (state[p] == kClose) {
                state[p] = kDone;
                continue;
            }
            ++iters_host[p];
            if (s[2] == 0.0)
                state[p] = kDone;                                   // the labels of the iteration before: settled
            else if (s[0] <= tol_host[p] || iters_host[p] >= max_iter_host[p])
                state[p] = kClose;
        }
    }
    return PXSOM_OK;
}
