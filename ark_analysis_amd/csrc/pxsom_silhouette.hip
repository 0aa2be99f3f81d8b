// pxsom_silhouette.hip -- silhouette coefficients of the rows of a matrix under M labelings at once (K15).
//
// reference: sklearn.metrics.silhouette_samples / silhouette_score (Euclidean) as ark/analysis/spatial_analysis_utils.py
// compute_kmeans_silhouette calls them once per k.  The distances do not depend on the labeling; the N x N matrix is never
// built.  For labeling m, row i and cluster c
//   S[m, i, c] = sum over j with labels[m, j] == c of sqrt(sum_t (X[i, t] - X[j, t])^2)
// in binary64: every difference is one rounding, the squares enter the sum through one fused multiply-add each (one
// rounding per term, all terms >= 0), the square root is the correctly rounded one.  A duplicate row gives exactly 0, and
// j == i needs no special case.
//
// Shape.  The grid is (blocks of 256 rows) x (clusters) x (labelings).  A thread owns one row, held in DMAX registers
// under static indices (DMAX = 8, 16, 32 or 64, the smallest that holds d; dimensions are walked four at a time under a
// wave-uniform test, the row padded with zeros to a multiple of four).  The candidates of labeling m come through `order`,
// a permutation that lists the rows of cluster 0, then of cluster 1, ...: the workgroup of (m, c) walks that cluster's run
// [start, start + count) in tiles of 4096 / DMAX candidates gathered into LDS and read as broadcasts, adds every distance
// to one accumulator per thread in the order of the run, and stores S[m, i, c] once.  There is no run-boundary logic and no
// atomic on a floating-point value: the order of every sum is fixed by `order` alone.
//
// Four stream-ordered launches: cluster sizes (an integer histogram of the labels in LDS), the sums above, the samples
//   a = S[i, c_i] / (n_{c_i} - 1),  b = min over c != c_i with n_c > 0 of S[i, c] / n_c,  s = (b - a) / max(a, b),
//   s = 0 when n_{c_i} == 1 or when the quotient is NaN
// (one thread per row), and their mean per labeling (one workgroup: a strided serial sum per thread, then a tree).
//
// Memory safety does not depend on the device-side inputs: a label outside [0, k) is counted nowhere and indexes nothing
// (its sample is NaN), run boundaries are clamped to [0, n], and an entry of `order` outside [0, n) stages a row of zeros.
#include "pxsom_common.h"

namespace {

constexpr int kBlock = 256;        // threads per workgroup = rows per workgroup
constexpr int kTileDoubles = 4096; // one LDS tile: 32 KB
constexpr int kMaxD = 64;
constexpr int kMaxK = 32;

__global__ __launch_bounds__(kBlock) void silhouette_counts_kernel(const int32_t *__restrict__ labels, int64_t n, int k,
                                                                   int32_t *__restrict__ counts)
{
    __shared__ int hist[kMaxK];
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    if (tid < kMaxK) hist[tid] = 0;
    __syncthreads();
    const int32_t *row = labels + m * n;
    for (int64_t i = tid; i < n; i += kBlock) {
        const int32_t l = row[i];
        if ((uint32_t)l < (uint32_t)k) atomicAdd(&hist[l], 1);
    }
    __syncthreads();
    if (tid < k) counts[m * k + tid] = hist[tid];
}

template <int DMAX>
__global__ __launch_bounds__(kBlock) void silhouette_sums_kernel(const double *__restrict__ x,
                                                                 const int32_t *__restrict__ order,
                                                                 const int32_t *__restrict__ counts, int64_t n, int d,
                                                                 int k, double *__restrict__ sums)
{
    constexpr int kTile = kTileDoubles / DMAX < kBlock ? kTileDoubles / DMAX : kBlock;   // candidates per tile
    constexpr int kRowsPerPass = kBlock / DMAX;                                          // candidates staged per sweep
    __shared__ __attribute__((aligned(16))) double cand[kTile * DMAX];

    const int tid = threadIdx.x;
    const int c = blockIdx.y;
    const int64_t m = blockIdx.z;
    const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
    const bool has_row = i < n;

    // the run of cluster c in order[m]: clamped, whatever the counts hold
    int64_t start = 0;
    for (int u = 0; u < c; ++u) {
        const int32_t v = counts[m * k + u];
        start += v > 0 ? v : 0;
    }
    const int32_t cnt = counts[m * k + c];
    start = start < n ? start : n;
    const int64_t end = start + (cnt > 0 ? cnt : 0) < n ? start + (cnt > 0 ? cnt : 0) : n;

    double xi[DMAX];
#pragma unroll
    for (int t = 0; t < DMAX; ++t) xi[t] = (has_row && t < d) ? x[i * d + t] : 0.0;

    const int32_t *run = order + m * n;
    const int st = tid % DMAX, sr = tid / DMAX;   // this thread stages dimension st of candidates sr, sr + kRowsPerPass, ...
    double acc = 0.0;
    for (int64_t base = start; base < end; base += kTile) {
        const int tile_n = end - base < kTile ? (int)(end - base) : kTile;
        __syncthreads();   // the previous tile has been read
        for (int q = sr; q < tile_n; q += kRowsPerPass) {
            const int64_t j = run[base + q];
            cand[q * DMAX + st] = (st < d && j >= 0 && j < n) ? x[j * d + st] : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < tile_n; ++q) {
            const double *cj = cand + q * DMAX;
            double s = 0.0;
#pragma unroll
            for (int t0 = 0; t0 < DMAX; t0 += 4) {
                if (t0 < d) {
#pragma unroll
                    for (int t = t0; t < t0 + 4; ++t) {
                        const double diff = xi[t] - cj[t];
                        s = __builtin_fma(diff, diff, s);
                    }
                }
            }
            acc += __builtin_sqrt(s);   // correctly rounded binary64
        }
    }
    if (has_row) sums[(m * n + i) * k + c] = acc;
}

__global__ __launch_bounds__(kBlock) void silhouette_samples_kernel(const double *__restrict__ sums,
                                                                    const int32_t *__restrict__ counts,
                                                                    const int32_t *__restrict__ labels, int64_t n, int k,
                                                                    double *__restrict__ samples)
{
    const int64_t m = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t ci = labels[m * n + i];
    double s = __builtin_nan("");
    if ((uint32_t)ci < (uint32_t)k) {
        const double *row = sums + (m * n + i) * k;
        const int32_t *cn = counts + m * k;
        double a = 0.0, b = __builtin_inf();
        int32_t own = 0;
        for (int c = 0; c < k; ++c) {
            const int32_t nc = cn[c];
            const double v = row[c];
            if (c == ci) {
                own = nc;
                a = v / (double)(nc - 1);
            } else if (nc > 0) {
                const double mean = v / (double)nc;
                b = mean < b ? mean : b;
            }
        }
        s = (b - a) / (a > b ? a : b);
        if (own == 1 || s != s) s = 0.0;
    }
    samples[m * n + i] = s;
}

// scores[m] = (sum of samples[m, :]) / n: thread t adds entries t, t + 256, ... in order, then a fixed tree over the threads
__global__ __launch_bounds__(kBlock) void silhouette_mean_kernel(const double *__restrict__ samples, int64_t n,
                                                                 double *__restrict__ scores)
{
    __shared__ double part[kBlock];
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += kBlock) acc += samples[m * n + i];
    part[tid] = acc;
    __syncthreads();
    for (int w = kBlock / 2; w >= 1; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) scores[m] = part[0] / (double)n;
}

template <int DMAX>
void launch_sums(dim3 grid, hipStream_t st, const double *x, const int32_t *order, const int32_t *counts, int64_t n, int d,
                 int k, double *sums)
{
    hipLaunchKernelGGL(silhouette_sums_kernel<DMAX>, grid, dim3(kBlock), 0, st, x, order, counts, n, d, k, sums);
}

}  // namespace

PXSOM_EXPORT int pxsom_silhouette(const double *x_dev, int64_t n, int d, const int32_t *labels_dev,
                                  const int32_t *order_dev, int n_labelings, int k, int32_t *counts_dev, double *sums_dev,
                                  double *samples_dev, double *scores_dev, void *stream)
{
    const char *fn = "pxsom_silhouette";
    if (d < 1 || d > kMaxD)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: d=%d is outside 1 .. %d, the device route's limit", fn, d, kMaxD);
    if (k < 2 || k > kMaxK)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: k=%d is outside 2 .. %d, the device route's limit", fn, k, kMaxK);
    if (n < 2 || n > 0x7fffffff)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld is outside 2 .. 2^31 - 1", fn, (long long)n);
    if (n_labelings < 1 || n_labelings > 65535)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_labelings=%d is outside 1 .. 65535", fn, n_labelings);
    if (!x_dev || !labels_dev || !order_dev || !counts_dev || !sums_dev || !samples_dev || !scores_dev)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);

    hipLaunchKernelGGL(silhouette_counts_kernel, dim3((unsigned)n_labelings), dim3(kBlock), 0, st, labels_dev, n, k,
                       counts_dev);
    PXSOM_LAUNCH_CHECK("silhouette_counts_kernel");
    const dim3 grid(blocks, (unsigned)k, (unsigned)n_labelings);
    if (d <= 8)
        launch_sums<8>(grid, st, x_dev, order_dev, counts_dev, n, d, k, sums_dev);
    else if (d <= 16)
        launch_sums<16>(grid, st, x_dev, order_dev, counts_dev, n, d, k, sums_dev);
    else if (d <= 32)
        launch_sums<32>(grid, st, x_dev, order_dev, counts_dev, n, d, k, sums_dev);
    else
        launch_sums<64>(grid, st, x_dev, order_dev, counts_dev, n, d, k, sums_dev);
    PXSOM_LAUNCH_CHECK("silhouette_sums_kernel");
    hipLaunchKernelGGL(silhouette_samples_kernel, dim3(blocks, (unsigned)n_labelings), dim3(kBlock), 0, st, sums_dev,
                       counts_dev, labels_dev, n, k, samples_dev);
    PXSOM_LAUNCH_CHECK("silhouette_samples_kernel");
    hipLaunchKernelGGL(silhouette_mean_kernel, dim3((unsigned)n_labelings), dim3(kBlock), 0, st, samples_dev, n,
                       scores_dev);
    PXSOM_LAUNCH_CHECK("silhouette_mean_kernel");
    return PXSOM_OK;
}
