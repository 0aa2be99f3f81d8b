// pxsom_celldist.hip -- per cell, the mean float32 distance to its k nearest cells of every phenotype (K14).
//
// reference: ark/analysis/cell_neighborhood_stats.py calculate_mean_distance_to_cell_type over the float32 distance matrix
// that calc_dist_matrix writes: the columns of one phenotype, where(dist > 0), a sort of every row, the mean of its first
// k entries (NaN when fewer than k are left).  That matrix is never built here.  For a query cell i and a candidate j of
// the same FOV and of type t
//   s = fl(fl(dx * dx) + fl(dy * dy))            (binary64, one IEEE operation per statement, no contraction)
// as in pxsom_neighbors.hip; j counts when s > s_zero (float32(sqrt(s)) != 0, som_device.neighbor_thresholds).  sqrt and
// the cast are monotone, so the k smallest distances are those of the k smallest s: the selection runs on s, and only the
// k survivors of a (cell, type) pair see a square root.
//
// Shape.  walk_fov_runs of pxsom_fovwalk.h (its memory-safety argument is there), the run's counter joined by a sorted
// list.  The list is L binary64 registers (L = 8, 16 or 32, the smallest that holds k), ascending, the k live entries at
// the TOP (a[L - k .. L - 1], +inf until filled) over L - k entries pinned at -inf:
// the k-th smallest so far is always a[L - 1], a static register, and one compare against it rejects the common
// candidate.  An insertion is a[j] = max(a[j - 1], min(a[j], s)) for every j (the pinned entries stay -inf by the same
// formula), all indices static: no scratch.  When the run ends the live entries are shifted to a[0 .. k - 1] by a
// log-step shifter under wave-uniform conditions, mapped to float32(sqrt(s)), summed in float32 in the order numpy's
// pairwise row reduction uses, and divided by float32(k).
#include "pxsom_common.h"
#include "pxsom_fovwalk.h"

namespace {

constexpr int kMaxK = 32;     // the largest list instantiated below

// The k smallest s of a run, ascending in a[L - k .. L - 1]; a[0 .. L - k - 1] stay -inf.  Every index is static.
template <int L>
struct NearestList {
    double a[L];

    __device__ __forceinline__ void reset(int k)
    {
#pragma unroll
        for (int j = 0; j < L; ++j) a[j] = j < L - k ? -__builtin_inf() : __builtin_inf();
    }
    __device__ __forceinline__ double kth() const { return a[L - 1]; }
    // s < kth(): s enters, the largest leaves
    __device__ __forceinline__ void insert(double s)
    {
#pragma unroll
        for (int j = L - 1; j >= 1; --j)
            a[j] = __builtin_fmax(a[j - 1], __builtin_fmin(a[j], s));
        a[0] = __builtin_fmin(a[0], s);
    }
    // mean of float32(sqrt(.)) over the k entries, in numpy's order for a float32 row reduction (pairwise sum: a fold for
    // k < 8; else eight strided accumulators over the first k - k % 8 terms, combined as a tree, then the rest in order;
    // k <= 128, so its recursion never splits).  Destroys the list.
    __device__ __forceinline__ float mean(int k)
    {
        const int shift = L - k;
#pragma unroll
        for (int b = 1; b < L; b <<= 1) {
            if (shift & b) {
#pragma unroll
                for (int j = 0; j + b < L; ++j) a[j] = a[j + b];
            }
        }
        float d[L];
#pragma unroll
        for (int j = 0; j < L; ++j) {
            d[j] = 0.0f;
            if (j < k) d[j] = (float)__builtin_sqrt(a[j]);   // correctly rounded binary64, then round to nearest even
        }
        float res;
        if (k < 8) {
            res = 0.0f;
#pragma unroll
            for (int j = 0; j < (L < 8 ? L : 8); ++j)
                if (j < k) res += d[j];
        } else {
            const int n8 = k & ~7;
            float r[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = d[j];
#pragma unroll
            for (int j = 8; j < L; ++j)
                if (j < n8) r[j & 7] += d[j];
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
            for (int j = 8; j < L; ++j)
                if (j >= n8 && j < k) res += d[j];
        }
        return res / (float)k;
    }
};

template <int L>
struct NearestRun {
    NearestList<L> near;
    int k;
    double s_zero;

    __device__ __forceinline__ void begin_run() { near.reset(k); }
    // counts the candidates at float32 distance > 0
    __device__ __forceinline__ void candidates(double xi, double yi, const double2 *cand, int p, int q, int &c)
    {
#pragma unroll 4
        for (int e = p; e < q; ++e) {
            const double s = squared_distance(xi, yi, cand[e]);
            const bool positive = s > s_zero;
            c += positive ? 1 : 0;
            if (positive && s < near.kth()) near.insert(s);
        }
    }
    __device__ __forceinline__ float end_run(int count) { return count >= k ? near.mean(k) : __builtin_nanf(""); }
};

template <int L>
__global__ __launch_bounds__(kBlock) void nearest_type_means_kernel(const double2 *__restrict__ xy,
                                                                    const int32_t *__restrict__ type,
                                                                    const int64_t *__restrict__ seg, int64_t n_fovs,
                                                                    int64_t n, int n_types, int k, double s_zero,
                                                                    float *__restrict__ means)
{
    __shared__ double2 cand[kBlock];
    __shared__ int32_t ctype[kBlock];
    __shared__ unsigned long long run_start[kBlock / kWave];
    NearestRun<L> run;
    run.k = k;
    run.s_zero = s_zero;
    run.begin_run();
    walk_fov_runs<float>(xy, type, seg, n_fovs, n, n_types, __builtin_nanf(""), means, cand, ctype, run_start, run);
}

template <int L>
void launch(unsigned blocks, hipStream_t st, const double2 *xy, const int32_t *type, const int64_t *seg, int64_t n_fovs,
            int64_t n, int n_types, int k, double s_zero, float *means)
{
    hipLaunchKernelGGL(nearest_type_means_kernel<L>, dim3(blocks), dim3(kBlock), 0, st, xy, type, seg, n_fovs, n, n_types,
                       k, s_zero, means);
}

}  // namespace

PXSOM_EXPORT int pxsom_nearest_type_means(const double *xy_dev, const int32_t *type_dev, const int64_t *seg_dev,
                                          int64_t n_fovs, int64_t n, int n_types, int k, double s_zero,
                                          float *means_dev, void *stream)
{
    const char *fn = "pxsom_nearest_type_means";
    unsigned blocks;
    const int rc = check_cell_args(fn, xy_dev, type_dev, seg_dev, n_fovs, n, n_types, means_dev, &blocks, [&] {
        if (k < 1 || k > kMaxK)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: k=%d is outside 1 .. %d, the device route's limit", fn, k, kMaxK);
        if (s_zero != s_zero) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: s_zero is NaN", fn);
        return (int)PXSOM_OK;
    });
    if (rc != PXSOM_OK || blocks == 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double2 *xy = reinterpret_cast<const double2 *>(xy_dev);
    if (k <= 8)
        launch<8>(blocks, st, xy, type_dev, seg_dev, n_fovs, n, n_types, k, s_zero, means_dev);
    else if (k <= 16)
        launch<16>(blocks, st, xy, type_dev, seg_dev, n_fovs, n, n_types, k, s_zero, means_dev);
    else
        launch<32>(blocks, st, xy, type_dev, seg_dev, n_fovs, n, n_types, k, s_zero, means_dev);
    PXSOM_LAUNCH_CHECK("nearest_type_means_kernel");
    return PXSOM_OK;
}
