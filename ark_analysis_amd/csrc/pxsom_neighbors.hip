// pxsom_neighbors.hip -- per-cell neighbour counts by phenotype, straight from the centroids (K13).
//
// reference: ark/analysis/spatial_analysis_utils.py compute_neighbor_counts over the float32 distance matrix that
// calc_dist_matrix writes.  That matrix is never built here: for a query cell i and a candidate j of the same FOV
//   s = fl(fl(dx * dx) + fl(dy * dy))            (binary64, one IEEE operation per statement, no contraction)
// and j is a neighbour of i when s < s_lim and (self_neighbor or s > s_zero).  The two thresholds are found on the host
// (som_device.neighbor_thresholds) such that this is float32(sqrt(s)) < distlim and float32(sqrt(s)) != 0 exactly.
//
// Shape.  walk_fov_runs of pxsom_fovwalk.h (its memory-safety argument is there); what a run gathers is one count in one
// register.
#include "pxsom_common.h"
#include "pxsom_fovwalk.h"

namespace {

template <bool SELF>
struct CountRun {
    double s_lim, s_zero;

    __device__ __forceinline__ void begin_run() {}
    __device__ __forceinline__ void candidates(double xi, double yi, const double2 *cand, int p, int q, int &c) const
    {
#pragma unroll 8
        for (int k = p; k < q; ++k) c += pair_is_close<SELF>(xi, yi, cand[k], s_lim, s_zero) ? 1 : 0;
    }
    __device__ __forceinline__ int32_t end_run(int count) const { return count; }
};

template <bool SELF>
__global__ __launch_bounds__(kBlock) void neighbor_counts_kernel(const double2 *__restrict__ xy,
                                                                 const int32_t *__restrict__ type,
                                                                 const int64_t *__restrict__ seg, int64_t n_fovs,
                                                                 int64_t n, int n_types, double s_lim, double s_zero,
                                                                 int32_t *__restrict__ counts)
{
    __shared__ double2 cand[kBlock];
    __shared__ int32_t ctype[kBlock];
    __shared__ unsigned long long run_start[kBlock / kWave];
    CountRun<SELF> run{s_lim, s_zero};
    walk_fov_runs<int32_t>(xy, type, seg, n_fovs, n, n_types, 0, counts, cand, ctype, run_start, run);
}

}  // namespace

PXSOM_EXPORT int pxsom_neighbor_counts(const double *xy_dev, const int32_t *type_dev, const int64_t *seg_dev,
                                       int64_t n_fovs, int64_t n, int n_types, double s_lim, double s_zero,
                                       int self_neighbor, int32_t *counts_dev, void *stream)
{
    const char *fn = "pxsom_neighbor_counts";
    unsigned blocks;
    const int rc = check_cell_args(fn, xy_dev, type_dev, seg_dev, n_fovs, n, n_types, counts_dev, &blocks,
                                   [&] { return check_pair_test(fn, self_neighbor, s_lim, s_zero); });
    if (rc != PXSOM_OK || blocks == 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double2 *xy = reinterpret_cast<const double2 *>(xy_dev);
    if (self_neighbor)
        hipLaunchKernelGGL(neighbor_counts_kernel<true>, dim3(blocks), dim3(kBlock), 0, st, xy, type_dev, seg_dev,
                           n_fovs, n, n_types, s_lim, s_zero, counts_dev);
    else
        hipLaunchKernelGGL(neighbor_counts_kernel<false>, dim3(blocks), dim3(kBlock), 0, st, xy, type_dev,
                           seg_dev, n_fovs, n, n_types, s_lim, s_zero, counts_dev);
    PXSOM_LAUNCH_CHECK("neighbor_counts_kernel");
    return PXSOM_OK;
}
