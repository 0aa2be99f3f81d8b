// pxsom_neighbors.hip -- per-cell neighbour counts by phenotype, straight from the centroids (K13).
//
// reference: ark/analysis/spatial_analysis_utils.py compute_neighbor_counts over the float32 distance matrix that
// calc_dist_matrix writes.  That matrix is never built here: for a query cell i and a candidate j of the same FOV
//   s = fl(fl(dx * dx) + fl(dy * dy))            (binary64, one IEEE operation per statement, no contraction)
// and j is a neighbour of i when s < s_lim and (self_neighbor or s > s_zero).  The two thresholds are found on the host
// (som_device.neighbor_thresholds) such that this is float32(sqrt(s)) < distlim and float32(sqrt(s)) != 0 exactly.
//
// Shape.  One thread owns one query cell (coordinates in registers); a workgroup of 256 owns 256 consecutive rows and
// walks, for every FOV those rows touch, all the FOV's cells as candidates in tiles of 256 staged in LDS.  Every lane
// reads the same candidate (one 16-byte broadcast read, no bank conflict).  The caller hands the cells of a FOV sorted by
// type, so the candidates of one type are one run: the count of the run lives in one register and is stored when the run
// ends.  Where runs begin is known per tile from one ballot per wave at staging time (a 64-bit mask per 64 candidates),
// so the loop over a run carries no type test.  The run boundaries are the same for every lane: no atomics, no LDS
// counters, any number of types.  Each thread writes every column of its own row exactly once -- zeros between the runs
// it met, after the last one, and for a row no FOV holds -- so the caller need not clear the output.
//
// Memory safety does not depend on the device-side inputs: FOV offsets are clamped to [0, n], and a type outside
// [0, n_types) or out of order is never stored (its row is then wrong, not its neighbours' memory).
#include "pxsom_common.h"

namespace {

constexpr int kBlock = 256;   // threads per workgroup = query rows per workgroup = candidates per tile
constexpr int kWave = 64;

struct RowWriter {
    int32_t *row;   // counts + i * n_types; touched only when `live`
    int n_types;
    int next;       // columns [0, next) are written
    bool live;

    // zeros for [next, t), then `c` at column t; t is the same for every lane
    __device__ __forceinline__ void put(int t, int c)
    {
        if (!live || t < next || t >= n_types) return;
        for (int u = next; u < t; ++u) row[u] = 0;
        row[t] = c;
        next = t + 1;
    }
    __device__ __forceinline__ void finish()
    {
        if (!live) return;
        for (int u = next; u < n_types; ++u) row[u] = 0;
        next = n_types;
    }
};

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool SELF>
__device__ __forceinline__ int is_neighbor(double xi, double yi, double2 cj, double s_lim, double s_zero)
{
#pragma clang fp contract(off)
    const double dx = xi - cj.x;
    const double dy = yi - cj.y;
    const double px = dx * dx;
    const double py = dy * dy;
    const double s = px + py;
    if constexpr (SELF) {
        (void)s_zero;
        return s < s_lim ? 1 : 0;
    } else {
        return (s < s_lim && s > s_zero) ? 1 : 0;
    }
}

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

    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kBlock;
    const int64_t r1 = r0 + kBlock < n ? r0 + kBlock : n;
    const int64_t i = r0 + tid;
    const bool has_row = i < n;
    double xi = 0.0, yi = 0.0;
    if (has_row) {
        const double2 q = xy[i];
        xi = q.x;
        yi = q.y;
    }
    RowWriter out{has_row ? counts + i * n_types : nullptr, n_types, 0, has_row};

    // the first FOV that ends beyond r0
    int64_t lo = 0, hi = n_fovs;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (seg[mid + 1] > r0) hi = mid; else lo = mid + 1;
    }

    for (int64_t f = lo; f < n_fovs; ++f) {
        const int64_t beg = clamp_i64(seg[f], 0, n);
        const int64_t end = clamp_i64(seg[f + 1], beg, n);
        if (beg >= r1) break;
        if (end <= r0 || end == beg) continue;
        const bool mine = has_row && i >= beg && i < end;
        int cur = -1, c = 0;   // the open run's type and count
        for (int64_t base = beg; base < end; base += kBlock) {
            const int tile_n = end - base < kBlock ? (int)(end - base) : kBlock;
            __syncthreads();   // the previous tile has been read
            bool starts = false;
            if (tid < tile_n) {
                const int64_t j = base + tid;
                const int32_t t = type[j];
                cand[tid] = xy[j];
                ctype[tid] = t;
                starts = j == beg || type[j - 1] != t;
            }
            const unsigned long long m = __ballot(starts);
            if ((tid & (kWave - 1)) == 0) run_start[tid / kWave] = m;
            __syncthreads();
            for (int w0 = 0; w0 < tile_n; w0 += kWave) {
                const unsigned long long full = run_start[w0 / kWave];
                const unsigned long long mask =
                    ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(full >> 32)) << 32) |
                    (unsigned)__builtin_amdgcn_readfirstlane((int)full);
                const int cnt = tile_n - w0 < kWave ? tile_n - w0 : kWave;
                int p = 0;
                while (p < cnt) {
                    if ((mask >> p) & 1ull) {
                        if (mine && cur >= 0) out.put(cur, c);
                        cur = __builtin_amdgcn_readfirstlane(ctype[w0 + p]);
                        c = 0;
                    }
                    const unsigned long long rest = p + 1 < kWave ? mask >> (p + 1) : 0ull;
                    int q = rest ? p + 1 + __builtin_ctzll(rest) : kWave;
                    q = q < cnt ? q : cnt;
#pragma unroll 8
                    for (int k = p; k < q; ++k) c += is_neighbor<SELF>(xi, yi, cand[w0 + k], s_lim, s_zero);
                    p = q;
                }
            }
        }
        if (mine && cur >= 0) out.put(cur, c);
    }
    out.finish();
}

}  // namespace

PXSOM_EXPORT int pxsom_neighbor_counts(const double *xy_dev, const int32_t *type_dev, const int64_t *seg_dev,
                                       int64_t n_fovs, int64_t n, int n_types, double s_lim, double s_zero,
                                       int self_neighbor, int32_t *counts_dev, void *stream)
{
    const char *fn = "pxsom_neighbor_counts";
    if (n < 0 || n_fovs < 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld, n_fovs=%lld", fn, (long long)n, (long long)n_fovs);
    if (n_types < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_types=%d < 1", fn, n_types);
    if (self_neighbor != 0 && self_neighbor != 1)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: self_neighbor=%d is not 0 or 1", fn, self_neighbor);
    if (s_lim != s_lim || s_zero != s_zero) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a threshold is NaN", fn);
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null seg", fn);
    if (n == 0) return PXSOM_OK;
    if (!xy_dev || !type_dev || !counts_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
    if (reinterpret_cast<uintptr_t>(xy_dev) % sizeof(double2) != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: xy is not 16-byte aligned", fn);
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld too large", fn, (long long)n);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double2 *xy = reinterpret_cast<const double2 *>(xy_dev);
    if (self_neighbor)
        hipLaunchKernelGGL(neighbor_counts_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, xy, type_dev, seg_dev,
                           n_fovs, n, n_types, s_lim, s_zero, counts_dev);
    else
        hipLaunchKernelGGL(neighbor_counts_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, xy, type_dev,
                           seg_dev, n_fovs, n, n_types, s_lim, s_zero, counts_dev);
    PXSOM_LAUNCH_CHECK("neighbor_counts_kernel");
    return PXSOM_OK;
}
