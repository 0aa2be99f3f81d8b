// pxsom_nearest_idx.hip -- per point, the positions of its k nearest other points of the same FOV (K23: the neighbours
// of the fibre alignment score).
//
// reference: ark/segmentation/fiber_segmentation.py calculate_fiber_alignment, cdist over a FOV's centroids and
// argsort()[1 : 1 + k] of every row.  That matrix is never built.  For a query point i and a candidate j != i of the same
// FOV
//   s = fl(fl(dx * dx) + fl(dy * dy))            (binary64, one IEEE operation per statement, no contraction)
// squared_distance of pxsom_fovwalk.h, as in pxsom_celldist.hip; sqrt is monotone, so the order on s is the order on the
// distance.  The k smallest (s, j) pairs in lexicographic order are the row: ties go to the lower position, and i is left
// out by identity (j == i), not by rank, so a point on top of i is a neighbour like any other.  A candidate whose s is
// not below +inf (overflow, NaN) is never a neighbour.  A FOV with fewer than k + 1 points leaves the tail of the row -1.
//
// Shape.  for_each_fov of pxsom_fovwalk.h (its memory-safety argument is there): one thread one query point, the FOV's
// points as candidates in tiles of 256 staged in LDS, every lane reading the same candidate.  walk_fov_runs is not the
// walk here: it hands a policy neither the candidate's position nor the thread's row, and stores one value per type run.
// The list is K14's (pxsom_celldist.hip NearestList): L binary64 registers (L = 8, 16 or 32, the smallest that holds k),
// ascending, the k live entries at the top over L - k entries pinned at -inf, so that the k-th smallest so far is the
// static register a[L - 1] and one compare rejects the common candidate -- with a second register file p[L] that carries
// each entry's position through the same moves.  Candidates arrive in ascending position, so "ties to the lower
// position" is: reject on s >= a[L - 1], and insert behind every entry with a[j] <= s.  All indices are static.
#include "pxsom_common.h"
#include "pxsom_fovwalk.h"

namespace {

constexpr int kMaxK = 32;     // the largest list instantiated below

// The k smallest (s, position) of the candidates so far, ascending in a[L - k .. L - 1] / p[L - k .. L - 1]; the entries
// below stay (-inf, -1); an unfilled live entry is (+inf, -1).
template <int L>
struct NearestPairs {
    double a[L];
    int32_t p[L];

    __device__ __forceinline__ void reset(int k)
    {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            a[j] = j < L - k ? -__builtin_inf() : __builtin_inf();
            p[j] = -1;
        }
    }
    __device__ __forceinline__ double kth() const { return a[L - 1]; }
    // s < kth(): (s, pos) enters behind every entry with a[j] <= s, the largest leaves
    __device__ __forceinline__ void insert(double s, int32_t pos)
    {
#pragma unroll
        for (int j = L - 1; j >= 1; --j) {
            const bool stays = a[j] <= s;
            const bool lands = a[j - 1] <= s;        // the entry below stays: this is the new pair's place
            const double na = lands ? s : a[j - 1];
            const int32_t np = lands ? pos : p[j - 1];
            a[j] = stays ? a[j] : na;
            p[j] = stays ? p[j] : np;
        }
        if (!(a[0] <= s)) {      // only with L == k: below a pinned entry nothing moves
            a[0] = s;
            p[0] = pos;
        }
    }
};

template <int L>
__global__ __launch_bounds__(kBlock) void nearest_indices_kernel(const double2 *__restrict__ xy,
                                                                 const int64_t *__restrict__ seg, int64_t n_fovs,
                                                                 int64_t n, int k, int32_t *__restrict__ idx)
{
    __shared__ double2 cand[kBlock];
    const int tid = threadIdx.x;
    const BlockRows rows = load_block_rows(xy, n);
    const double xi = rows.xi, yi = rows.yi;
    bool written = false;

    for_each_fov(seg, n_fovs, n, rows, [&](int64_t, int64_t beg, int64_t end, bool mine) __attribute__((always_inline)) {
        NearestPairs<L> near;
        near.reset(k);
        for (int64_t base = beg; base < end; base += kBlock) {
            const int tile_n = end - base < kBlock ? (int)(end - base) : kBlock;
            __syncthreads();   // the previous tile has been read
            if (tid < tile_n) cand[tid] = xy[base + tid];
            __syncthreads();
            if (mine) {
                const int self = rows.i >= base && rows.i < base + tile_n ? (int)(rows.i - base) : -1;
#pragma unroll 4
                for (int e = 0; e < tile_n; ++e) {
                    const double s = squared_distance(xi, yi, cand[e]);
                    if (s < near.kth() && e != self) near.insert(s, (int32_t)(base + e));
                }
            }
        }
        if (mine) {
            int32_t *row = idx + rows.i * k;
#pragma unroll
            for (int j = 0; j < L; ++j)
                if (j >= L - k) row[j - (L - k)] = near.p[j];
            written = true;
        }
    });
    if (rows.has_row && !written) {        // a row no FOV holds
        int32_t *row = idx + rows.i * k;
        for (int j = 0; j < k; ++j) row[j] = -1;
    }
}

template <int L>
void launch(unsigned blocks, hipStream_t st, const double2 *xy, const int64_t *seg, int64_t n_fovs, int64_t n, int k,
            int32_t *idx)
{
    hipLaunchKernelGGL(nearest_indices_kernel<L>, dim3(blocks), dim3(kBlock), 0, st, xy, seg, n_fovs, n, k, idx);
}

}  // namespace

PXSOM_EXPORT int pxsom_nearest_indices(const double *xy_dev, const int64_t *seg_dev, int64_t n_fovs, int64_t n, int k,
                                       int32_t *idx_dev, void *stream)
{
    const char *fn = "pxsom_nearest_indices";
    if (n < 0 || n_fovs < 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld, n_fovs=%lld", fn, (long long)n, (long long)n_fovs);
    if (k < 1 || k > kMaxK)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: k=%d is outside 1 .. %d, the device route's limit", fn, k, kMaxK);
    if (n > 0x7fffffffLL) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld too large", fn, (long long)n);
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null seg", fn);
    if (n == 0) return PXSOM_OK;
    if (!xy_dev || !idx_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
    if (reinterpret_cast<uintptr_t>(xy_dev) % sizeof(double2) != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: xy is not 16-byte aligned", fn);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
    const double2 *xy = reinterpret_cast<const double2 *>(xy_dev);
    if (k <= 8)
        launch<8>(blocks, st, xy, seg_dev, n_fovs, n, k, idx_dev);
    else if (k <= 16)
        launch<16>(blocks, st, xy, seg_dev, n_fovs, n, k, idx_dev);
    else
        launch<32>(blocks, st, xy, seg_dev, n_fovs, n, k, idx_dev);
    PXSOM_LAUNCH_CHECK("nearest_indices_kernel");
    return PXSOM_OK;
}
