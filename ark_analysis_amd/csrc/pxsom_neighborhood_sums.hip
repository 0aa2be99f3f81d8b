// pxsom_neighborhood_sums.hip -- per-cell sums of feature rows over the cells within a radius, straight from the
// centroids (K24): the neighbourhood features of the spatial-LDA preprocessing.
//
// reference: ark/spLDA/processing.py featurize_cell_table, which hands every FOV to spatial_lda's featurize_samples (one
// pandas sub-frame per anchor cell; that library is not a dependency here and its behaviour is taken as DESIGN.md K24
// states it).  For a query cell i and a candidate j of the same FOV (j = i included)
//   s = fl(fl(dx * dx) + fl(dy * dy))            (squared_distance of pxsom_fovwalk.h)
// and j is in the neighbourhood of i when s < s_lim; the threshold is found on the host (som_device.radius_threshold)
// such that this is sqrt(s) < radius, or <= radius, exactly.  counts[i] is the size of the neighbourhood and
// sums[i, t] the sum of feat[j, t] over it in ascending row order: one plain add per member, from +0.0.  A member is
// taken by a select on the accumulator, never by a product, so a NaN or infinite feature reaches the cells within the
// radius of its cell and nobody else.
//
// Shape.  for_each_fov of pxsom_fovwalk.h (one thread one query cell, a workgroup of 256 owns 256 consecutive rows and
// visits every FOV those rows touch), the FOV's cells as candidates in tiles of 256 staged in LDS: the coordinates as
// double2 (4 KB) and kPC = 8 feature columns as a [256][8] block of doubles (16 KB); blockIdx.y names the chunk of 8
// columns, the columns past n_feat are zeros in LDS and are never stored.  Every lane reads the same candidate, so each
// LDS read is a broadcast.  A tile is walked 32 candidates at a time (K20's split of the pair tests from the set
// arithmetic): first the lane's 32 pair tests into one word, the 16-byte reads unrolled so that they are in flight
// together; then one ballot per candidate gives the word of the candidates that some lane of the wave takes, and only
// those, in ascending order, cost the 4 x 16 bytes of their feature row and the adds -- at ten neighbours among hundreds
// of candidates most are outside the radius of all 64 lanes.  The slots past a tile's end hold NaN coordinates, which
// fail every pair test.  The kPC accumulators and the count live in registers; a thread stores its own words once, the
// count from blockIdx.y == 0 only.  No atomics, and the caller need not clear anything: a row that no FOV holds stores
// count 0 and sums +0.0.
//
// Memory safety: the argument of pxsom_fovwalk.h for the cell arrays -- candidates are rows of [beg, end) inside [0, n],
// whatever seg holds, and a feature index is (row, t0 + t) with t0 + t < n_feat; the stores are to the thread's own row
// i < n.  Bad offsets give wrong sums, never an access outside the arrays.
#include "pxsom_common.h"
#include "pxsom_fovwalk.h"

namespace {

constexpr int kPC = 8;                  // feature columns per workgroup
constexpr int kMaxChunks = 65535;       // grid.y
constexpr int kGroup = 32;              // candidates per round of pair tests: a lane's results are one 32-bit word
static_assert(kBlock % kGroup == 0, "a round of pair tests stays inside the staged tile");

__global__ __launch_bounds__(kBlock) void neighborhood_sums_kernel(const double2 *__restrict__ xy,
                                                                   const double *__restrict__ feat,
                                                                   const int64_t *__restrict__ seg, int64_t n_fovs,
                                                                   int64_t n, int n_feat, double s_lim,
                                                                   double *__restrict__ sums,
                                                                   int32_t *__restrict__ counts)
{
    __shared__ double2 cand[kBlock];
    __shared__ __attribute__((aligned(16))) double cfeat[kBlock * kPC];   // [candidate][column of the chunk]

    const int tid = threadIdx.x;
    const int t0 = (int)blockIdx.y * kPC;
    const int pc = n_feat - t0 < kPC ? n_feat - t0 : kPC;   // live columns of this chunk (0 when n_feat == 0)
    const BlockRows rows = load_block_rows(xy, n);
    const double xi = rows.xi, yi = rows.yi;

    double acc[kPC];
#pragma unroll
    for (int t = 0; t < kPC; ++t) acc[t] = 0.0;
    int count = 0;

    for_each_fov(seg, n_fovs, n, rows,
                 [&](int64_t, int64_t beg, int64_t end, bool mine) __attribute__((always_inline)) {
        for (int64_t base = beg; base < end; base += kBlock) {
            const int tile_n = end - base < kBlock ? (int)(end - base) : kBlock;
            __syncthreads();   // the previous tile has been read
            // past the tile's end: NaN coordinates, in nobody's radius
            cand[tid] = tid < tile_n ? xy[base + tid] : make_double2(__builtin_nan(""), __builtin_nan(""));
            // the tile's [tile_n][pc] block of feat: 8 consecutive threads read one row's chunk
#pragma unroll
            for (int r = 0; r < kPC; ++r) {
                const int e = r * kBlock + tid;
                const int cr = e / kPC, t = e % kPC;
                double v = 0.0;
                if (cr < tile_n && t < pc) v = feat[(base + cr) * n_feat + t0 + t];
                cfeat[e] = v;
            }
            __syncthreads();

            for (int k0 = 0; k0 < tile_n; k0 += kGroup) {
                // the lane's pair tests of kGroup candidates, their LDS reads in flight together
                const double2 *cc = cand + k0;
                uint32_t close = 0u;
#pragma unroll
                for (int j = 0; j < kGroup; ++j)
                    close |= (uint32_t)(squared_distance(xi, yi, cc[j]) < s_lim) << j;
                if (!mine) close = 0u;
                count += __popc(close);
                if (pc <= 0) continue;
                // the candidates some lane of the wave takes (the same word in every lane), in ascending order
                uint32_t some = 0u;
#pragma unroll
                for (int j = 0; j < kGroup; ++j)
                    some |= (uint32_t)(__ballot((int)((close >> j) & 1u)) != 0ull) << j;
                some = (uint32_t)__builtin_amdgcn_readfirstlane((int)some);
                while (some) {
                    const int j = __builtin_ctz(some);
                    some &= some - 1u;
                    const bool in = (close >> j) & 1u;
                    const double *f = cfeat + (k0 + j) * kPC;
#pragma unroll
                    for (int t = 0; t < kPC; ++t) {
                        const double with = acc[t] + f[t];
                        acc[t] = in ? with : acc[t];
                    }
                }
            }
        }
    });

    if (!rows.has_row) return;
    if (blockIdx.y == 0) counts[rows.i] = count;
    double *out = sums + rows.i * n_feat + t0;
#pragma unroll
    for (int t = 0; t < kPC; ++t)
        if (t < pc) out[t] = acc[t];
}

}  // namespace

PXSOM_EXPORT int pxsom_neighborhood_sums(const double *xy_dev, const double *feat_dev, const int64_t *seg_dev,
                                         int64_t n_fovs, int64_t n, int n_feat, double s_lim, double *sums_dev,
                                         int32_t *counts_dev, void *stream)
{
    const char *fn = "pxsom_neighborhood_sums";
    if (n < 0 || n_fovs < 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld, n_fovs=%lld", fn, (long long)n, (long long)n_fovs);
    if (n_feat < 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_feat=%d < 0", fn, n_feat);
    const int chunks = n_feat == 0 ? 1 : (n_feat + kPC - 1) / kPC;
    if (chunks > kMaxChunks)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_feat=%d above %d", fn, n_feat, kMaxChunks * kPC);
    if (s_lim != s_lim) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: the threshold is NaN", fn);
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null seg", fn);
    if (n == 0) return PXSOM_OK;
    if (!xy_dev || !counts_dev || (n_feat > 0 && (!feat_dev || !sums_dev)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
    if (reinterpret_cast<uintptr_t>(xy_dev) % sizeof(double2) != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: xy is not 16-byte aligned", fn);
    if (reinterpret_cast<uintptr_t>(feat_dev) % sizeof(double) != 0 || reinterpret_cast<uintptr_t>(sums_dev) % sizeof(double) != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: feat or sums is not 8-byte aligned", fn);
    const int64_t nb = (n + kBlock - 1) / kBlock;
    if (nb > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld too large", fn, (long long)n);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double2 *xy = reinterpret_cast<const double2 *>(xy_dev);
    hipLaunchKernelGGL(neighborhood_sums_kernel, dim3((unsigned)nb, (unsigned)chunks), dim3(kBlock), 0, st, xy, feat_dev,
                       seg_dev, n_fovs, n, n_feat, s_lim, sums_dev, counts_dev);
    PXSOM_LAUNCH_CHECK("neighborhood_sums_kernel");
    return PXSOM_OK;
}
