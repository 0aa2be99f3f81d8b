// pxsom_edt.hip -- K25: the exact Euclidean distance transform of a binary plane
// (scipy.ndimage.distance_transform_edt(fg): the distance of every foreground pixel to the nearest background pixel).
//
//   pxsom_distance_transform_edt   sq[y][x] = min over background (v, u) of (y - v)^2 + (x - u)^2, exact in int32;
//                                  out[y][x] = sqrt((double)sq), one correctly rounded binary64 square root.
//
// The minimum separates: with g[y][u] the distance from (y, u) to the nearest background pixel of COLUMN u,
// sq[y][x] = min over u of (x - u)^2 + g[y][u]^2.
//
//   pass 1  column distances g (int32, in the workspace).  A workgroup of 64 x 16 threads owns 64 columns of a band of 256
//           rows; thread (c, k) owns the 16 rows [256 band + 16 k, + 16) of column c and keeps them as 16 bits in a
//           register (16 independent byte loads, consecutive lanes on consecutive columns).  It learns the nearest
//           background row above and below its stretch from the other 15 stretches of the band through LDS (first and
//           last background row of each: 2 x 16 x 64 ints = 8 KB) and, where the band has none on that side, from a
//           per-band summary [bands][w] of (first, last) that a first launch of the same body wrote; then two sweeps
//           over the 16 bits give the distances, stored once.  A column without a background pixel gets kEdtNone in
//           every row.
//   pass 2  one thread per pixel minimises along its row, outward from x: d = 1, 2, ... while d^2 < best.  Exact, no
//           envelope stack; the cost is the distance itself (a fibre's half width in this workload, 0 for a background
//           pixel).  The row of g is read through the vector L1: neighbouring pixels read overlapping windows.
//
// kEdtNone is never squared: both passes test for it first.  With h^2 + w^2 <= INT32_MAX (the entry refuses more) every
// square and every sum of two squares is an int32.  A pixel whose row holds only kEdtNone -- then no column, hence no
// pixel of the plane is background -- gets the defined answer of that case: sq = INT32_MAX, out = +inf.
#include <cmath>
#include <cstdint>

#include "pxsom_common.h"
#include "pxsom_plane.h"

namespace {

constexpr int kEdtNone = 0x7fffffff;       // g: the column holds no background pixel; sq: the plane holds none
constexpr int kEdtCols = 64;               // columns of a pass-1 workgroup: one wave wide
constexpr int kEdtParts = 16;              // stretches of a column in a pass-1 workgroup
constexpr int kEdtRows = 16;               // rows of a stretch: one thread's, kept as bits
constexpr int kEdtBand = kEdtParts * kEdtRows;   // 256 rows of a pass-1 workgroup

inline size_t edt_g_bytes(int h, int w) { return pxsom::align_up((size_t)h * (size_t)w * sizeof(int32_t), 8); }
inline int edt_bands(int h) { return (h + kEdtBand - 1) / kEdtBand; }

// kSummary: write the band's (first, last) background row per column and stop; else: write g, reading the summaries
template <bool kSummary>
__global__ __launch_bounds__(kEdtCols * kEdtParts) void edt_columns_kernel(const uint8_t *__restrict__ fg, int H, int W, int64_t ld,
                                                                          int2 *__restrict__ summary, int32_t *__restrict__ g)
{
    __shared__ int s_first[kEdtParts][kEdtCols], s_last[kEdtParts][kEdtCols];
    const int c = threadIdx.x, k = threadIdx.y, band = blockIdx.y;
    const int x = blockIdx.x * kEdtCols + c;
    const int y0 = band * kEdtBand + k * kEdtRows;
    const bool live = x < W;

    unsigned bg = 0;                       // bit r: row y0 + r lies in the plane and is background
    if (live) {
#pragma unroll
        for (int r = 0; r < kEdtRows; r++)
            if (y0 + r < H && fg[(int64_t)(y0 + r) * ld + x] == 0) bg |= 1u << r;
    }
    s_first[k][c] = bg ? y0 + __ffs(bg) - 1 : -1;
    s_last[k][c] = bg ? y0 + 31 - __clz(bg) : -1;
    __syncthreads();
    if (!live) return;
    if (kSummary) {
        if (k == 0) {
            int first = -1, last = -1;
            for (int kk = kEdtParts - 1; kk >= 0; kk--)
                if (s_first[kk][c] >= 0) first = s_first[kk][c];
            for (int kk = 0; kk < kEdtParts; kk++)
                if (s_last[kk][c] >= 0) last = s_last[kk][c];
            summary[(int64_t)band * W + x] = make_int2(first, last);
        }
        return;
    }

    int above = -1, below = -1;            // nearest background row before y0 / from y0 + 16 on; -1: none
    for (int kk = k - 1; kk >= 0 && above < 0; kk--) above = s_last[kk][c];
    for (int b = band - 1; b >= 0 && above < 0; b--) above = summary[(int64_t)b * W + x].y;
    for (int kk = k + 1; kk < kEdtParts && below < 0; kk++) below = s_first[kk][c];
    for (int b = band + 1; b < (int)gridDim.y && below < 0; b++) below = summary[(int64_t)b * W + x].x;

    int up[kEdtRows];
#pragma unroll
    for (int r = 0; r < kEdtRows; r++) {
        if ((bg >> r) & 1u) above = y0 + r;
        up[r] = above >= 0 ? y0 + r - above : kEdtNone;
    }
#pragma unroll
    for (int r = kEdtRows - 1; r >= 0; r--) {
        if ((bg >> r) & 1u) below = y0 + r;
        const int down = below >= 0 ? below - (y0 + r) : kEdtNone;
        if (y0 + r < H) g[(int64_t)(y0 + r) * W + x] = min(up[r], down);
    }
}

__global__ __launch_bounds__(256) void edt_rows_kernel(const int32_t *__restrict__ g, int H, int W, double *__restrict__ out,
                                                       int64_t ldo, int32_t *__restrict__ sq, int64_t ldsq)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int32_t *row = g + (int64_t)y * W;
    const int g0 = row[x];
    int best = g0 == kEdtNone ? kEdtNone : g0 * g0;
    const int reach = max(x, W - 1 - x);                       // the farthest column of the row
    for (int d = 1; d <= reach; d++) {
        const int dd = d * d;                                  // <= (w - 1)^2
        if (dd >= best) break;
        if (x - d >= 0) {
            const int gj = row[x - d];
            if (gj != kEdtNone) best = min(best, dd + gj * gj);   // <= (w - 1)^2 + (h - 1)^2 < INT32_MAX
        }
        if (x + d < W) {
            const int gj = row[x + d];
            if (gj != kEdtNone) best = min(best, dd + gj * gj);
        }
    }
    if (sq) sq[(int64_t)y * ldsq + x] = best;
    if (out) out[(int64_t)y * ldo + x] = best == kEdtNone ? (double)INFINITY : __dsqrt_rn((double)best);
}

int edt_check(const char *fn, int h, int w)
{
    if (h < 1 || w < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a %d x %d plane", fn, h, w);
    if ((int64_t)h * h + (int64_t)w * w > 0x7fffffffLL)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: h^2 + w^2 of a %d x %d plane is beyond int32", fn, h, w);
    return PXSOM_OK;
}

}  // namespace

PXSOM_EXPORT size_t pxsom_distance_transform_edt_workspace_bytes(int h, int w)
{
    if (h < 1 || w < 1 || (int64_t)h * h + (int64_t)w * w > 0x7fffffffLL) return 0;
    return edt_g_bytes(h, w) + (size_t)edt_bands(h) * (size_t)w * sizeof(int2);      // g, then the band summaries
}

PXSOM_EXPORT int pxsom_distance_transform_edt(const uint8_t *fg_dev, int h, int w, int64_t ld, double *out_dev, int64_t ldo,
                                              int32_t *sq_dev, int64_t ldsq, void *workspace_dev, size_t workspace_bytes,
                                              void *stream)
{
    const char *fn = "pxsom_distance_transform_edt";
    if (const int rc = edt_check(fn, h, w)) return rc;
    if (!fg_dev || (!out_dev && !sq_dev)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (ld < w || (out_dev && ldo < w) || (sq_dev && ldsq < w))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row strides %lld / %lld / %lld < w=%d", fn, (long long)ld, (long long)ldo,
                           (long long)ldsq, w);
    if (out_dev && (reinterpret_cast<uintptr_t>(out_dev) & 7)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: out is not 8-byte aligned", fn);
    if ((sq_dev && (reinterpret_cast<uintptr_t>(sq_dev) & 3)) || (reinterpret_cast<uintptr_t>(workspace_dev) & 7))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: sq is not 4-byte or the workspace not 8-byte aligned", fn);
    const size_t need = pxsom_distance_transform_edt_workspace_bytes(h, w);
    if (!workspace_dev || workspace_bytes < need)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_dev ? workspace_bytes : (size_t)0, need);

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int32_t *g = static_cast<int32_t *>(workspace_dev);
    int2 *summary = reinterpret_cast<int2 *>(static_cast<char *>(workspace_dev) + edt_g_bytes(h, w));
    const dim3 grid((unsigned)((w + kEdtCols - 1) / kEdtCols), (unsigned)edt_bands(h)), block(kEdtCols, kEdtParts);
    hipLaunchKernelGGL(edt_columns_kernel<true>, grid, block, 0, st, fg_dev, h, w, ld, summary, g);
    PXSOM_LAUNCH_CHECK("edt_columns_kernel<summary>");
    hipLaunchKernelGGL(edt_columns_kernel<false>, grid, block, 0, st, fg_dev, h, w, ld, summary, g);
    PXSOM_LAUNCH_CHECK("edt_columns_kernel");
    hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, st, g, h, w, out_dev, ldo, sq_dev,
                       ldsq);
    PXSOM_LAUNCH_CHECK("edt_rows_kernel");
    return PXSOM_OK;
}
