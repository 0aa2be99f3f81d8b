// pxsom_markers.hip -- K25: from a smoothed distance map to the two inputs of the fibre watershed
// (ark.segmentation.fiber_segmentation.segment_fibers between frangi and watershed), binary64 planes throughout.
//
//   pxsom_plane_greater      out = plane > level                                     uint8 0 / 1
//   pxsom_plane_minmax       {min, max} of the plane; {NaN, NaN} if it holds a NaN    two launches, no atomics
//   pxsom_plane_histogram    np.histogram(plane, nbins, (e[0], e[nbins]))[0] over uploaded edges:
//                            bin i = [e_i, e_i+1), the last bin closed               int64 counts, integer atomics
//   pxsom_sobel_magnitude    sqrt((a^2 + b^2) / 2), a, b = scipy.ndimage.sobel(plane, axis, mode="reflect") / 4
//   pxsom_class_markers      0; 1 where v < t0; 2 where v > t1 (applied last)        int32
//
// Every kernel streams the plane once with consecutive lanes on consecutive columns.  The Sobel kernel reads its 3 x 3
// neighbourhood straight from global memory: the eight re-reads of a pixel come from the vector L1 (a workgroup's 64 x 4
// tile with its halo is 66 x 6 doubles), and the kernel stays at one HBM read and one write per pixel without LDS.
// The arithmetic of the Sobel kernel is compiled without contraction and follows scipy's correlate1d term by term, so
// the result equals the scipy statement bit for bit.
#include <cmath>
#include <cstdint>

#include "pxsom_common.h"
#include "pxsom_plane.h"

namespace {

constexpr int kMaxBins = 1024;
constexpr int kHistThreads = 1024;
constexpr int kMinmaxBlocks = 1024;                        // partial results of the first launch

struct MinMax {
    double lo, hi;
    int nan;
};

__device__ __forceinline__ MinMax minmax_merge(MinMax a, const MinMax &b)
{
    a.lo = b.lo < a.lo ? b.lo : a.lo;
    a.hi = b.hi > a.hi ? b.hi : a.hi;
    a.nan |= b.nan;
    return a;
}

// the 256 threads' values folded into thread 0's
__device__ __forceinline__ MinMax minmax_block(MinMax v)
{
    __shared__ double s_lo[4], s_hi[4];
    __shared__ int s_nan[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        MinMax o;
        o.lo = __shfl_down(v.lo, off);
        o.hi = __shfl_down(v.hi, off);
        o.nan = __shfl_down(v.nan, off);
        v = minmax_merge(v, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[wave] = v.lo;
        s_hi[wave] = v.hi;
        s_nan[wave] = v.nan;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < 4; k++) v = minmax_merge(v, MinMax{s_lo[k], s_hi[k], s_nan[k]});
    return v;
}

__global__ __launch_bounds__(256) void minmax_partial_kernel(const double *__restrict__ plane, unsigned total, unsigned W, int64_t ld,
                                                             double *__restrict__ partial)
{
    MinMax v{INFINITY, -INFINITY, 0};
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned y = e / W, x = e - y * W;
        const double p = plane[(int64_t)y * ld + x];
        v.nan |= p != p;
        v.lo = p < v.lo ? p : v.lo;
        v.hi = p > v.hi ? p : v.hi;
    }
    v = minmax_block(v);
    if (threadIdx.x == 0) {
        partial[3 * blockIdx.x] = v.lo;
        partial[3 * blockIdx.x + 1] = v.hi;
        partial[3 * blockIdx.x + 2] = v.nan ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(256) void minmax_final_kernel(const double *__restrict__ partial, int n, double *__restrict__ out)
{
    MinMax v{INFINITY, -INFINITY, 0};
    for (int b = threadIdx.x; b < n; b += 256)
        v = minmax_merge(v, MinMax{partial[3 * b], partial[3 * b + 1], partial[3 * b + 2] != 0.0});
    v = minmax_block(v);
    if (threadIdx.x == 0) {
        out[0] = v.nan ? (double)NAN : v.lo;
        out[1] = v.nan ? (double)NAN : v.hi;
    }
}

__global__ __launch_bounds__(256) void plane_greater_kernel(const double *__restrict__ plane, unsigned total, unsigned W, int64_t ld,
                                                            double level, uint8_t *__restrict__ out, int64_t ldo)
{
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned y = e / W, x = e - y * W;
        out[(int64_t)y * ldo + x] = plane[(int64_t)y * ld + x] > level;
    }
}

// One workgroup of 1024 threads per CU at most: every workgroup ends with one global atomic per occupied bin, all of them
// on the same nbins words, and with 1024 workgroups of 256 threads that flush was most of the kernel's time.
// The bin of v is first estimated as numpy estimates it, then moved until e[bin] <= v < e[bin + 1] holds (v == e[nbins]
// belongs to the last bin): the count depends on the edges alone, never on how the estimate rounded.
__global__ __launch_bounds__(kHistThreads) void histogram_kernel(const double *__restrict__ plane, unsigned total, unsigned W, int64_t ld,
                                                        const double *__restrict__ edges, int nbins,
                                                        unsigned long long *__restrict__ counts)
{
    __shared__ double s_edge[kMaxBins + 1];
    __shared__ unsigned s_count[kMaxBins];
    for (int i = threadIdx.x; i <= nbins; i += kHistThreads) s_edge[i] = edges[i];
    for (int i = threadIdx.x; i < nbins; i += kHistThreads) s_count[i] = 0;
    __syncthreads();
    const double first = s_edge[0], last = s_edge[nbins], scale = (double)nbins / (last - first);
    const int lane = threadIdx.x & 63;
    for (unsigned e = blockIdx.x * (unsigned)kHistThreads + threadIdx.x; e < total; e += gridDim.x * (unsigned)kHistThreads) {
        const unsigned y = e / W, x = e - y * W;
        const double v = plane[(int64_t)y * ld + x];
        int bin = -1;                                          // outside the range, or NaN: counted nowhere
        if (v >= first && v <= last) {
            const double est = (v - first) * scale;
            bin = est >= (double)(nbins - 1) ? nbins - 1 : (est > 0.0 ? (int)est : 0);   // a NaN estimate: bin 0
            while (bin > 0 && v < s_edge[bin]) bin--;
            while (bin < nbins - 1 && v >= s_edge[bin + 1]) bin++;
        }
        // A distance map is mostly one value (0: the background), and 64 lanes adding to one LDS word take 64 turns:
        // the lanes that share the first counted lane's bin add once, through that lane; the others add for themselves.
        const unsigned long long counted = __ballot(bin >= 0);
        if (counted) {                                         // (uniform over the wave's active lanes)
            const int leader = __ffsll(counted) - 1;
            const int common = __shfl(bin, leader);
            const unsigned long long same = __ballot(bin == common);
            if (lane == leader) atomicAdd(&s_count[common], (unsigned)__popcll(same));   // a workgroup sees < 2^31 pixels
            else if (bin >= 0 && bin != common) atomicAdd(&s_count[bin], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += kHistThreads)
        if (s_count[i]) atomicAdd(&counts[i], (unsigned long long)s_count[i]);
}

__global__ __launch_bounds__(256) void class_markers_kernel(const double *__restrict__ plane, unsigned total, unsigned W, int64_t ld,
                                                            double t0, double t1, int32_t *__restrict__ out, int64_t ldo)
{
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned y = e / W, x = e - y * W;
        const double v = plane[(int64_t)y * ld + x];
        int m = 0;
        if (v < t0) m = 1;
        if (v > t1) m = 2;
        out[(int64_t)y * ldo + x] = m;
    }
}

#pragma clang fp contract(off)

// correlate1d with [-1, 0, 1] at the middle of (lo, mid, hi), and with [1, 2, 1], as scipy's symmetric / antisymmetric
// loops form them: centre term first, then the pair
__device__ __forceinline__ double sobel_diff(double lo, double mid, double hi) { return mid * 0.0 + (lo - hi) * -1.0; }
__device__ __forceinline__ double sobel_smooth(double lo, double mid, double hi) { return mid * 2.0 + (lo + hi) * 1.0; }

__global__ __launch_bounds__(256) void sobel_magnitude_kernel(const double *__restrict__ plane, int H, int W, int64_t ld,
                                                              double *__restrict__ out, int64_t ldo, int32_t *__restrict__ out_i32,
                                                              int64_t ldi)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int xs[3] = {border_idx(x - 1, W, 0), x, border_idx(x + 1, W, 0)};
    const int ys[3] = {border_idx(y - 1, H, 0), y, border_idx(y + 1, H, 0)};
    double v[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) v[i][j] = plane[(int64_t)ys[i] * ld + xs[j]];
    // axis 0: the difference down every column, smoothed along the row
    const double a = sobel_smooth(sobel_diff(v[0][0], v[1][0], v[2][0]), sobel_diff(v[0][1], v[1][1], v[2][1]),
                                  sobel_diff(v[0][2], v[1][2], v[2][2])) / 4.0;
    // axis 1: the difference along every row, smoothed down the column
    const double b = sobel_smooth(sobel_diff(v[0][0], v[0][1], v[0][2]), sobel_diff(v[1][0], v[1][1], v[1][2]),
                                  sobel_diff(v[2][0], v[2][1], v[2][2])) / 4.0;
    const double m = __dsqrt_rn((a * a + b * b) / 2.0);
    if (out) out[(int64_t)y * ldo + x] = m;
    if (out_i32) out_i32[(int64_t)y * ldi + x] = (int)m;      // toward zero
}

#pragma clang fp contract(fast)

// what the five entries check alike: a [h, w] binary64 plane with row stride ld, at most 2^31 - 1 pixels
int plane_check(const char *fn, const double *plane, int h, int w, int64_t ld)
{
    if (!plane) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (h < 1 || w < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a %d x %d plane", fn, h, w);
    if (ld < w) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row stride %lld < w=%d", fn, (long long)ld, w);
    if (reinterpret_cast<uintptr_t>(plane) & 7) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: the plane is not 8-byte aligned", fn);
    return PXSOM_OK;
}

int plane_size_check(const char *fn, int h, int w)
{
    if ((int64_t)h * w > 0x7fffffffLL) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: %d x %d pixels are beyond int32", fn, h, w);
    return PXSOM_OK;
}

}  // namespace

PXSOM_EXPORT int pxsom_plane_greater(const double *plane_dev, int h, int w, int64_t ld, double level, uint8_t *out_dev, int64_t ldo,
                                     void *stream)
{
    const char *fn = "pxsom_plane_greater";
    if (const int rc = plane_check(fn, plane_dev, h, w, ld)) return rc;
    if (!out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (ldo < w) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row stride %lld < w=%d", fn, (long long)ldo, w);
    if (level != level) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: level is NaN", fn);
    if (const int rc = plane_size_check(fn, h, w)) return rc;
    const unsigned total = (unsigned)h * (unsigned)w;
    hipLaunchKernelGGL(plane_greater_kernel, dim3(pxsom::flat_grid(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       plane_dev, total, (unsigned)w, ld, level, out_dev, ldo);
    PXSOM_LAUNCH_CHECK("plane_greater_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT size_t pxsom_plane_minmax_workspace_bytes(void) { return (size_t)kMinmaxBlocks * 3 * sizeof(double); }

PXSOM_EXPORT int pxsom_plane_minmax(const double *plane_dev, int h, int w, int64_t ld, double *minmax_dev, void *workspace_dev,
                                    size_t workspace_bytes, void *stream)
{
    const char *fn = "pxsom_plane_minmax";
    if (const int rc = plane_check(fn, plane_dev, h, w, ld)) return rc;
    if (!minmax_dev || (reinterpret_cast<uintptr_t>(minmax_dev) & 7) || (reinterpret_cast<uintptr_t>(workspace_dev) & 7))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: minmax or the workspace is null or not 8-byte aligned", fn);
    if (!workspace_dev || workspace_bytes < pxsom_plane_minmax_workspace_bytes())
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_dev ? workspace_bytes : (size_t)0,
                           pxsom_plane_minmax_workspace_bytes());
    if (const int rc = plane_size_check(fn, h, w)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned total = (unsigned)h * (unsigned)w;
    const int grid = std::min(kMinmaxBlocks, pxsom::flat_grid(total, 4));
    double *partial = static_cast<double *>(workspace_dev);
    hipLaunchKernelGGL(minmax_partial_kernel, dim3(grid), dim3(256), 0, st, plane_dev, total, (unsigned)w, ld, partial);
    PXSOM_LAUNCH_CHECK("minmax_partial_kernel");
    hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(256), 0, st, partial, grid, minmax_dev);
    PXSOM_LAUNCH_CHECK("minmax_final_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_plane_histogram(const double *plane_dev, int h, int w, int64_t ld, const double *edges_dev, int nbins,
                                       int64_t *counts_dev, void *stream)
{
    const char *fn = "pxsom_plane_histogram";
    if (const int rc = plane_check(fn, plane_dev, h, w, ld)) return rc;
    if (nbins < 1 || nbins > kMaxBins) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: nbins=%d outside [1, %d]", fn, nbins, kMaxBins);
    if (!edges_dev || !counts_dev || (reinterpret_cast<uintptr_t>(edges_dev) & 7) || (reinterpret_cast<uintptr_t>(counts_dev) & 7))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: edges or counts are null or not 8-byte aligned", fn);
    if (const int rc = plane_size_check(fn, h, w)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)nbins * sizeof(int64_t), st));
    const unsigned total = (unsigned)h * (unsigned)w;
    const int grid = (int)std::min<int64_t>(((int64_t)total + kHistThreads - 1) / kHistThreads, pxsom::device_cu_count());
    hipLaunchKernelGGL(histogram_kernel, dim3(grid), dim3(kHistThreads), 0, st, plane_dev, total, (unsigned)w, ld, edges_dev,
                       nbins, reinterpret_cast<unsigned long long *>(counts_dev));
    PXSOM_LAUNCH_CHECK("histogram_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_sobel_magnitude(const double *plane_dev, int h, int w, int64_t ld, double *out_dev, int64_t ldo,
                                       int32_t *out_i32_dev, int64_t ldi, void *stream)
{
    const char *fn = "pxsom_sobel_magnitude";
    if (const int rc = plane_check(fn, plane_dev, h, w, ld)) return rc;
    if (!out_dev && !out_i32_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if ((out_dev && ldo < w) || (out_i32_dev && ldi < w))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row strides %lld / %lld < w=%d", fn, (long long)ldo, (long long)ldi, w);
    if ((reinterpret_cast<uintptr_t>(out_dev) & 7) || (reinterpret_cast<uintptr_t>(out_i32_dev) & 3))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: an output is misaligned", fn);
    // neither output may share a byte with the plane: every pixel is read by its neighbours
    const size_t plane_bytes = pxsom::plane_span_bytes(h, w, ld, 8);
    if (pxsom::spans_overlap(out_dev, pxsom::plane_span_bytes(h, w, ldo, 8), plane_dev, plane_bytes))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: out overlaps the plane", fn);
    if (pxsom::spans_overlap(out_i32_dev, pxsom::plane_span_bytes(h, w, ldi, 4), plane_dev, plane_bytes))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: the int32 output overlaps the plane", fn);
    if (const int rc = plane_size_check(fn, h, w)) return rc;
    if ((h + 3) / 4 > 65535) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: h=%d > %d", fn, h, 4 * 65535);
    hipLaunchKernelGGL(sobel_magnitude_kernel, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), dim3(64, 4), 0,
                       reinterpret_cast<hipStream_t>(stream), plane_dev, h, w, ld, out_dev, ldo, out_i32_dev, ldi);
    PXSOM_LAUNCH_CHECK("sobel_magnitude_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_class_markers(const double *dist_dev, int h, int w, int64_t ld, double t0, double t1, int32_t *out_dev,
                                     int64_t ldo, void *stream)
{
    const char *fn = "pxsom_class_markers";
    if (const int rc = plane_check(fn, dist_dev, h, w, ld)) return rc;
    if (!out_dev || (reinterpret_cast<uintptr_t>(out_dev) & 3)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: out is null or misaligned", fn);
    if (ldo < w) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row stride %lld < w=%d", fn, (long long)ldo, w);
    if (t0 != t0 || t1 != t1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a threshold is NaN", fn);
    if (const int rc = plane_size_check(fn, h, w)) return rc;
    const unsigned total = (unsigned)h * (unsigned)w;
    hipLaunchKernelGGL(class_markers_kernel, dim3(pxsom::flat_grid(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dist_dev,
                       total, (unsigned)w, ld, t0, t1, out_dev, ldo);
    PXSOM_LAUNCH_CHECK("class_markers_kernel");
    return PXSOM_OK;
}
