// pxsom_clahe.hip -- K27: contrast-limited adaptive histogram equalisation, the front of fibre segmentation (skimage 0.19's
// equalize_adapthist(image, kernel_size, clip_limit, nbins=256) for a 2-D plane and a scalar kernel size, as recalled;
// tests/clahe_reference.py states the same operations in numpy).  Integer arithmetic but for three places, all compiled
// without contraction: the quantisation, the float64 product of the tile maps and the float32 interpolation.
//
//   pxsom_plane_divide    out = plane / divisor                              (the division by the maximum)
//   pxsom_clahe_quantize  gray = uint16(rint((clip(v, lo, hi) - lo) / (hi - lo) * 16383 + 0)); lo == hi: rint(clip(v, 0, 16383))
//   pxsom_clahe_equalize  three launches:
//     tile_maps_kernel    one wave per k x k tile (four tiles a workgroup; a tile of more than 1024 pixels gets a workgroup
//                         to count it): the 256-bin histogram of gray / 65 in LDS, the tail of a border tile read at
//                         2 (S - 1) - i; clip_histogram with four consecutive bins per lane
//                         in registers and every count wave-wide by ballot; an inclusive scan; map = int(min(cumsum *
//                         map_scale, 16383)) as uint16 [nty, ntx, 256]
//     interpolate_kernel  per pixel: p = r + k / 2, b = p / k, j = p % k per axis, the tiles clamp(b - 1) and clamp(b) with
//                         the weights 1 - j / k and j / k; four uint16 gathers, float32(double(map) * (cr * cc)) added in
//                         float32 in the order (0,0), (0,1), (1,0), (1,1), truncated to uint16; the plane's minimum and
//                         maximum reduced per workgroup and folded into two device words by integer atomics,
//                         issued only where they would change the word
//     rescale_kernel      out = (raw - min) / (max - min); min == max: clip(raw, 0, 1)
// No padded plane exists: a tile index and a reflected read replace it.  Integer atomics only: the same input gives the same
// bits on every run.
//
// The redistribution loop of clip_histogram is the statement's, iteration by iteration: `under` = the bins below the
// limit, step = max(1, under / excess), every bin b >= index with (b - index) % step == 0 that is under the limit gains
// one, the excess falls by their number (below zero if it must) and the pass ends at excess <= 0; a pass that moved nothing
// ends the loop.  One shortcut that changes no integer: with no bin under the limit nothing can move in the rest of this
// pass or in the next, so the loop ends there instead of walking the remaining indices.
#include <cmath>
#include <cstdint>

#include "pxsom_common.h"
#include "pxsom_plane.h"
#include "pxsom_wave.h"

namespace {

constexpr int kBins = 256, kBinSize = 65;                  // 1 + 16384 / 256
constexpr double kGreyMax = 16383.0;                       // NR_OF_GRAY - 1
constexpr int kTilesPerBlock = 4;                          // one wave each
constexpr unsigned kWaveTilePixels = 1024;                 // above this a tile gets a whole workgroup: 16 trips of a wave at most
constexpr size_t kWordsBytes = 16;                         // the two minimum / maximum words at the head of the workspace

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void divide_kernel(const double *__restrict__ src, int H, int W, int64_t ld, double divisor,
                                                     double *__restrict__ out, int64_t ldo)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    out[(int64_t)y * ldo + x] = src[(int64_t)y * ld + x] / divisor;
}

__global__ __launch_bounds__(256) void quantize_kernel(const double *__restrict__ src, int H, int W, int64_t ld, double lo, double hi,
                                                       uint16_t *__restrict__ gray, int64_t ldg)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    double v = src[(int64_t)y * ld + x];
    v = v < lo ? lo : v;                                       // np.clip(img, imin, imax)
    v = v > hi ? hi : v;
    double t;
    if (lo != hi) {
        t = (v - lo) / (hi - lo);
        t = t * kGreyMax + 0.0;
    } else {                                                   // a constant plane: np.clip(img, 0, NR - 1)
        t = v < 0.0 ? 0.0 : v;
        t = t > kGreyMax ? kGreyMax : t;
    }
    t = rint(t);                                               // half to even
    const int q = t >= 0.0 ? (t <= kGreyMax ? (int)t : (int)kGreyMax) : 0;     // (a NaN pixel: 0)
    gray[(int64_t)y * ldg + x] = (uint16_t)q;
}

__device__ __forceinline__ int popc(unsigned long long m) { return __popcll(m); }

// kWide: one tile per workgroup, its four waves counting into one histogram and wave 0 going on alone (tiles of more
// than kWaveTilePixels pixels); otherwise one tile per wave.
template <bool kWide>
__global__ __launch_bounds__(256) void tile_maps_kernel(const uint16_t *__restrict__ gray, int H, int W, int64_t ld, int k, int nty,
                                                        int ntx, int clim, double map_scale, uint16_t *__restrict__ maps,
                                                        unsigned *__restrict__ minmax)
{
    __shared__ __attribute__((aligned(16))) unsigned s_hist[kTilesPerBlock][kBins];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = kWide ? 0 : wave;                         // the histogram this wave counts into
    if (blockIdx.x == 0 && threadIdx.x == 0) {                 // the interpolation, the next launch, folds into these
        minmax[0] = 0xffffffffu;
        minmax[1] = 0u;
    }
    const int64_t tile = kWide ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kTilesPerBlock + wave;
    const bool live = tile < (int64_t)nty * ntx;               // uniform over the wave
#pragma unroll
    for (int q = 0; q < 4; q++) s_hist[wave][lane + 64 * q] = 0u;
    __syncthreads();
    const unsigned ke = (unsigned)k * (unsigned)k;             // <= h * w <= 2^31 - 1
    if (live) {
        const int ty = (int)(tile / ntx), tx = (int)(tile - (int64_t)ty * ntx);
        const int y0 = ty * k, x0 = tx * k;
        const unsigned first = kWide ? threadIdx.x : (unsigned)lane, stride = kWide ? 256u : 64u;
        for (unsigned e = first; e < ke; e += stride) {
            const unsigned r = e / (unsigned)k, c = e - r * (unsigned)k;
            int y = y0 + (int)r, x = x0 + (int)c;              // < S + k <= 2 S: one reflection, back inside for k <= S
            y = y >= H ? 2 * (H - 1) - y : y;
            x = x >= W ? 2 * (W - 1) - x : x;
            const int bin = min((int)gray[(int64_t)y * ld + x] / kBinSize, kBins - 1);
            atomicAdd(&s_hist[slot][bin], 1u);
        }
    }
    __syncthreads();
    if (!live || (kWide && wave != 0)) return;

    // ---- clip_histogram: bins 4 lane .. 4 lane + 3 in registers ----
    const uint4 loaded = *reinterpret_cast<const uint4 *>(&s_hist[slot][4 * lane]);
    int hv[4] = {(int)loaded.x, (int)loaded.y, (int)loaded.z, (int)loaded.w};
    const int cl = (unsigned)clim < ke ? clim : (int)ke;       // no count exceeds ke: a larger limit clips nothing either
    long long part = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (hv[q] > cl) {
            part += hv[q] - cl;
            hv[q] = cl;
        }
    long long n_excess = pxsom::wave_sum(part);
    const long long bin_incr = n_excess / kBins;
    const long long upper = (long long)cl - bin_incr;
    part = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (hv[q] < upper) {
            hv[q] += (int)bin_incr;
            part++;
        }
    n_excess -= pxsom::wave_sum(part) * bin_incr;
    part = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)                                // on the updated counts, as the statement has it
        if (hv[q] >= upper && hv[q] < cl) {
            part += hv[q] - cl;
            hv[q] = cl;
        }
    n_excess += pxsom::wave_sum(part);
    bool spent = false;
    while (n_excess > 0 && !spent) {
        const long long prev = n_excess;
        for (int index = 0; index < kBins; index++) {
            const int under = popc(__ballot(hv[0] < cl)) + popc(__ballot(hv[1] < cl)) + popc(__ballot(hv[2] < cl)) +
                              popc(__ballot(hv[3] < cl));
            if (under == 0) {                                  // nothing can move any more (see the file header)
                spent = true;
                break;
            }
            const int step = n_excess >= under ? 1 : under / (int)n_excess;
            int moved = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int d = 4 * lane + q - index;
                const bool hit = d >= 0 && hv[q] < cl && (step == 1 || (unsigned)d % (unsigned)step == 0u);
                hv[q] += hit ? 1 : 0;
                moved += popc(__ballot(hit));
            }
            n_excess -= moved;
            if (n_excess <= 0) break;
        }
        if (prev == n_excess) break;
    }

    // ---- map_histogram: the inclusive scan, one float64 product, the clip, the truncation ----
    const int c0 = hv[0], c1 = c0 + hv[1], c2 = c1 + hv[2], c3 = c2 + hv[3];
    int incl = c3;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const int base = incl - c3;
    const int cum[4] = {base + c0, base + c1, base + c2, base + c3};
    uint16_t m[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        double v = (double)cum[q] * map_scale;
        v = v + 0.0;
        v = v > kGreyMax ? kGreyMax : v;
        m[q] = (uint16_t)(int)v;
    }
    *reinterpret_cast<ushort4 *>(maps + tile * kBins + 4 * lane) = make_ushort4(m[0], m[1], m[2], m[3]);
}

__global__ __launch_bounds__(256) void interpolate_kernel(const uint16_t *__restrict__ gray, int H, int W, int64_t ld, int k, int nty,
                                                          int ntx, const uint16_t *__restrict__ maps, uint16_t *__restrict__ raw,
                                                          int64_t ldr, unsigned *__restrict__ minmax)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    unsigned v_lo = 0xffffffffu, v_hi = 0u;
    if (x < W && y < H) {
        const int bin = min((int)gray[(int64_t)y * ld + x] / kBinSize, kBins - 1);
        const int py = y + k / 2, px = x + k / 2;
        const int by = py / k, bx = px / k;
        const int jy = py - by * k, jx = px - bx * k;
        const int ty0 = min(max(by - 1, 0), nty - 1), ty1 = min(by, nty - 1);
        const int tx0 = min(max(bx - 1, 0), ntx - 1), tx1 = min(bx, ntx - 1);
        const double cr = (double)jy / (double)k, cc = (double)jx / (double)k;
        const double ncr = 1.0 - cr, ncc = 1.0 - cc;
        const uint16_t *at = maps + bin;
        const double m00 = (double)at[((int64_t)ty0 * ntx + tx0) * kBins], m01 = (double)at[((int64_t)ty0 * ntx + tx1) * kBins];
        const double m10 = (double)at[((int64_t)ty1 * ntx + tx0) * kBins], m11 = (double)at[((int64_t)ty1 * ntx + tx1) * kBins];
        float acc = 0.0f;
        acc += (float)(m00 * (ncr * ncc));
        acc += (float)(m01 * (ncr * cc));
        acc += (float)(m10 * (cr * ncc));
        acc += (float)(m11 * (cr * cc));
        const unsigned r = (unsigned)(int)acc;                 // toward zero; 0 .. 16383
        raw[(int64_t)y * ldr + x] = (uint16_t)r;
        v_lo = v_hi = r;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v_lo = min(v_lo, (unsigned)__shfl_xor((int)v_lo, off));
        v_hi = max(v_hi, (unsigned)__shfl_xor((int)v_hi, off));
    }
    // One fold per workgroup, and an atomic only where it would change the word: every wave of the plane adding to the same
    // two addresses was most of this kernel's time.  The minimum only falls and the maximum only rises, so a stale read can
    // only cause a needless atomic, never a missed one.
    __shared__ unsigned s_lo[4], s_hi[4];
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.y] = v_lo;
        s_hi[threadIdx.y] = v_hi;
    }
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const unsigned b_lo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
        const unsigned b_hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
        if (b_lo <= b_hi) {
            if (b_lo < __hip_atomic_load(&minmax[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&minmax[0], b_lo);
            if (b_hi > __hip_atomic_load(&minmax[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&minmax[1], b_hi);
        }
    }
}

__global__ __launch_bounds__(256) void rescale_kernel(const uint16_t *__restrict__ raw, int H, int W, int64_t ldr,
                                                      const unsigned *__restrict__ minmax, double *__restrict__ out, int64_t ldo)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const double lo = (double)minmax[0], hi = (double)minmax[1];
    double v = (double)raw[(int64_t)y * ldr + x];
    if (lo != hi) {
        v = (v - lo) / (hi - lo);
        v = v * (1.0 - 0.0) + 0.0;
    } else {                                                   // a constant plane: np.clip(img, 0, 1)
        v = v > 1.0 ? 1.0 : v;
    }
    out[(int64_t)y * ldo + x] = v;
}

#pragma clang fp contract(fast)

bool is_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

struct Span {
    const void *p;
    size_t bytes;
    const char *name;
};

Span plane_span(const void *p, int h, int w, int64_t ld, size_t elem, const char *name)
{
    return Span{p, pxsom::plane_span_bytes(h, w, ld, elem), name};
}

// the first two of n spans that share a byte, or -1
int first_overlap(const Span *s, int n, int *other)
{
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (pxsom::spans_overlap(s[i].p, s[i].bytes, s[j].p, s[j].bytes)) {
                *other = j;
                return i;
            }
    return -1;
}

// what the three entries check alike: the size of the plane and of the launch grid
int size_check(const char *fn, int h, int w)
{
    if (h < 2 || w < 2) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a %d x %d plane (2 per axis at least)", fn, h, w);
    return PXSOM_OK;
}

int limit_check(const char *fn, int h, int w)
{
    if ((int64_t)h * w > 0x7fffffffLL) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: %d x %d pixels are beyond int32", fn, h, w);
    if ((h + 3) / 4 > 65535) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: h=%d > %d", fn, h, 4 * 65535);
    return PXSOM_OK;
}

dim3 pixel_grid(int h, int w) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)); }

size_t maps_bytes(int h, int w, int k)
{
    const size_t nty = ((size_t)h + k - 1) / k, ntx = ((size_t)w + k - 1) / k;
    return nty * ntx * kBins * sizeof(uint16_t);
}

}  // namespace

PXSOM_EXPORT int pxsom_plane_divide(const double *plane_dev, int h, int w, int64_t ld, double divisor, double *out_dev, int64_t ldo,
                                    void *stream)
{
    const char *fn = "pxsom_plane_divide";
    if (!plane_dev || !out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (const int rc = size_check(fn, h, w)) return rc;
    if (ld < w || ldo < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row strides %lld / %lld < w=%d", fn, (long long)ld, (long long)ldo, w);
    if ((reinterpret_cast<uintptr_t>(plane_dev) & 7) || (reinterpret_cast<uintptr_t>(out_dev) & 7))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a plane is not 8-byte aligned", fn);
    if (!is_finite(divisor) || divisor == 0.0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: divisor=%g must be finite and not 0", fn, divisor);
    if (out_dev != plane_dev || ldo != ld) {   // in place (every pixel read and written by its own thread) or apart
        const Span s[2] = {plane_span(plane_dev, h, w, ld, 8, "plane"), plane_span(out_dev, h, w, ldo, 8, "out")};
        int other;
        if (first_overlap(s, 2, &other) >= 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: out overlaps the plane without being it", fn);
    }
    if (const int rc = limit_check(fn, h, w)) return rc;
    hipLaunchKernelGGL(divide_kernel, pixel_grid(h, w), dim3(64, 4), 0, reinterpret_cast<hipStream_t>(stream), plane_dev, h, w, ld,
                       divisor, out_dev, ldo);
    PXSOM_LAUNCH_CHECK("divide_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_clahe_quantize(const double *src_dev, int h, int w, int64_t ld, double lo, double hi, uint16_t *gray_dev,
                                      int64_t ld_gray, void *stream)
{
    const char *fn = "pxsom_clahe_quantize";
    if (!src_dev || !gray_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (const int rc = size_check(fn, h, w)) return rc;
    if (ld < w || ld_gray < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row strides %lld / %lld < w=%d", fn, (long long)ld, (long long)ld_gray, w);
    if ((reinterpret_cast<uintptr_t>(src_dev) & 7) || (reinterpret_cast<uintptr_t>(gray_dev) & 1))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a plane is misaligned", fn);
    if (!is_finite(lo) || !is_finite(hi) || lo > hi)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: lo=%g, hi=%g must be finite with lo <= hi", fn, lo, hi);
    {
        const Span s[2] = {plane_span(src_dev, h, w, ld, 8, "src"), plane_span(gray_dev, h, w, ld_gray, 2, "gray")};
        int other;
        if (first_overlap(s, 2, &other) >= 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: gray overlaps src", fn);
    }
    if (const int rc = limit_check(fn, h, w)) return rc;
    hipLaunchKernelGGL(quantize_kernel, pixel_grid(h, w), dim3(64, 4), 0, reinterpret_cast<hipStream_t>(stream), src_dev, h, w, ld, lo,
                       hi, gray_dev, ld_gray);
    PXSOM_LAUNCH_CHECK("quantize_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT size_t pxsom_clahe_workspace_bytes(int h, int w, int k)
{
    if (h < 2 || w < 2 || k < 1 || k > std::min(h, w) || (int64_t)h * w > 0x7fffffffLL) return 0;
    return kWordsBytes + pxsom::align_up(maps_bytes(h, w, k), 16) + pxsom::align_up((size_t)h * (size_t)w * sizeof(uint16_t), 16);
}

PXSOM_EXPORT int pxsom_clahe_equalize(const uint16_t *gray_dev, int h, int w, int64_t ld, int k, int clim, double map_scale,
                                      double *out_dev, int64_t ld_out, uint16_t *maps_out_dev, uint16_t *raw_out_dev, int64_t ld_raw,
                                      void *workspace_dev, size_t workspace_bytes, void *stream)
{
    const char *fn = "pxsom_clahe_equalize";
    if (!gray_dev || !out_dev || !workspace_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (const int rc = size_check(fn, h, w)) return rc;
    if (ld < w || ld_out < w || (raw_out_dev && ld_raw < w))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row strides %lld / %lld / %lld < w=%d", fn, (long long)ld, (long long)ld_out,
                           (long long)ld_raw, w);
    if ((reinterpret_cast<uintptr_t>(gray_dev) & 1) || (reinterpret_cast<uintptr_t>(out_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(maps_out_dev) & 7) || (reinterpret_cast<uintptr_t>(raw_out_dev) & 1) ||
        (reinterpret_cast<uintptr_t>(workspace_dev) & 15))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a buffer is misaligned (gray, raw: 2 bytes; out, maps: 8; workspace: 16)", fn);
    if (k < 1 || k > std::min(h, w)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: k=%d outside [1, min(h, w)=%d]", fn, k, std::min(h, w));
    if (clim < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: clim=%d < 1", fn, clim);
    if (!is_finite(map_scale) || !(map_scale > 0.0)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: map_scale=%g must be finite and > 0", fn, map_scale);
    if (const int rc = limit_check(fn, h, w)) return rc;
    const size_t need = pxsom_clahe_workspace_bytes(h, w, k);
    if (workspace_bytes < need) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    {
        Span s[5] = {plane_span(gray_dev, h, w, ld, 2, "gray"), plane_span(out_dev, h, w, ld_out, 8, "out"),
                     Span{workspace_dev, need, "workspace"}};
        int n = 3;
        if (maps_out_dev) s[n++] = Span{maps_out_dev, maps_bytes(h, w, k), "maps_out"};
        if (raw_out_dev) s[n++] = plane_span(raw_out_dev, h, w, ld_raw, 2, "raw_out");
        int other;
        const int one = first_overlap(s, n, &other);
        if (one >= 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: %s overlaps %s", fn, s[other].name, s[one].name);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_dev);
    unsigned *minmax = reinterpret_cast<unsigned *>(ws);
    uint16_t *maps = maps_out_dev ? maps_out_dev : reinterpret_cast<uint16_t *>(ws + kWordsBytes);
    uint16_t *raw = raw_out_dev ? raw_out_dev : reinterpret_cast<uint16_t *>(ws + kWordsBytes + pxsom::align_up(maps_bytes(h, w, k), 16));
    const int64_t ldr = raw_out_dev ? ld_raw : (int64_t)w;
    const int nty = (h + k - 1) / k, ntx = (w + k - 1) / k;
    const int64_t tiles = (int64_t)nty * ntx;
    if ((unsigned)k * (unsigned)k > kWaveTilePixels)
        hipLaunchKernelGGL(tile_maps_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, gray_dev, h, w, ld, k, nty, ntx, clim,
                           map_scale, maps, minmax);
    else
        hipLaunchKernelGGL(tile_maps_kernel<false>, dim3((unsigned)((tiles + kTilesPerBlock - 1) / kTilesPerBlock)),
                           dim3(64 * kTilesPerBlock), 0, st, gray_dev, h, w, ld, k, nty, ntx, clim, map_scale, maps, minmax);
    PXSOM_LAUNCH_CHECK("tile_maps_kernel");
    hipLaunchKernelGGL(interpolate_kernel, pixel_grid(h, w), dim3(64, 4), 0, st, gray_dev, h, w, ld, k, nty, ntx, maps, raw, ldr, minmax);
    PXSOM_LAUNCH_CHECK("interpolate_kernel");
    hipLaunchKernelGGL(rescale_kernel, pixel_grid(h, w), dim3(64, 4), 0, st, raw, h, w, ldr, minmax, out_dev, ld_out);
    PXSOM_LAUNCH_CHECK("rescale_kernel");
    return PXSOM_OK;
}
