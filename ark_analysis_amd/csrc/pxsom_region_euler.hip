// pxsom_region_euler.hip -- per key, the Euler number of (seg == key) under 8-connectivity: objects minus holes, the
// plane padded by a zero border (skimage regionprops' euler_number of a label; K23, the fibre object table).
//
// Statement (bit quads).  Over every 2 x 2 window of the padded plane -- window (wr, wc), 0 <= wr <= h, 0 <= wc <= w,
// covers the pixels (wr - 1, wc - 1), (wr - 1, wc), (wr, wc - 1), (wr, wc), background outside the image -- and every
// distinct non-zero label l in it, the four bits (window == l) give
//   one bit set +1,  three bits set -1,  two bits set on a diagonal -2,  anything else 0
// and the total over the windows is 4 E(l).
//
//   quads_kernel   one pass over the windows.  A wave owns 64 window columns of kRowsPerWave consecutive window rows,
//                  requests its pixel rows together and keeps the upper row of a window from the trip before; the left
//                  column comes from the neighbouring lane by a shuffle (lane 0 reads it).  A pixel is reduced at once
//                  to an int32 code:
//                  its label, or 0 for background and for a label past int32, which no key names and which therefore
//                  is background for every key.  A window of four equal codes ends there (nearly every window), and so
//                  does every label of a window whose term is 0 -- a straight edge is two adjacent bits -- so only the
//                  corners of an outline reach the key table and one 64-bit integer atomic each.
//   finish_kernel  out[i] = total[i] / 4 in place (the totals are multiples of 4 by the identity above).
// Integer atomics only: the same input gives the same bits.  Memory safety: a pixel is read only at 0 <= r < h,
// 0 <= c < w, and an atomic goes to out[k] only for the index k in [0, n_keys) that find_key returns.
#include "pxsom_common.h"
#include "pxsom_keytable.h"

namespace {

constexpr int kWaveCols = 64;          // window columns per wave: one per lane
constexpr int kWavesPerBlock = 4;
constexpr int kRowsPerWave = 16;       // consecutive window rows per wave
constexpr int kBlockRows = kWavesPerBlock * kRowsPerWave;
constexpr int kMaxSide = 0x7fffffff - 128;   // h, w: window indices up to h + kBlockRows and w + kWaveCols stay inside int

// the pixel's code: its label as int32, 0 for background, outside the image and labels no int32 key can name
template <typename TI>
__device__ __forceinline__ int32_t pixel_code(const TI *__restrict__ seg, int64_t ld, int h, int w, int r, int c)
{
    if (r < 0 || r >= h || c < 0 || c >= w) return 0;
    const TI v = seg[(int64_t)r * ld + c];
    const int64_t wide = (int64_t)v;
    return wide == (int64_t)(int32_t)wide ? (int32_t)wide : 0;
}

// 4 E's term of the bits (tl, tr, bl, br) = (bit 0 .. bit 3) of one label in one window
__device__ __forceinline__ int quad_term(unsigned bits)
{
    const int n = __popc(bits);
    if (n == 1) return 1;
    if (n == 3) return -1;
    if (bits == 0x9u || bits == 0x6u) return -2;      // tl & br, or tr & bl
    return 0;
}

__device__ __forceinline__ void add_term(const KeyTable &t, unsigned long long *__restrict__ total, int32_t label,
                                         unsigned bits)
{
    const int term = quad_term(bits);
    if (term == 0) return;
    const int64_t k = find_key(t, label);
    if (k >= 0) atomicAdd(&total[k], (unsigned long long)(long long)term);     // two's complement: adds `term`
}

template <typename TI>
__global__ __launch_bounds__(256) void quads_kernel(const TI *__restrict__ seg, int h, int w, int64_t ld, KeyTable t,
                                                    int strips_x, unsigned long long *__restrict__ total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wc = (int)(blockIdx.x % strips_x) * kWaveCols + lane;                       // window column
    const int wr0 = ((int)(blockIdx.x / strips_x) * kWavesPerBlock + wave) * kRowsPerWave;    // first window row
    if (wr0 > h) return;                                                                  // whole wave; no barriers below
    // out-of-range lanes (wc > w) keep running with background pixels: the shuffles want the whole wave.  The rows of the
    // chunk are all requested before the first is looked at (independent loads in flight); a window row past h holds
    // background only and ends at the equality test, so the loop needs no early exit.
    int32_t up = pixel_code<TI>(seg, ld, h, w, wr0 - 1, wc);
    int32_t up_left = lane == 0 ? pixel_code<TI>(seg, ld, h, w, wr0 - 1, wc - 1) : 0;
    int32_t dn_row[kRowsPerWave], dn_left[kRowsPerWave];
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) {
        dn_row[j] = pixel_code<TI>(seg, ld, h, w, wr0 + j, wc);
        dn_left[j] = lane == 0 ? pixel_code<TI>(seg, ld, h, w, wr0 + j, wc - 1) : 0;
    }
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) {
        const int32_t dn = dn_row[j];
        int32_t tl = __shfl_up(up, 1, 64), bl = __shfl_up(dn, 1, 64);
        if (lane == 0) { tl = up_left; bl = dn_left[j]; }
        const int32_t tr = up, br = dn;
        if (!(tl == tr && tl == bl && tl == br)) {
            // every distinct non-zero label once, at its first position
            if (tl != 0)
                add_term(t, total, tl, 1u | (tr == tl ? 2u : 0u) | (bl == tl ? 4u : 0u) | (br == tl ? 8u : 0u));
            if (tr != 0 && tr != tl)
                add_term(t, total, tr, 2u | (bl == tr ? 4u : 0u) | (br == tr ? 8u : 0u));
            if (bl != 0 && bl != tl && bl != tr)
                add_term(t, total, bl, 4u | (br == bl ? 8u : 0u));
            if (br != 0 && br != tl && br != tr && br != bl)
                add_term(t, total, br, 8u);
        }
        up = dn;
        up_left = dn_left[j];
    }
}

__global__ __launch_bounds__(256) void finish_kernel(int64_t n, long long *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = out[i] / 4;
}

}  // namespace

PXSOM_EXPORT size_t pxsom_region_euler_workspace_bytes(int64_t n_keys, int32_t key_min, int32_t key_max, int flags)
{
    if (n_keys <= 0 || (flags & PXSOM_REGION_FORCE_SEARCH)) return 0;
    return pxsom::align_up(pxsom::dense_lut_bytes(n_keys, key_min, key_max), 256);
}

PXSOM_EXPORT int pxsom_region_euler(const void *seg_dev, int seg_dtype, int64_t ld, int h, int w,
                                    const int32_t *keys_dev, int64_t n_keys, int32_t key_min, int32_t key_max,
                                    int64_t *euler_dev, void *workspace_dev, size_t workspace_bytes, int flags,
                                    void *stream)
{
    const char *fn = "pxsom_region_euler";
    if (!pxsom::is_label_dtype(seg_dtype)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad seg_dtype %d", fn, seg_dtype);
    if (h < 1 || w < 1 || ld < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad sizes (%d x %d, ld %lld)", fn, h, w, (long long)ld);
    // the kernel forms window rows and columns up to one chunk past h and w in int
    if (h > kMaxSide || w > kMaxSide)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: %d x %d is past the limit of %d pixels per side", fn, h, w, kMaxSide);
    if (flags & ~PXSOM_REGION_FORCE_SEARCH) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: unknown flags %d", fn, flags);
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null image", fn);
    if (n_keys < 0 || (n_keys > 0 && (!keys_dev || key_min > key_max || !euler_dev)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad key table or output", fn);
    const size_t need = pxsom_region_euler_workspace_bytes(n_keys, key_min, key_max, flags);
    if (need && (!workspace_dev || workspace_bytes < need))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    const int strips_x = (int)(((int64_t)w + 1 + kWaveCols - 1) / kWaveCols);
    const int64_t blocks = (((int64_t)h + 1 + kBlockRows - 1) / kBlockRows) * strips_x;
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: image too large", fn);
    if (n_keys == 0) return PXSOM_OK;

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_HIP_TRY(hipMemsetAsync(euler_dev, 0, (size_t)n_keys * sizeof(int64_t), st));
    KeyTable t{keys_dev, nullptr, n_keys, key_min, 0};
    const size_t lut_b = need ? pxsom::dense_lut_bytes(n_keys, key_min, key_max) : 0;
    if (lut_b) {
        const int rc = build_lut(t, reinterpret_cast<int32_t *>(workspace_dev), lut_b, st);
        if (rc != PXSOM_OK) return rc;
    }
    unsigned long long *total = reinterpret_cast<unsigned long long *>(euler_dev);
    pxsom::dispatch_label(seg_dtype, [&](auto ti) {
        typedef decltype(ti) TI;
        PXSOM_TIMED_LAUNCH((quads_kernel<TI>), dim3((unsigned)blocks), dim3(256), 0, st,
                           reinterpret_cast<const TI *>(seg_dev), h, w, ld, t, strips_x, total);
    });
    PXSOM_LAUNCH_CHECK("quads_kernel");
    hipLaunchKernelGGL(finish_kernel, dim3(pxsom::flat_grid(n_keys, 4)), dim3(256), 0, st, n_keys,
                       reinterpret_cast<long long *>(euler_dev));
    PXSOM_LAUNCH_CHECK("finish_kernel");
    return PXSOM_OK;
}
