// pxsom_overlay.hip -- cell overlays and coloured masks on gfx950 (K29).
//
//   pxsom_overlay_rgb   the body of plot_utils.create_overlay and of segmentation_utils.save_segmentation_labels
//                       (ark/utils/plot_utils.py:567-603, ark/segmentation/segmentation_utils.py:217-219 of the reference):
//                       find_boundaries(seg, connectivity=1, mode="inner"), rescale_intensity per channel to uint8, the white
//                       border of the segmentation and the red border of an alternate segmentation, in one pass
//   pxsom_colorize      the gather of save_colored_masks, (mc_colors[mask] * 255.999).astype(uint8), over a table the host
//                       has converted once
//
// The overlay kernel runs on the tile K10 uses (pxsom_plane.h; pxsom_segmask.hip): a block is 4 waves, a wave owns 256
// columns x 4 rows, a lane 4 consecutive pixels of each row.  load_halo_tile loads the label rows row0 - 1 .. row0 + 4 in one
// sweep (the halo rows are the neighbouring wave's own rows, served by L1 / L2), the left / right neighbour comes from the
// adjacent lane by a shuffle and only lanes 0 and 63 load one extra element per row.  Labels are compared as raw bits of
// their width (1, 2, 4 or 8 bytes): equality and "non-zero" do not depend on the sign, so six label dtypes are four
// instantiations.  A lane's 4 RGB pixels are 12 bytes: three 32-bit words stored together when the row's first byte is 4-byte
// aligned (always when w % 4 == 0), else byte stores, as at a ragged right edge.  The border plane is one 32-bit word per
// lane and row under the same rule.
//
// The arithmetic of the rescale is numpy 2's: binary32 throughout for a float32 plane, binary64 for an integer plane, one
// rounding per operation.  No contraction in this file.
#pragma clang fp contract(off)
#include <cmath>
#include <type_traits>

#include "pxsom_plane.h"

namespace {

// bit (4 i + k): pixel k of the lane's row row0 + i is an inner border pixel -- an in-image 4-neighbour holds another
// label (a neighbour outside the image is the clamped pixel itself: equal) and the pixel's own label is not 0.
// The whole wave calls this (the shuffles need every lane).
template <typename TS>
__device__ __forceinline__ unsigned border_bits(const void *__restrict__ base, int h, int w, int row0, int rows, int c0, int lane)
{
    const TS *seg = static_cast<const TS *>(base);
    TS v[kTileHaloRows][4], left[kTileHaloRows], right[kTileHaloRows];
    load_halo_tile(seg, w, h, w, row0, c0, lane, rows_aligned4(seg, w, sizeof(TS)), v, left, right);
    unsigned bits = 0;
#pragma unroll
    for (int i = 1; i <= kTileRowsPerWave; i++) {
        if (i > rows) break;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const TS c = v[i][k];
            const TS l1 = k == 0 ? left[i] : v[i][k - 1], r1 = k == 3 ? right[i] : v[i][k + 1];
            const bool edge = ((v[i - 1][k] != c) | (v[i + 1][k] != c) | (l1 != c) | (r1 != c)) & (c != (TS)0);
            bits |= (edge ? 1u : 0u) << (4 * (i - 1) + k);
        }
    }
    return bits;
}

__device__ __forceinline__ unsigned border_bits_any(const void *base, int bytes, int h, int w, int row0, int rows, int c0,
                                                    int lane)
{
    switch (bytes) {
    case 1: return border_bits<uint8_t>(base, h, w, row0, rows, c0, lane);
    case 2: return border_bits<uint16_t>(base, h, w, row0, rows, c0, lane);
    case 4: return border_bits<uint32_t>(base, h, w, row0, rows, c0, lane);
    default: return border_bits<uint64_t>(base, h, w, row0, rows, c0, lane);
    }
}

// one output byte: its plane (null: mode 0), the mode, and (lo, hi, hi - lo) in the arithmetic of the plane's dtype
struct Channel {
    const void *plane;
    int mode;
    double lo, hi, span;
    float lo32, hi32, span32;
};

struct OverlayArgs {
    Channel ch[3];          // R, G, B
    const void *seg, *alt;
    int seg_bytes, alt_bytes;
    int h, w, col_blocks;
    uint8_t *rgb, *borders;
};

// rescale_intensity(plane, in_range=(lo, hi), out_range="uint8") of one pixel: clip, then (x - lo) / (hi - lo) * 255.0 + 0.0
// (mode 1) or a second clip to [0, 255] (mode 2, lo == hi), then the truncating cast
template <typename TP>
__device__ __forceinline__ unsigned rescale(TP x, const Channel &c)
{
    if constexpr (std::is_same<TP, float>::value) {
        float y = fminf(fmaxf(x, c.lo32), c.hi32);
        if (c.mode == 1) {
            y = (y - c.lo32) / c.span32;
            y = y * 255.0f + 0.0f;
        } else {
            y = fminf(fmaxf(y, 0.0f), 255.0f);
        }
        return (unsigned)(int)y & 255u;
    } else {
        double y = fmin(fmax((double)x, c.lo), c.hi);
        if (c.mode == 1) {
            y = (y - c.lo) / c.span;
            y = y * 255.0 + 0.0;
        } else {
            y = fmin(fmax(y, 0.0), 255.0);
        }
        return (unsigned)(int)y & 255u;
    }
}

template <typename TP>
__global__ __launch_bounds__(256) void overlay_kernel(OverlayArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bx = (int)(blockIdx.x % (unsigned)a.col_blocks), by = (int)(blockIdx.x / (unsigned)a.col_blocks);
    const int row0 = by * kTileBlockRows + wave * kTileRowsPerWave;
    const int h = a.h, w = a.w;
    if (row0 >= h) return;                                   // whole wave: the shuffles below stay inside live waves
    const int c0 = bx * kTileWaveCols + lane * 4;
    const int rows = min(kTileRowsPerWave, h - row0);

    const unsigned seg_bits = border_bits_any(a.seg, a.seg_bytes, h, w, row0, rows, c0, lane);
    const unsigned alt_bits = a.alt ? border_bits_any(a.alt, a.alt_bytes, h, w, row0, rows, c0, lane) : 0u;
    if (c0 >= w) return;                                     // (after the shuffles)

    if (a.borders) {
#pragma unroll
        for (int i = 0; i < kTileRowsPerWave; i++) {
            if (i >= rows) break;
            uint8_t *row = a.borders + (int64_t)(row0 + i) * w;
            const unsigned b4 = (seg_bits >> (4 * i)) & 15u;
            if (c0 + 3 < w && reinterpret_cast<uintptr_t>(row) % 4 == 0) {
                const unsigned word = ((b4 & 1u) ? 0xffu : 0u) | ((b4 & 2u) ? 0xff00u : 0u) | ((b4 & 4u) ? 0xff0000u : 0u) |
                                      ((b4 & 8u) ? 0xff000000u : 0u);
                *reinterpret_cast<unsigned *>(row + c0) = word;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (c0 + k < w) row[c0 + k] = ((b4 >> k) & 1u) ? 255 : 0;
            }
        }
    }
    if (!a.rgb) return;

    // the planes: every load in flight before the first division
    TP p[3][kTileRowsPerWave][4];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        if (a.ch[j].mode == 0) continue;
        const TP *plane = static_cast<const TP *>(a.ch[j].plane);
        const bool vec = rows_aligned4(plane, w, sizeof(TP));
#pragma unroll
        for (int i = 0; i < kTileRowsPerWave; i++) load4(plane, w, min(row0 + i, h - 1), c0, w, vec, p[j][i]);
    }
#pragma unroll
    for (int i = 0; i < kTileRowsPerWave; i++) {
        if (i >= rows) break;
        unsigned px[4][3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
#pragma unroll
            for (int k = 0; k < 4; k++) px[k][j] = a.ch[j].mode == 0 ? 0u : rescale<TP>(p[j][i][k], a.ch[j]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((seg_bits >> (4 * i + k)) & 1u) px[k][0] = px[k][1] = px[k][2] = 255u;
            if ((alt_bits >> (4 * i + k)) & 1u) {
                px[k][0] = 255u;
                px[k][1] = px[k][2] = 0u;
            }
        }
        uint8_t *row = a.rgb + ((int64_t)(row0 + i) * w + c0) * 3;
        if (c0 + 3 < w && reinterpret_cast<uintptr_t>(row) % 4 == 0) {
            struct Words {
                unsigned a, b, c;
            } words;
            words.a = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
            words.b = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
            words.c = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
            *reinterpret_cast<Words *>(row) = words;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (c0 + k < w) {
#pragma unroll
                    for (int j = 0; j < 3; j++) row[3 * k + j] = (uint8_t)px[k][j];
                }
            }
        }
    }
}

// a thread owns 4 consecutive pixels of the flat mask: one wide load, and the 12 or 16 output bytes as 32-bit words where
// the output is 4-byte aligned; the last, ragged group goes element by element
template <typename TM, int NC>
__global__ __launch_bounds__(256) void colorize_kernel(const TM *__restrict__ mask, int64_t n_px, const uint8_t *__restrict__ table,
                                                       int n_rows, uint8_t *__restrict__ out, int *__restrict__ status,
                                                       bool vec_in, bool vec_out)
{
    bool bad = false;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g * 4 < n_px; g += (int64_t)gridDim.x * 256) {
        const int64_t p0 = g * 4;
        const int cnt = (int)min((int64_t)4, n_px - p0);
        TM m[4];
        if (vec_in && cnt == 4) {
            const typename Vec4<TM>::type x = *reinterpret_cast<const typename Vec4<TM>::type *>(mask + p0);
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = x[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = mask[p0 + min(k, cnt - 1)];
        }
        uint8_t o[4 * NC];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t idx = (int64_t)m[k];
            const bool ok = idx >= 0 && idx < n_rows;
            if (!ok && k < cnt) bad = true;
#pragma unroll
            for (int j = 0; j < NC; j++) o[k * NC + j] = ok ? table[idx * NC + j] : (uint8_t)0;
        }
        uint8_t *dst = out + p0 * NC;
        if (vec_out && cnt == 4) {
#pragma unroll
            for (int q = 0; q < NC; q++)
                reinterpret_cast<unsigned *>(dst)[q] = (unsigned)o[4 * q] | ((unsigned)o[4 * q + 1] << 8) |
                                                      ((unsigned)o[4 * q + 2] << 16) | ((unsigned)o[4 * q + 3] << 24);
        } else {
            for (int e = 0; e < cnt * NC; e++) dst[e] = o[e];
        }
    }
    if (bad) atomicOr(status, PXSOM_COLORIZE_BAD_INDEX);
}

}  // namespace

PXSOM_EXPORT int pxsom_overlay_rgb(const void *r_dev, const void *g_dev, const void *b_dev, int plane_dtype,
                                   const int32_t *modes_host, const double *ranges_host, const void *seg_dev, int seg_dtype,
                                   const void *alt_dev, int alt_dtype, int h, int w, uint8_t *rgb_dev, uint8_t *borders_dev,
                                   void *stream)
{
    const char *fn = "pxsom_overlay_rgb";
    if (h < 1 || w < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad sizes (%d x %d)", fn, h, w);
    if (!seg_dev || !pxsom::is_label_dtype(seg_dtype))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null seg or bad seg_dtype %d", fn, seg_dtype);
    if (alt_dev && !pxsom::is_label_dtype(alt_dtype))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad alt_dtype %d", fn, alt_dtype);
    if (!rgb_dev && !borders_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: no output", fn);
    const void *planes[3] = {r_dev, g_dev, b_dev};
    OverlayArgs a{};
    bool any = false;
    if (rgb_dev) {
        if (!modes_host || !ranges_host) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null modes or ranges", fn);
        for (int j = 0; j < 3; j++) {
            const int mode = modes_host[j];
            const double lo = ranges_host[2 * j], hi = ranges_host[2 * j + 1];
            if (mode < PXSOM_OVERLAY_ZERO || mode > PXSOM_OVERLAY_CLIP)
                return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: channel %d: bad mode %d", fn, j, mode);
            Channel &c = a.ch[j];
            c.mode = mode;
            if (mode == PXSOM_OVERLAY_ZERO) continue;
            if (!planes[j]) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: channel %d: mode %d without a plane", fn, j, mode);
            if (!std::isfinite(lo) || !std::isfinite(hi) || (mode == PXSOM_OVERLAY_RESCALE ? !(lo < hi) : lo != hi))
                return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: channel %d: range (%g, %g) does not fit mode %d", fn, j, lo, hi,
                                   mode);
            any = true;
            c.plane = planes[j];
            c.lo = lo;
            c.hi = hi;
            c.span = hi - lo;
            c.lo32 = (float)lo;               // numpy rounds each Python float to the array's binary32
            c.hi32 = (float)hi;
            c.span32 = (float)(hi - lo);
        }
        if (any && !pxsom::is_image_dtype(plane_dtype, false))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad plane_dtype %d", fn, plane_dtype);
    }
    const size_t px = (size_t)h * (size_t)w;
    const size_t seg_bytes = px * pxsom::plane_dtype_bytes(seg_dtype);
    const size_t alt_bytes = alt_dev ? px * pxsom::plane_dtype_bytes(alt_dtype) : 0;
    // the border test reads neighbours another block may already have written
    using pxsom::spans_overlap;
    if (spans_overlap(rgb_dev, px * 3, seg_dev, seg_bytes) || spans_overlap(rgb_dev, px * 3, alt_dev, alt_bytes) ||
        spans_overlap(borders_dev, px, seg_dev, seg_bytes) || spans_overlap(borders_dev, px, alt_dev, alt_bytes) ||
        spans_overlap(rgb_dev, px * 3, borders_dev, px))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: an output overlaps a label plane or the other output", fn);
    const int col_blocks = (w + kTileWaveCols - 1) / kTileWaveCols;
    const int64_t blocks = (int64_t)col_blocks * ((h + kTileBlockRows - 1) / kTileBlockRows);
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: image too large", fn);

    a.seg = seg_dev;
    a.alt = alt_dev;
    a.seg_bytes = pxsom::plane_dtype_bytes(seg_dtype);
    a.alt_bytes = alt_dev ? pxsom::plane_dtype_bytes(alt_dtype) : 0;
    a.h = h;
    a.w = w;
    a.col_blocks = col_blocks;
    a.rgb = rgb_dev;
    a.borders = borders_dev;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // without a plane to read (borders only, or every channel mode 0) the plane type does not matter
    return pxsom::dispatch_image<false>(any ? plane_dtype : PXSOM_SEG_U8, [&](auto tp) {
        PXSOM_TIMED_LAUNCH((overlay_kernel<decltype(tp)>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        PXSOM_LAUNCH_CHECK("overlay_kernel");
        return (int)PXSOM_OK;
    });
}

namespace {
template <typename TM>
int colorize_typed(const void *mask_dev, int64_t n_px, const uint8_t *table_dev, int n_rows, int n_cols, uint8_t *out_dev,
                   int32_t *status_dev, hipStream_t st)
{
    const TM *mask = static_cast<const TM *>(mask_dev);
    const bool vec_in = reinterpret_cast<uintptr_t>(mask) % (4 * sizeof(TM)) == 0;
    const bool vec_out = reinterpret_cast<uintptr_t>(out_dev) % 4 == 0;
    const int grid = pxsom::flat_grid((n_px + 3) / 4);
    if (n_cols == 3)
        hipLaunchKernelGGL((colorize_kernel<TM, 3>), dim3(grid), dim3(256), 0, st, mask, n_px, table_dev, n_rows, out_dev,
                           status_dev, vec_in, vec_out);
    else
        hipLaunchKernelGGL((colorize_kernel<TM, 4>), dim3(grid), dim3(256), 0, st, mask, n_px, table_dev, n_rows, out_dev,
                           status_dev, vec_in, vec_out);
    PXSOM_LAUNCH_CHECK("colorize_kernel");
    return PXSOM_OK;
}
}  // namespace

PXSOM_EXPORT int pxsom_colorize(const void *mask_dev, int mask_dtype, int h, int w, const uint8_t *table_dev, int n_rows,
                                int n_cols, uint8_t *out_dev, int32_t *status_dev, void *stream)
{
    const char *fn = "pxsom_colorize";
    if (h < 1 || w < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad sizes (%d x %d)", fn, h, w);
    if (mask_dtype != PXSOM_SEG_U8 && mask_dtype != PXSOM_SEG_I16 && mask_dtype != PXSOM_SEG_U16 && mask_dtype != PXSOM_SEG_I32)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad mask_dtype %d", fn, mask_dtype);
    if (n_rows < 1 || (n_cols != 3 && n_cols != 4))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad table (%d x %d; 3 or 4 columns)", fn, n_rows, n_cols);
    if (!mask_dev || !table_dev || !out_dev || !status_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    const int64_t n_px = (int64_t)h * w;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
    switch (mask_dtype) {
    case PXSOM_SEG_U8: return colorize_typed<uint8_t>(mask_dev, n_px, table_dev, n_rows, n_cols, out_dev, status_dev, st);
    case PXSOM_SEG_I16: return colorize_typed<int16_t>(mask_dev, n_px, table_dev, n_rows, n_cols, out_dev, status_dev, st);
    case PXSOM_SEG_U16: return colorize_typed<uint16_t>(mask_dev, n_px, table_dev, n_rows, n_cols, out_dev, status_dev, st);
    default: return colorize_typed<int32_t>(mask_dev, n_px, table_dev, n_rows, n_cols, out_dev, status_dev, st);
    }
}
