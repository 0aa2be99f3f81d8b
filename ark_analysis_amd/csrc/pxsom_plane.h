// pxsom_plane.h -- what the image-plane and cell kernels (K10 - K29) share: dispatch over the PXSOM_SEG_* dtype codes,
// the grid of a grid-stride launch, the overlap test of the C entries, the K10 / K29 tile (its constants, 4-pixel loads
// and stores and the halo loader with its neighbour-lane shuffles), the Hessian eigenvalue rule of K22 / K26, the blur
// taps and borders.  (The key table of K10 / K12 is pxsom_keytable.h, the pair table of K18 / K21 pxsom_pairtable.h.)
//
// The device functions and the kernel-argument structs sit in an unnamed namespace, i.e. they are `static`: every unit
// that includes this header gets its own copy.  That keeps the mangled names of the kernels that take a Taps what they
// were when each unit declared its own struct, so profiler traces stay comparable.
#pragma once
#include <algorithm>

#include "pxsom_common.h"

namespace pxsom {

// bytes of one element of a PXSOM_SEG_* code, 0 for an unknown one
inline int plane_dtype_bytes(int dt)
{
    switch (dt) {
    case PXSOM_SEG_U8: return 1;
    case PXSOM_SEG_I16: case PXSOM_SEG_U16: return 2;
    case PXSOM_SEG_I32: case PXSOM_SEG_U32: case PXSOM_SEG_F32: return 4;
    case PXSOM_SEG_I64: case PXSOM_SEG_F64: return 8;
    default: return 0;
    }
}

// a segmentation dtype: u8, i16, u16, i32, u32, i64
inline bool is_label_dtype(int dt) { return dt >= PXSOM_SEG_U8 && dt <= PXSOM_SEG_I64; }

// an image dtype: u8, i16, u16, i32, f32, and f64 where the entry takes it
inline bool is_image_dtype(int dt, bool with_f64)
{
    return dt == PXSOM_SEG_U8 || dt == PXSOM_SEG_I16 || dt == PXSOM_SEG_U16 || dt == PXSOM_SEG_I32 || dt == PXSOM_SEG_F32 ||
           (with_f64 && dt == PXSOM_SEG_F64);
}

// `return f(T())` with T the element type of a label dtype; the caller has refused every other code (is_label_dtype)
template <typename F>
auto dispatch_label(int dt, F &&f)
{
    switch (dt) {
    case PXSOM_SEG_U8: return f(uint8_t());
    case PXSOM_SEG_I16: return f(int16_t());
    case PXSOM_SEG_U16: return f(uint16_t());
    case PXSOM_SEG_I32: return f(int32_t());
    case PXSOM_SEG_U32: return f(uint32_t());
    default: return f(int64_t());
    }
}

// the same for an image dtype the caller has accepted with is_image_dtype(dt, kWithF64); without kWithF64 nothing is
// instantiated for double
template <bool kWithF64, typename F>
auto dispatch_image(int dt, F &&f)
{
    if constexpr (kWithF64) {
        if (dt == PXSOM_SEG_F64) return f(double());
    }
    switch (dt) {
    case PXSOM_SEG_U8: return f(uint8_t());
    case PXSOM_SEG_I16: return f(int16_t());
    case PXSOM_SEG_U16: return f(uint16_t());
    case PXSOM_SEG_I32: return f(int32_t());
    default: return f(float());
    }
}

// workgroups of 256 for a grid-stride loop over `total` elements: enough to cover them, at most per_cu a CU, at least one
inline int flat_grid(int64_t total, int per_cu = 16)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, (int64_t)device_cu_count() * per_cu));
}

// bytes from the first element of a [h, w] plane with row stride ld (in elements of `elem` bytes) to the end of its last
inline size_t plane_span_bytes(int h, int w, int64_t ld, size_t elem)
{
    return ((size_t)(h - 1) * (size_t)ld + (size_t)w) * elem;
}

// do the a_bytes at a and the b_bytes at b share a byte?  (A null pointer names none.)
inline bool spans_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace pxsom

namespace {

// Workgroup b runs on XCD b % 8 (round robin) and every XCD has an L2 of its own: tiles are dealt to the XCDs in
// contiguous runs, so that neighbouring tiles, which share their halo, meet in the same L2.
__device__ __forceinline__ int64_t xcd_contiguous(int64_t b, int64_t nb)
{
    constexpr int kXcds = 8;
    const int64_t per = (nb + kXcds - 1) / kXcds;
    return (b % kXcds) * per + b / kXcds;     // may be >= nb: the caller skips those
}

// ---- a lane's 4 consecutive pixels and its neighbours' (the tile shape of K10 and K29) ----
template <typename T>
struct Vec4 {
    typedef T type __attribute__((ext_vector_type(4)));
};

template <typename T>
__device__ __forceinline__ T shfl_up1(T v)
{
    if constexpr (sizeof(T) == 8)
        return (T)__shfl_up((long long)v, 1, 64);
    else
        return (T)__shfl_up((int)v, 1, 64);
}

template <typename T>
__device__ __forceinline__ T shfl_down1(T v)
{
    if constexpr (sizeof(T) == 8)
        return (T)__shfl_down((long long)v, 1, 64);
    else
        return (T)__shfl_down((int)v, 1, 64);
}

// A block is kTileWaves waves; a wave owns kTileWaveCols columns x kTileRowsPerWave rows, a lane 4 consecutive pixels of
// each row.  (kTile...: pxsom_region_euler.hip and pxsom_cellquant.hip have tile constants of their own.)
constexpr int kTileWaveCols = 256;       // 64 lanes x 4 pixels
constexpr int kTileRowsPerWave = 4;
constexpr int kTileWaves = 4;
constexpr int kTileBlockRows = kTileRowsPerWave * kTileWaves;
constexpr int kTileHaloRows = kTileRowsPerWave + 2;

// may the rows of a plane at p with row stride ld go through 4-element loads and stores?
__host__ __device__ __forceinline__ bool rows_aligned4(const void *p, int64_t ld, size_t elem)
{
    return reinterpret_cast<uintptr_t>(p) % (4 * elem) == 0 && ld % 4 == 0;
}

// 4 elements of row r from column c0: one wide load when the 4 lie inside the row and the rows are aligned (vec), else
// element loads with the column clamped to w - 1 (the clamp is scipy's reflect at distance 1: the right neighbour of the
// last column is the column itself)
template <typename T>
__device__ __forceinline__ void load4(const T *__restrict__ p, int64_t ld, int r, int c0, int w, bool vec, T (&v)[4])
{
    const T *row = p + (int64_t)r * ld;
    if (vec && c0 + 3 < w) {
        const typename Vec4<T>::type x = *reinterpret_cast<const typename Vec4<T>::type *>(row + c0);
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = x[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = row[min(c0 + k, w - 1)];
    }
}

// the 4 elements back: one packed store under the same rule, else the columns inside the row one by one
template <typename T>
__device__ __forceinline__ void store4(T *__restrict__ p, int64_t ld, int r, int c0, int w, bool vec, const T (&o)[4])
{
    T *row = p + (int64_t)r * ld;
    if (vec && c0 + 3 < w) {
        typename Vec4<T>::type x;
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = o[k];
        *reinterpret_cast<typename Vec4<T>::type *>(row + c0) = x;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c0 + k < w) row[c0 + k] = o[k];
    }
}

// A wave's rows row0 - 1 .. row0 + kTileRowsPerWave, clamped into the image (reflect at distance 1), all loads in flight at
// once: v[i] the lane's 4 pixels of row row0 - 1 + i, left[i] / right[i] the pixel before / after them.  Those come from the
// neighbouring lane by a shuffle; lanes 0 and 63 load the halo column of the wave's tile, one element per row, from L1 / L2.
// The whole wave calls this (the shuffles need every lane).  K29 calls it; K10 keeps the same lines written out over load4
// (pxsom_segmask.hip says why).
template <typename T>
__device__ __forceinline__ void load_halo_tile(const T *base, int64_t ld, int h, int w, int row0, int c0, int lane,
                                               bool vec, T (&v)[kTileHaloRows][4], T (&left)[kTileHaloRows],
                                               T (&right)[kTileHaloRows])
{
#pragma unroll
    for (int i = 0; i < kTileHaloRows; i++) load4(base, ld, min(max(row0 - 1 + i, 0), h - 1), c0, w, vec, v[i]);
#pragma unroll
    for (int i = 0; i < kTileHaloRows; i++) {
        left[i] = shfl_up1(v[i][3]);     // lane - 1's last pixel
        right[i] = shfl_down1(v[i][0]);  // lane + 1's first pixel
    }
    if (lane == 0 || lane == 63) {
        const int cc = lane == 0 ? max(c0 - 1, 0) : min(c0 + 4, w - 1);
#pragma unroll
        for (int i = 0; i < kTileHaloRows; i++) {
            const T x = base[(int64_t)min(max(row0 - 1 + i, 0), h - 1) * ld + cc];
            if (lane == 0) left[i] = x;
            else right[i] = x;
        }
    }
}

// ---- the eigenvalues of a symmetric 2 x 2 Hessian (K22, K26) ----
// Closed form, binary64, one rounding per operation whatever the including file's contraction state.  big: the one of the
// larger magnitude, and e_lo on a tie; with a NaN the comparison is false and big is e_hi.  A parity rule (no fmax / fmin).
__device__ __forceinline__ void hessian_eigenvalues(double hrr, double hrc, double hcc, double &big, double &small)
{
#pragma clang fp contract(off)
    const double d = hrr - hcc;
    const double r = __dsqrt_rn(d * d + 4.0 * (hrc * hrc));
    const double t = hrr + hcc;
    const double e_hi = (t + r) / 2.0, e_lo = (t - r) / 2.0;
    const bool lo_big = fabs(e_lo) >= fabs(e_hi);
    big = lo_big ? e_lo : e_hi;
    small = lo_big ? e_hi : e_lo;
}

// ---- blur taps and borders ----
constexpr int kMaxRadius = 64;

struct Taps {
    double w[kMaxRadius + 1];  // w[0] centre, w[d] weight at distance d (symmetric kernel)
    int radius;
};

// from the 2 * radius + 1 weights of a symmetric kernel (w[r + d] == w[r - d]); radius <= kMaxRadius
inline Taps fill_taps(const double *weights_host, int radius)
{
    Taps taps;
    taps.radius = radius;
    for (int d = 0; d <= radius; d++) taps.w[d] = weights_host[radius + d];
    for (int d = radius + 1; d <= kMaxRadius; d++) taps.w[d] = 0.0;
    return taps;
}

// Position i of a line of `len` extended as scipy extends it, for any i (the image may be shorter than the kernel radius:
// NI_ExtendLine keeps reflecting, period 2 * len).
//   NI_EXTEND_REFLECT (d c b a | a b c d | d c b a);  nearest: NI_EXTEND_NEAREST (a a a | a b c d | d d d)
__device__ __forceinline__ int border_idx(int i, int len, int nearest)
{
    if (nearest) return i < 0 ? 0 : (i >= len ? len - 1 : i);
    if (len == 1) return 0;
    const int sz2 = 2 * len;
    int m = i % sz2;
    if (m < 0) m += sz2;
    return m < len ? m : sz2 - 1 - m;
}

}  // namespace
