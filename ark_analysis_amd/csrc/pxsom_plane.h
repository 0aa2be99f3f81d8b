// pxsom_plane.h -- what the image-plane and cell kernels (K10 - K16) share: dispatch over the PXSOM_SEG_* dtype codes,
// the grid of a grid-stride launch, the 4-pixel vector and neighbour-lane shuffles of the K10 / K29 tile, the blur taps and
// borders.  (The key table of K10 / K12 is pxsom_keytable.h.)
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
