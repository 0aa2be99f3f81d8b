// pxsom_metric.h -- FlowSOM's other distances (distf 1, 3, 4), one channel term at a time, in binary64.
//
// The caller walks j = 0..c-1 in ascending order and keeps one accumulator per (row, node); every helper is one IEEE
// operation per statement, no contraction, so the accumulated value is the one of FlowSOM's C loop bit for bit:
//   Manhattan  acc = acc + fabs(x - w)
//   Chebyshev  acc = fmax(acc, fabs(x - w))   -- `if (t > d) d = t`: acc is never NaN (it starts at +0 and only takes a t
//              that compared greater), so maxNum's "the non-NaN operand" is exactly that test; equal values are equal bits
//              (t = fabs(...) is never -0)
//   cosine     acc = acc + x * w (the numerator); d1 = sum x*x and d2 = sum w*w are accumulated the same way, each in its
//              own register, which gives the same bits as the one fused loop of the C code
// Padding with x = w = 0 leaves every accumulator unchanged: fabs(0 - 0) = +0, acc + +0 == acc for acc >= 0 and for the
// numerator (a sum that starts at +0 is never -0 under round-to-nearest), fmax(acc, +0) == acc.
#pragma once
#include <hip/hip_runtime.h>

#include "pxsom.h"

namespace pxsom_metric {

template <int M>
__device__ __forceinline__ double term(double acc, double x, double w)
{
#pragma clang fp contract(off)
    static_assert(M == PXSOM_METRIC_MANHATTAN || M == PXSOM_METRIC_CHEBYSHEV || M == PXSOM_METRIC_COSINE, "metric");
    if constexpr (M == PXSOM_METRIC_MANHATTAN) {
        const double t = x - w;
        return acc + fabs(t);
    } else if constexpr (M == PXSOM_METRIC_CHEBYSHEV) {
        const double t = x - w;
        return fmax(acc, fabs(t));
    } else {
        const double p = x * w;
        return acc + p;
    }
}

__device__ __forceinline__ double square_add(double acc, double v)
{
#pragma clang fp contract(off)
    const double p = v * v;
    return acc + p;
}

// distance from the accumulated numerator (cosine) or sum / maximum (the others); sx = sqrt(d1), sw = sqrt(d2)
template <int M>
__device__ __forceinline__ double finish(double acc, double sx, double sw)
{
#pragma clang fp contract(off)
    if constexpr (M == PXSOM_METRIC_COSINE) {
        const double den = sx * sw;
        const double q = -acc / den;
        return q + 1.0;
    } else {
        (void)sx;
        (void)sw;
        return acc;
    }
}

}  // namespace pxsom_metric
