// pxsom_frangi.hip -- K26: one scale of the Frangi ridge filter (skimage 0.19's 2-D frangi as recalled, black_ridges=False),
// folded into the running maximum over the scales.  binary64 throughout, compiled without contraction.
//
//   pxsom_frangi_scale   g = gaussian_filter(x, sigma, mode="reflect") comes from pxsom_gaussian_blur_plane_mode; per pixel
//                        the Hessian s2 * np.gradient(np.gradient(g)), its two eigenvalues ordered by magnitude, the
//                        vesselness exp_neg(-rb / bsq) * (1 - exp_neg(-rg / gsq)) with 0 where the larger eigenvalue is
//                        positive, then out = np.maximum(first ? 0 : out, v) * scale.
//
// np.gradient is (f[i + 1] - f[i - 1]) / 2 inside a line and the one-sided difference f[1] - f[0], f[n - 1] - f[n - 2] at
// its ends.  Applied twice, Hrr and Hcc reach two pixels along their axis and Hrc the four diagonals: 13 points of g, a
// cross of radius 2 and the diagonals, with the form of each difference resolved per index (`ends`).  Every index lies
// inside the plane for h, w >= 2, which the entry checks.  The kernel has the shape of sobel_magnitude_kernel: 64 x 4
// threads, consecutive lanes on consecutive columns, the neighbours re-read through the vector L1 (a workgroup's tile with
// its halo is 68 x 8 doubles); one HBM read of g, one read-modify-write of out per pixel, no LDS.
//
// exp_neg is the statement's own exponential for t <= 0 (tests/frangi_reference.py states the same operations in numpy):
// no maths-library call whose bits could move with a ROCm release.  t < -708 gives 0 (no subnormal is ever produced), NaN
// gives NaN; otherwise k = rint(t * LOG2E), r = (t - k * LN2_HI) - k * LN2_LO (k * LN2_HI is exact: LN2_HI ends in 21
// zero bits, |k| < 2^11), p = the degree-13 Taylor polynomial of exp(r) by Horner (|r| <= ln2 / 2: the remainder is below
// 2^-57 relative), and the result is p * 2^k with 2^k built from its bit pattern.
#include <cmath>
#include <cstdint>

#include "pxsom_common.h"
#include "pxsom_plane.h"

namespace {

#pragma clang fp contract(off)

constexpr double kLog2e = 1.4426950408889634, kLn2Hi = 0.6931471803691238, kLn2Lo = 1.9082149292705877e-10;
constexpr double kExpNegFloor = -708.0;
// 1 / k!, k = 0 .. 13
constexpr double kInvFactorial[14] = {1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333,
                                      0.001388888888888889, 0.0001984126984126984, 2.48015873015873e-05,
                                      2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08,
                                      2.08767569878681e-09, 1.6059043836821613e-10};

__device__ __forceinline__ double exp_neg(double t)
{
    const bool in_range = t >= kExpNegFloor;                   // false for NaN
    const double ts = in_range ? t : 0.0;
    const double k = rint(ts * kLog2e);
    const double r = (ts - k * kLn2Hi) - k * kLn2Lo;
    double p = kInvFactorial[13];
#pragma unroll
    for (int i = 12; i >= 0; i--) p = p * r + kInvFactorial[i];
    const double two_k = __longlong_as_double(((long long)k + 1023) << 52);       // k in -1021 .. 0: a normal number
    const double e = p * two_k;
    return t != t ? t : (in_range ? e : 0.0);
}

// the two positions np.gradient reads for position i of a line of n >= 2, and whether the difference is halved
struct Ends {
    int lo, hi;
    bool inner;
};

__device__ __forceinline__ Ends ends(int i, int n)
{
    const int lo = max(min(i - 1, n - 2), 0), hi = min(max(i + 1, 1), n - 1);
    return Ends{lo, hi, hi - lo == 2};
}

__device__ __forceinline__ double gradient(double lo, double hi, bool inner)
{
    return (hi - lo) * (inner ? 0.5 : 1.0);                   // exact either way: the halving of np.gradient's interior
}

__global__ __launch_bounds__(256) void frangi_scale_kernel(const double *__restrict__ g, int64_t ldg, int H, int W, double s2, double bsq,
                                                           double gsq, int first, double scale, double *__restrict__ out, int64_t ldo)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const Ends ey = ends(y, H), ex = ends(x, W);
    const Ends ey_lo = ends(ey.lo, H), ey_hi = ends(ey.hi, H), ex_lo = ends(ex.lo, W), ex_hi = ends(ex.hi, W);
    const double *row = g + (int64_t)y * ldg, *col = g + x;
    // g0 = np.gradient(g, axis=0) at the two rows Hrr reads, g1 = np.gradient(g, axis=1) at the two columns Hcc reads
    const double g0_up = gradient(col[(int64_t)ey_lo.lo * ldg], col[(int64_t)ey_lo.hi * ldg], ey_lo.inner);
    const double g0_down = gradient(col[(int64_t)ey_hi.lo * ldg], col[(int64_t)ey_hi.hi * ldg], ey_hi.inner);
    const double g1_left = gradient(row[ex_lo.lo], row[ex_lo.hi], ex_lo.inner);
    const double g1_right = gradient(row[ex_hi.lo], row[ex_hi.hi], ex_hi.inner);
    // g0 in this row at the two columns Hrc reads
    const double *up = g + (int64_t)ey.lo * ldg, *down = g + (int64_t)ey.hi * ldg;
    const double g0_left = gradient(up[ex.lo], down[ex.lo], ey.inner);
    const double g0_right = gradient(up[ex.hi], down[ex.hi], ey.inner);
    const double hrr = s2 * gradient(g0_up, g0_down, ey.inner);
    const double hrc = s2 * gradient(g0_left, g0_right, ex.inner);
    const double hcc = s2 * gradient(g1_left, g1_right, ex.inner);
    // the eigenvalues, the larger magnitude first, by the rule K22 uses
    double big, small;
    hessian_eigenvalues(hrr, hrc, hcc, big, small);
    double den = fabs(big);
    if (den == 0.0) den = 1e-10;
    const double q = small / den;
    const double rb = q * q, rg = small * small + big * big;
    double v = exp_neg(-rb / bsq) * (1.0 - exp_neg(-rg / gsq));
    if (big > 0.0) v = 0.0;
    // np.maximum(prev, v): a NaN on either side stays (fmax would drop it)
    double *o = out + (int64_t)y * ldo + x;
    const double prev = first ? 0.0 : *o;
    *o = ((prev >= v || prev != prev) ? prev : v) * scale;
}

#pragma clang fp contract(fast)

bool positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

}  // namespace

PXSOM_EXPORT int pxsom_frangi_scale(const double *g_dev, int64_t ldg, int h, int w, double s2, double bsq, double gsq, int first,
                                    double scale, double *out_dev, int64_t ldo, void *stream)
{
    const char *fn = "pxsom_frangi_scale";
    if (!g_dev || !out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (h < 2 || w < 2) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a %d x %d plane (np.gradient needs 2 per axis)", fn, h, w);
    if (ldg < w || ldo < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row strides %lld / %lld < w=%d", fn, (long long)ldg, (long long)ldo, w);
    if ((reinterpret_cast<uintptr_t>(g_dev) & 7) || (reinterpret_cast<uintptr_t>(out_dev) & 7))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a plane is not 8-byte aligned", fn);
    if (!positive_finite(s2) || !positive_finite(bsq) || !positive_finite(gsq))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: s2=%g, bsq=%g, gsq=%g must be finite and > 0", fn, s2, bsq, gsq);
    {   // out must not share a byte with g: every pixel of g is read by its neighbours
        if (pxsom::spans_overlap(out_dev, pxsom::plane_span_bytes(h, w, ldo, 8), g_dev, pxsom::plane_span_bytes(h, w, ldg, 8)))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: out overlaps g", fn);
    }
    if ((int64_t)h * w > 0x7fffffffLL) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: %d x %d pixels are beyond int32", fn, h, w);
    if ((h + 3) / 4 > 65535) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: h=%d > %d", fn, h, 4 * 65535);
    hipLaunchKernelGGL(frangi_scale_kernel, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), dim3(64, 4), 0,
                       reinterpret_cast<hipStream_t>(stream), g_dev, ldg, h, w, s2, bsq, gsq, first ? 1 : 0, scale, out_dev, ldo);
    PXSOM_LAUNCH_CHECK("frangi_scale_kernel");
    return PXSOM_OK;
}
