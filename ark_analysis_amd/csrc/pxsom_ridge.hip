// pxsom_ridge.hip -- K22: where skimage 0.19's Meijering ridge filter is positive, on a binary plane (the "projection"
// object masks of ez_object_segmentation._create_object_mask).
//
//   pxsom_ridge_sign   out = OR over the scales of (aux < 0), with per scale
//                        g   = gaussian_filter(x, sigma, mode="reflect")            axis 0, then axis 1
//                        H   = s2 * np.gradient(np.gradient(g))                     Hrr, Hrc, Hcc; edge_order 1
//                        e   = closed-form eigenvalues of [[Hrr, Hrc], [Hrc, Hcc]]
//                        aux = big + alpha * small                                  big: the larger |e|, a tie takes e_lo
//
// All binary64, one rounding per operation in the statement's order (fp contraction off), so the mask equals the numpy
// statement of tests/projection_mask_reference.py bit for bit.
//
// ONE launch, no workspace, no binary64 plane in HBM.  A workgroup of 1024 threads owns a 64 x 64 output tile; in LDS:
//   s8  [100][100] uint8    the tile with a halo of R_max + 2 (<= 18) on each side, 0 / 1, reflect borders resolved here
//   a   [68][100]  double   the axis-0 pass of one scale: rows -2 .. 65 of the tile, columns -2 - r .. 65 + r
//   g   [68][68]   double   the axis-1 pass: the blurred tile with the halo of 2 that the second difference needs
// 10 000 + 54 400 + 36 992 B = 101 392 B of LDS: one workgroup (16 waves) per CU.  Consecutive threads take consecutive
// columns in every stage; the row pitch of `a` is 68 + 32 doubles so that a wave which straddles two rows of the 68-wide
// axis-1 pass still reads 64 consecutive banks (pitch - 68 = 0 mod 32 doubles).
#include <cmath>
#include <cstdint>

#include "pxsom_common.h"
#include "pxsom_plane.h"

namespace {

constexpr int kRidgeTile = 64;
constexpr int kRidgeMaxRadius = 16;                                  // sigma = 4: the reference's largest scale
constexpr int kRidgeMaxScales = 8;
constexpr int kRidgeThreads = 1024;
constexpr int kRidgeG = kRidgeTile + 4;                              // 68: the tile and the stencil's halo of 2
constexpr int kRidgeS = kRidgeTile + 2 * (kRidgeMaxRadius + 2);      // 100: edge of the staged uint8 tile
constexpr int kRidgeAPitch = kRidgeG + 32;                           // 100 doubles
constexpr int kRidgeOrigin = kRidgeMaxRadius + 2;                    // staged index of tile row / column 0
constexpr size_t kRidgeLds = (size_t)(kRidgeG * kRidgeAPitch + kRidgeG * kRidgeG) * sizeof(double) + (size_t)kRidgeS * kRidgeS;

struct RidgeScales {                                                 // 1.2 KB, by value
    double w[kRidgeMaxScales][kRidgeMaxRadius + 1];                  // w[s][0] centre, w[s][d] weight at distance d
    double s2[kRidgeMaxScales];
    double alpha;
    int radius[kRidgeMaxScales];
    int n, rmax;
};

#pragma clang fp contract(off)

// Both blur passes of one scale, the radius R a template argument: the taps d = R .. 1 of an output are straight-line
// code in correlate1d's order, every LDS offset an immediate, the weights fetched once per scale, and the width of the
// axis-0 pass a constant divisor.  `w`: the scale's weights in the kernel's argument block (uniform reads).
template <int R>
__device__ __forceinline__ void ridge_blur(const uint8_t *s8, double *a, double *g, const double *w, int tid)
{
    double wr[R + 1];
#pragma unroll
    for (int d = 0; d <= R; d++) wr[d] = w[d];
    // axis 0: a[i][j] <-> tile row i - 2, tile column j - 2 - R
    constexpr int aw = kRidgeG + 2 * R;
    for (int e = tid; e < kRidgeG * aw; e += kRidgeThreads) {
        const int i = e / aw, j = e - i * aw;
        const uint8_t *c = s8 + (i + kRidgeOrigin - 2) * kRidgeS + (j + kRidgeOrigin - 2 - R);
        double tmp = (double)c[0] * wr[0];
#pragma unroll
        for (int d = R; d >= 1; d--) tmp += (double)((int)c[-d * kRidgeS] + (int)c[d * kRidgeS]) * wr[d];   // 0 / 1 / 2: exact
        a[i * kRidgeAPitch + j] = tmp;
    }
    __syncthreads();
    // axis 1: g[i][j] <-> tile row i - 2, tile column j - 2
    for (int e = tid; e < kRidgeG * kRidgeG; e += kRidgeThreads) {
        const int i = e / kRidgeG, j = e - i * kRidgeG;
        const double *c = a + i * kRidgeAPitch + j + R;
        double tmp = c[0] * wr[0];
#pragma unroll
        for (int d = R; d >= 1; d--) tmp += (c[-d] + c[d]) * wr[d];
        g[e] = tmp;
    }
    __syncthreads();
}

// np.gradient(f)[i] along one axis from the three values around position i of a line of `len` (edge_order 1)
__device__ __forceinline__ double grad1(double lo, double mid, double hi, int i, int len)
{
    if (i == 0) return hi - mid;
    if (i == len - 1) return mid - lo;
    return (hi - lo) / 2.0;
}

// Whether the Meijering combination of the scale with factor s2 is negative at image pixel (y, x); c: the pixel in g.
// The Hessian is np.gradient twice: first differences along axis 0 (g0) and axis 1 (g1) at (dy, dx) from the pixel, then
// theirs.  grad1 drops the neighbour that lies outside the image, at both levels: what the halo of g holds there (the
// blur of the reflected plane, or a difference taken at a position outside the image) is read from LDS but enters no
// result.  (A form without the edge tests for tiles inside the image measured the same and was not kept.)
__device__ __forceinline__ bool ridge_negative(const double *c, int y, int x, int H, int W, double s2, double alpha)
{
    auto at = [&](int dy, int dx) { return c[dy * kRidgeG + dx]; };
    auto g0 = [&](int dy, int dx) { return grad1(at(dy - 1, dx), at(dy, dx), at(dy + 1, dx), y + dy, H); };
    auto g1 = [&](int dy, int dx) { return grad1(at(dy, dx - 1), at(dy, dx), at(dy, dx + 1), x + dx, W); };
    const double hrr = s2 * grad1(g0(-1, 0), g0(0, 0), g0(1, 0), y, H);
    const double hrc = s2 * grad1(g0(0, -1), g0(0, 0), g0(0, 1), x, W);
    const double hcc = s2 * grad1(g1(0, -1), g1(0, 0), g1(0, 1), x, W);
    double big, small;
    hessian_eigenvalues(hrr, hrc, hcc, big, small);
    return big + alpha * small < 0.0;
}

__global__ __launch_bounds__(kRidgeThreads) void ridge_sign_kernel(const uint8_t *__restrict__ fg, int H, int W, int64_t ld,
                                                                   RidgeScales sc, uint8_t *__restrict__ out, int64_t ldo,
                                                                   int tiles_x, int64_t nblocks)
{
    // s8 comes first: its 2 R + 1 reads per output of the axis-0 pass then take their offsets as 16-bit immediates
    extern __shared__ double ridge_lds[];
    uint8_t *s8 = reinterpret_cast<uint8_t *>(ridge_lds);            // [100][100]
    double *a = ridge_lds + kRidgeS * kRidgeS / 8;                   // [68][100]
    double *g = a + kRidgeG * kRidgeAPitch;                          // [68][68]
    static_assert(kRidgeS * kRidgeS % 8 == 0, "the doubles follow the staged bytes");

    const int64_t b = xcd_contiguous(blockIdx.x, nblocks);
    if (b >= nblocks) return;
    const int y0 = (int)(b / tiles_x) * kRidgeTile, x0 = (int)(b % tiles_x) * kRidgeTile;
    const int tid = threadIdx.x;

    // the staged tile: rows and columns kRidgeOrigin - hb .. kRidgeOrigin + 64 + hb of s8
    const int hb = sc.rmax + 2, span = kRidgeTile + 2 * hb, first = kRidgeOrigin - hb;
    for (int e = tid; e < span * span; e += kRidgeThreads) {
        const int i = e / span, j = e - i * span;
        const int y = border_idx(y0 - hb + i, H, 0), x = border_idx(x0 - hb + j, W, 0);
        s8[(first + i) * kRidgeS + first + j] = fg[(int64_t)y * ld + x] != 0;
    }
    __syncthreads();

    unsigned on = 0;                                                  // bit k: pixel tid + k * 1024 of the tile
    for (int s = 0; s < sc.n; s++) {
        const int r = sc.radius[s];
        static_assert(kRidgeMaxRadius == 16, "the switch below lists the radii 1 .. 16");
        switch (r) {                                                // uniform over the workgroup, as are the barriers inside
#define PXSOM_RIDGE_CASE(R) case R: ridge_blur<R>(s8, a, g, sc.w[s], tid); break
            PXSOM_RIDGE_CASE(1); PXSOM_RIDGE_CASE(2); PXSOM_RIDGE_CASE(3); PXSOM_RIDGE_CASE(4);
            PXSOM_RIDGE_CASE(5); PXSOM_RIDGE_CASE(6); PXSOM_RIDGE_CASE(7); PXSOM_RIDGE_CASE(8);
            PXSOM_RIDGE_CASE(9); PXSOM_RIDGE_CASE(10); PXSOM_RIDGE_CASE(11); PXSOM_RIDGE_CASE(12);
            PXSOM_RIDGE_CASE(13); PXSOM_RIDGE_CASE(14); PXSOM_RIDGE_CASE(15); PXSOM_RIDGE_CASE(16);
            default: continue;                                       // no such radius passes the entry: the scale adds nothing
#undef PXSOM_RIDGE_CASE
        }
        // the sign test of this scale for the thread's four pixels
        const double s2 = sc.s2[s];
#pragma unroll
        for (int k = 0; k < kRidgeTile * kRidgeTile / kRidgeThreads; k++) {
            const int p = tid + k * kRidgeThreads, ty = p / kRidgeTile, tx = p % kRidgeTile;
            const int y = y0 + ty, x = x0 + tx;
            if (y < H && x < W && ridge_negative(g + (ty + 2) * kRidgeG + tx + 2, y, x, H, W, s2, sc.alpha)) on |= 1u << k;
        }
        // (the next scale's axis-0 pass writes `a`, which no thread reads any more; `g` is rewritten only after the
        // barrier that follows that pass)
    }
#pragma unroll
    for (int k = 0; k < kRidgeTile * kRidgeTile / kRidgeThreads; k++) {
        const int p = tid + k * kRidgeThreads, y = y0 + p / kRidgeTile, x = x0 + p % kRidgeTile;
        if (y < H && x < W) out[(int64_t)y * ldo + x] = (on >> k) & 1u;
    }
}

#pragma clang fp contract(fast)

}  // namespace

PXSOM_EXPORT int pxsom_ridge_sign(const uint8_t *fg_dev, int h, int w, int64_t ld, const double *weights_host,
                                  const int *radii_host, const double *scales_host, int n_scales, double alpha,
                                  uint8_t *out_dev, int64_t ldo, void *stream)
{
    const char *fn = "pxsom_ridge_sign";
    if (!fg_dev || !weights_host || !radii_host || !scales_host || !out_dev)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (h < 2 || w < 2)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a %d x %d plane (np.gradient needs 2 elements per axis)", fn, h, w);
    if (ld < w || ldo < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row strides %lld / %lld < w=%d", fn, (long long)ld, (long long)ldo, w);
    if (n_scales < 1 || n_scales > kRidgeMaxScales)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_scales=%d outside [1, %d]", fn, n_scales, kRidgeMaxScales);
    if (!std::isfinite(alpha)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: alpha is not finite", fn);
    for (int s = 0; s < n_scales; s++) {
        if (radii_host[s] < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: radius %d of scale %d < 1", fn, radii_host[s], s);
        if (!std::isfinite(scales_host[s]) || !(scales_host[s] > 0.0))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: factor %g of scale %d is not a finite positive number", fn, scales_host[s], s);
    }
    {   // out must not share a byte with fg
        if (pxsom::spans_overlap(out_dev, pxsom::plane_span_bytes(h, w, ldo, 1), fg_dev, pxsom::plane_span_bytes(h, w, ld, 1)))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: out overlaps fg", fn);
    }
    for (int s = 0; s < n_scales; s++)
        if (radii_host[s] > kRidgeMaxRadius)
            return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: radius %d of scale %d > %d", fn, radii_host[s], s, kRidgeMaxRadius);
    if ((int64_t)h * w > 0x7fffffffLL)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: %d x %d pixels are beyond int32", fn, h, w);

    RidgeScales sc;
    sc.n = n_scales;
    sc.rmax = 0;
    sc.alpha = alpha;
    const double *wp = weights_host;
    for (int s = 0; s < kRidgeMaxScales; s++) {
        const int r = s < n_scales ? radii_host[s] : 0;
        sc.radius[s] = r;
        sc.s2[s] = s < n_scales ? scales_host[s] : 0.0;
        for (int d = 0; d <= kRidgeMaxRadius; d++) sc.w[s][d] = (s < n_scales && d <= r) ? wp[r + d] : 0.0;
        if (s < n_scales) wp += 2 * r + 1;
        sc.rmax = std::max(sc.rmax, r);
    }
    static pxsom::PerDevice<int> raised;                              // beyond the default dynamic LDS limit
    int &have = raised.here();
    if (!have) {
        PXSOM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ridge_sign_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRidgeLds));
        have = 1;
    }
    const int tiles_x = (w + kRidgeTile - 1) / kRidgeTile;
    const int64_t nb = (int64_t)tiles_x * ((h + kRidgeTile - 1) / kRidgeTile), grid = (nb + 7) / 8 * 8;
    hipLaunchKernelGGL(ridge_sign_kernel, dim3((unsigned)grid), dim3(kRidgeThreads), kRidgeLds, reinterpret_cast<hipStream_t>(stream),
                       fg_dev, h, w, ld, sc, out_dev, ldo, tiles_x, nb);
    PXSOM_LAUNCH_CHECK("ridge_sign_kernel");
    return PXSOM_OK;
}
