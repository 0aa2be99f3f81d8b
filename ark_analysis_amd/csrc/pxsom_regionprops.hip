// pxsom_regionprops.hip -- the morphology regionprops of generate_cell_table(fast_extraction=False) on gfx950 (K17):
// the raw integers behind area, eccentricity, the axis lengths, perimeter, convex_area, centroid_dif and
// num_concavities of every cell of a finished segmentation.  A cell is every pixel of one label, connected or not;
// the floats are formed on the host from these integers (ark_analysis_amd/segmentation/regionprops_extraction.py).
//
//   shape_kernel  one workgroup per 32 x 64 tile of the label image.  The tile and a two-pixel halo are keyed through
//                 the K10 key table into LDS (dense cell index, -1 for background and outside the image); a second sweep
//                 marks the border pixels of the tile and a one-pixel halo (a pixel of a cell with a 4-neighbour that is
//                 not the cell); the third gives every border pixel its code 1 + 2 * (4-neighbours that are border
//                 pixels of the cell) + 10 * (diagonal ones) and sorts it into skimage.measure.perimeter's three weight
//                 classes.  One wave owns 64 columns of a row: every run of equal cells in it adds its sums of r^2, c^2
//                 and r * c (closed forms) and its three class counts (ballots) with one set of integer atomics --
//                 exact in any order, so every run gives the same bits.  On request the same atomics also give K12's
//                 count, coordinate sums and bounding box.
//   hull_kernel   one wave per cell whose bounding box is at most 64 x 64: lane = row, one 64-bit mask per row.  The
//                 hull of the diamond points (r +- 1/2, c), (r, c +- 1/2) is built in doubled integer coordinates from
//                 the extremes of every doubled row (monotone chain, one lane per side); every row takes its interval of
//                 centres inside or on the hull by integer division, which gives convex_area and the convex coordinate
//                 sums without a raster.  (convex row & ~cell row) is the difference image: its 4-connected components
//                 are flooded one at a time (Kogge-Stone fills along the row, shuffles between rows), each one's area and
//                 perimeter classes are counted with bit-sliced adders, and the component counts as a concavity by the
//                 reference's rule, formed in binary64 in the host's order without contraction.  A larger cell is
//                 reported in left_out and takes the host route of the package.
#include <climits>

#include "pxsom_common.h"
#include "pxsom_keytable.h"
#include "pxsom_wave.h"

namespace {

constexpr int kTileH = 32, kTileW = 64, kHalo = 2;
constexpr int kLdsW = kTileW + 2 * kHalo;          // 68
constexpr int kLdsH = kTileH + 2 * kHalo;          // 36
constexpr int kHullWaves = 4;
constexpr int kMaxSide = 64;                       // the hull kernel's bounding-box limit
constexpr int kDoubled = 2 * kMaxSide + 1;         // doubled rows of a 64-row box: 0 .. 128

template <typename TI>
__device__ __forceinline__ int32_t dense_index(const KeyTable &t, TI label)
{
    if (label == (TI)0) return -1;
    if ((int64_t)label != (int64_t)(int32_t)(int64_t)label) return -1;     // past int32: no key names it
    return (int32_t)find_key(t, (int32_t)(int64_t)label);
}

// skimage.measure.perimeter's weight class of a border pixel with n4 / nd border neighbours: 1 -> weight 1
// (codes 5, 7, 15, 17, 25, 27), 2 -> sqrt 2 (21, 33), 3 -> (1 + sqrt 2) / 2 (13, 23), 0 -> none
__device__ __forceinline__ int perimeter_class(int n4, int nd)
{
    if ((n4 == 2 || n4 == 3) && nd <= 2) return 1;
    if ((n4 == 0 && nd == 2) || (n4 == 1 && nd == 3)) return 2;
    if (n4 == 1 && (nd == 1 || nd == 2)) return 3;
    return 0;
}

__device__ __forceinline__ long long sum_squares_upto(long long x)     // 0^2 + ... + x^2, x >= -1
{
    return x * (x + 1) * (2 * x + 1) / 6;
}

__global__ __launch_bounds__(256) void stats_init_kernel(int64_t n, unsigned long long *__restrict__ count,
                                                         unsigned long long *__restrict__ sums, int32_t *__restrict__ bbox)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        count[i] = 0;
        sums[2 * i] = 0;
        sums[2 * i + 1] = 0;
        bbox[4 * i + 0] = INT_MAX;   // row min, row max, column min, column max: K12's layout
        bbox[4 * i + 1] = -1;
        bbox[4 * i + 2] = INT_MAX;
        bbox[4 * i + 3] = -1;
    }
}

template <typename TI, bool kStats>
__global__ __launch_bounds__(256) void shape_kernel(const TI *__restrict__ seg, int h, int w, int64_t ld, KeyTable t,
                                                    int tiles_x, unsigned long long *__restrict__ shape,
                                                    unsigned long long *__restrict__ count,
                                                    unsigned long long *__restrict__ sums, int32_t *__restrict__ bbox)
{
    __shared__ int32_t s_idx[kLdsH][kLdsW];
    __shared__ uint8_t s_border[kLdsH][kLdsW + 4];
    const int tr0 = (int)(blockIdx.x / tiles_x) * kTileH, tc0 = (int)(blockIdx.x % tiles_x) * kTileW;

    for (int i = threadIdx.x; i < kLdsH * kLdsW; i += 256) {
        const int lr = i / kLdsW, lc = i % kLdsW;
        const int r = tr0 - kHalo + lr, c = tc0 - kHalo + lc;
        int32_t k = -1;
        if (r >= 0 && r < h && c >= 0 && c < w) k = dense_index<TI>(t, seg[(int64_t)r * ld + c]);
        s_idx[lr][lc] = k;
        s_border[lr][lc] = 0;
    }
    __syncthreads();
    // border pixels of the tile and a one-pixel halo
    for (int i = threadIdx.x; i < (kLdsH - 2) * (kLdsW - 2); i += 256) {
        const int lr = 1 + i / (kLdsW - 2), lc = 1 + i % (kLdsW - 2);
        const int32_t k = s_idx[lr][lc];
        s_border[lr][lc] = k >= 0 && (s_idx[lr - 1][lc] != k || s_idx[lr + 1][lc] != k || s_idx[lr][lc - 1] != k ||
                                      s_idx[lr][lc + 1] != k);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = kHalo + lane, col = tc0 + lane;
    for (int j = wave; j < kTileH; j += 4) {
        const int r = tr0 + j, lr = kHalo + j;
        if (r >= h) break;                                  // whole wave
        const int32_t k = col < w ? s_idx[lr][lc] : -1;
        int cls = 0;
        if (k >= 0 && s_border[lr][lc]) {
            int n4 = 0, nd = 0;
            n4 += s_idx[lr - 1][lc] == k && s_border[lr - 1][lc];
            n4 += s_idx[lr + 1][lc] == k && s_border[lr + 1][lc];
            n4 += s_idx[lr][lc - 1] == k && s_border[lr][lc - 1];
            n4 += s_idx[lr][lc + 1] == k && s_border[lr][lc + 1];
            nd += s_idx[lr - 1][lc - 1] == k && s_border[lr - 1][lc - 1];
            nd += s_idx[lr - 1][lc + 1] == k && s_border[lr - 1][lc + 1];
            nd += s_idx[lr + 1][lc - 1] == k && s_border[lr + 1][lc - 1];
            nd += s_idx[lr + 1][lc + 1] == k && s_border[lr + 1][lc + 1];
            cls = perimeter_class(n4, nd);
        }
        const unsigned long long b1 = __ballot(cls == 1), b2 = __ballot(cls == 2), b3 = __ballot(cls == 3);
        const int32_t left = __shfl_up(k, 1, 64), right = __shfl_down(k, 1, 64);
        const bool head = k >= 0 && (lane == 0 || left != k);
        const bool tail = k >= 0 && (lane == 63 || col + 1 >= w || right != k);
        const unsigned long long heads = __ballot(head);
        if (tail) {
            const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
            const int start = 63 - __builtin_clzll(heads & upto);
            const unsigned long long run = upto & ~((1ull << start) - 1);
            const long long len = lane - start + 1, c0 = tc0 + start, c1 = col, rr = r;
            unsigned long long *out = shape + 6 * (int64_t)k;
            atomicAdd(&out[0], (unsigned long long)(rr * rr * len));
            atomicAdd(&out[1], (unsigned long long)(sum_squares_upto(c1) - sum_squares_upto(c0 - 1)));
            atomicAdd(&out[2], (unsigned long long)(rr * ((c0 + c1) * len / 2)));
            const int n1 = __popcll(b1 & run), n2 = __popcll(b2 & run), n3 = __popcll(b3 & run);
            if (n1) atomicAdd(&out[3], (unsigned long long)n1);
            if (n2) atomicAdd(&out[4], (unsigned long long)n2);
            if (n3) atomicAdd(&out[5], (unsigned long long)n3);
            if constexpr (kStats) {
                atomicAdd(&count[k], (unsigned long long)len);
                atomicAdd(&sums[2 * (int64_t)k], (unsigned long long)(rr * len));
                atomicAdd(&sums[2 * (int64_t)k + 1], (unsigned long long)((c0 + c1) * len / 2));
                atomicMin(&bbox[4 * (int64_t)k + 0], r);
                atomicMax(&bbox[4 * (int64_t)k + 1], r);
                atomicMin(&bbox[4 * (int64_t)k + 2], (int)c0);
                atomicMax(&bbox[4 * (int64_t)k + 3], (int)c1);
            }
        }
    }
}

// ---- hull kernel ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src)
{
    const int lo = __shfl((int)(unsigned)v, src, 64), hi = __shfl((int)(unsigned)(v >> 32), src, 64);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

// every bit of `open` reachable from a bit of `seed` along a run of set bits (both directions): Kogge-Stone fills
__device__ __forceinline__ unsigned long long fill_runs(unsigned long long seed, unsigned long long open)
{
    unsigned long long g = seed & open, p = open;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        g |= p & (g << s);
        p &= p << s;
    }
    unsigned long long g2 = g;
    p = open;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        g2 |= p & (g2 >> s);
        p &= p >> s;
    }
    return g2;
}

// bit-sliced sum of four one-bit planes: bit i of (s2 s1 s0) is the count at position i
__device__ __forceinline__ void add4(unsigned long long a, unsigned long long b, unsigned long long c,
                                     unsigned long long d, unsigned long long &s0, unsigned long long &s1,
                                     unsigned long long &s2)
{
    const unsigned long long h1 = a ^ b, c1 = a & b, h2 = c ^ d, c2 = c & d, c3 = h1 & h2;
    s0 = h1 ^ h2;
    s1 = c1 ^ c2 ^ c3;
    s2 = c1 & c2;
}

struct HullArgs {
    int h, w;
    int64_t ld, n;
    const int32_t *keys;
    const long long *count;
    const int32_t *bbox;
    double small_min, max_compactness, large_min;
    long long *hull;             // [n, 4]: convex area, convex row sum, convex column sum, concavities
    int32_t *left_out;           // [n]: 1 when the cell's box is past 64 x 64 (nothing computed)
};

template <typename TI>
__global__ __launch_bounds__(256) void hull_kernel(const TI *__restrict__ seg, HullArgs a)
{
#pragma clang fp contract(off)
    __shared__ int s_xmin[kHullWaves][kDoubled + 3], s_xmax[kHullWaves][kDoubled + 3];
    __shared__ short s_chain[kHullWaves][2][kDoubled + 3];
    __shared__ int s_len[kHullWaves][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * kHullWaves + wv;
    // no early return: the block's waves meet at barriers below, so an idle wave runs with an empty cell
    const bool live = k < a.n;
    const long long n_px = live ? a.count[k] : 0;
    int r0 = 0, r1 = -1, c0 = 0, c1 = -1;
    if (n_px > 0) { r0 = a.bbox[4 * k]; r1 = a.bbox[4 * k + 1]; c0 = a.bbox[4 * k + 2]; c1 = a.bbox[4 * k + 3]; }
    // a box that does not lie in the image (bad device-side input) is treated as an empty cell: no read outside seg
    const bool sane = n_px > 0 && r0 >= 0 && r1 >= r0 && r1 < a.h && c0 >= 0 && c1 >= c0 && c1 < a.w;
    const int rows = sane ? r1 - r0 + 1 : 0, cols = sane ? c1 - c0 + 1 : 0;
    const bool big = rows > kMaxSide || cols > kMaxSide;
    const int nrows = big ? 0 : rows;

    // the cell's rows as 64-bit masks: lane i keeps row r0 + i
    unsigned long long m = 0;
    const int32_t key = live ? a.keys[k] : 0;
    for (int i = 0; i < nrows; i++) {
        const bool member = lane < cols && (int64_t)seg[(int64_t)(r0 + i) * a.ld + c0 + lane] == (int64_t)key;
        const unsigned long long b = __ballot(member);
        if (lane == i) m = b;
    }

    // extremes of the doubled rows, x' = 2 (c - c0) + 2 -+ 1 so that every coordinate is positive
    {
        const int lo = m ? __builtin_ctzll(m) : 0, hi = m ? 63 - __builtin_clzll(m) : 0;
        const int own_min = m ? 2 * lo + 2 : INT_MAX, own_max = m ? 2 * hi + 2 : -1;
        int up_min = __shfl_up(own_min, 1, 64), up_max = __shfl_up(own_max, 1, 64);
        if (lane == 0) { up_min = INT_MAX; up_max = -1; }
        s_xmin[wv][2 * lane] = min(own_min, up_min);
        s_xmax[wv][2 * lane] = max(own_max, up_max);
        s_xmin[wv][2 * lane + 1] = m ? own_min - 1 : INT_MAX;
        s_xmax[wv][2 * lane + 1] = m ? own_max + 1 : -1;
        if (lane == 63) { s_xmin[wv][128] = own_min; s_xmax[wv][128] = own_max; }
    }
    __syncthreads();
    // monotone chain over the doubled rows: lane 0 the left side (x as a convex function of y), lane 1 the right
    if (lane < 2 && nrows > 0) {
        const int *x = lane == 0 ? s_xmin[wv] : s_xmax[wv];
        short *st = s_chain[wv][lane];
        int sp = 0;
        for (int y = 0; y <= 2 * nrows; y++) {
            const int xv = x[y];
            if (xv == INT_MAX || xv < 0) continue;          // a doubled row without points
            while (sp >= 2) {
                const int ya = st[sp - 2], yb = st[sp - 1];
                const long long lhs = (long long)(x[yb] - x[ya]) * (y - ya), rhs = (long long)(xv - x[ya]) * (yb - ya);
                const bool drop = lane == 0 ? lhs >= rhs : lhs <= rhs;     // b on the chord a - new or outside it
                if (!drop) break;
                sp--;
            }
            st[sp++] = (short)y;
        }
        s_len[wv][lane] = sp;
    }
    __syncthreads();

    // the row's interval of centres inside or on the hull
    unsigned long long conv = 0;
    long long area = 0, sum_r = 0, sum_c = 0;
    if (lane < nrows) {
        const int y = 2 * lane + 1;
        int bound[2];
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const int *x = side == 0 ? s_xmin[wv] : s_xmax[wv];
            const short *st = s_chain[wv][side];
            const int len = s_len[wv][side];
            // a tight box gives a chain over 0 .. 2 nrows; a box that is not tight (or holds no pixel of the key) leaves
            // rows outside the chain, which have no convex pixel
            if (len < 2 || y < st[0] || y > st[len - 1]) { bound[side] = side == 0 ? 64 : -1; continue; }
            int j = 0;
            while (j + 2 < len && st[j + 1] < y) j++;        // st[j] <= y <= st[j + 1]
            const int ya = st[j], yb = st[j + 1];
            const long long dy = yb - ya;
            const long long num = (long long)x[ya] * dy + (long long)(x[yb] - x[ya]) * (y - ya);   // x at y, times dy
            // centre x' = 2 c' + 2: left 2 c' + 2 >= num / dy, right 2 c' + 2 <= num / dy
            bound[side] = side == 0 ? (int)((num + 2 * dy - 1) / (2 * dy)) - 1 : (int)(num / (2 * dy)) - 1;
        }
        const int cl = max(bound[0], 0), cr = min(bound[1], 63);
        if (cr >= cl) {
            const int len = cr - cl + 1;
            conv = (len == 64 ? ~0ull : ((1ull << len) - 1)) << cl;
            area = len;
            sum_r = (long long)(r0 + lane) * len;
            sum_c = (long long)c0 * len + (long long)(cl + cr) * len / 2;
        }
    }
    area = pxsom::wave_sum(area);
    sum_r = pxsom::wave_sum(sum_r);
    sum_c = pxsom::wave_sum(sum_c);

    // concavities: the 4-connected components of the difference image, one flood at a time
    unsigned long long rest = conv & ~m;
    int concavities = 0;
    const double sqrt2 = 1.4142135623730951, half = (1.0 + sqrt2) / 2.0;
    for (;;) {
        const unsigned long long has = __ballot(rest != 0);
        if (has == 0) break;
        const int first = __builtin_ctzll(has);
        unsigned long long comp = lane == first ? fill_runs(rest & (~rest + 1), rest) : 0;
        for (;;) {
            unsigned long long up = shfl64(comp, lane - 1), dn = shfl64(comp, lane + 1);
            if (lane == 0) up = 0;
            if (lane == 63) dn = 0;
            const unsigned long long grown = fill_runs(comp | up | dn, rest);
            const bool changed = grown != comp;
            comp = grown;
            if (!__ballot(changed)) break;
        }
        rest &= ~comp;
        // the component's area and its perimeter classes, on the component alone
        unsigned long long up = shfl64(comp, lane - 1), dn = shfl64(comp, lane + 1);
        if (lane == 0) up = 0;
        if (lane == 63) dn = 0;
        const unsigned long long bd = comp & ~(up & dn & (comp << 1) & (comp >> 1));
        unsigned long long bu = shfl64(bd, lane - 1), bn = shfl64(bd, lane + 1);
        if (lane == 0) bu = 0;
        if (lane == 63) bn = 0;
        // a border neighbour of the same component: the component is the only cell here, so `bd` bits suffice
        unsigned long long a0, a1, a2, d0, d1, d2;
        add4(bu, bn, bd << 1, bd >> 1, a0, a1, a2);
        add4(bu << 1, bu >> 1, bn << 1, bn >> 1, d0, d1, d2);
        const unsigned long long n4_23 = a1 & ~a2, n4_0 = ~(a0 | a1 | a2), n4_1 = a0 & ~a1 & ~a2;
        const unsigned long long nd_le2 = ~d2 & ~(d1 & d0), nd_1 = d0 & ~d1 & ~d2, nd_2 = d1 & ~d0 & ~d2,
                                 nd_3 = d0 & d1 & ~d2;
        const long long ca = pxsom::wave_sum(__popcll(comp));
        const long long p1 = pxsom::wave_sum(__popcll(bd & n4_23 & nd_le2));
        const long long p2 = pxsom::wave_sum(__popcll(bd & ((n4_0 & nd_2) | (n4_1 & nd_3))));
        const long long p3 = pxsom::wave_sum(__popcll(bd & n4_1 & (nd_1 | nd_2)));
        const double p = ((double)p1 + (double)p2 * sqrt2) + (double)p3 * half;
        const double ar = (double)ca;
        if ((ar > a.small_min && (p * p) / ar < a.max_compactness) || ar > a.large_min) concavities++;
    }

    if (live && lane == 0) {
        a.hull[4 * k + 0] = area;
        a.hull[4 * k + 1] = sum_r;
        a.hull[4 * k + 2] = sum_c;
        a.hull[4 * k + 3] = concavities;
        a.left_out[k] = big ? 1 : 0;
    }
}

}  // namespace

PXSOM_EXPORT size_t pxsom_region_shape_workspace_bytes(int64_t n_keys, int32_t key_min, int32_t key_max, int flags)
{
    if (n_keys <= 0 || (flags & PXSOM_REGION_FORCE_SEARCH)) return 0;
    return pxsom::align_up(pxsom::dense_lut_bytes(n_keys, key_min, key_max), 256);
}

PXSOM_EXPORT int pxsom_region_shape(const void *seg_dev, int seg_dtype, int64_t ld, int h, int w,
                                    const int32_t *keys_dev, int64_t n_keys, int32_t key_min, int32_t key_max,
                                    int64_t *shape_dev, int64_t *count_dev, int64_t *sums_dev, int32_t *bbox_dev,
                                    void *workspace_dev, size_t workspace_bytes, int flags, void *stream)
{
    const char *fn = "pxsom_region_shape";
    if (!pxsom::is_label_dtype(seg_dtype)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad seg_dtype %d", fn, seg_dtype);
    if (h < 1 || w < 1 || ld < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad sizes (%d x %d, ld %lld)", fn, h, w, (long long)ld);
    if (flags & ~PXSOM_REGION_FORCE_SEARCH) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: unknown flags %d", fn, flags);
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null image", fn);
    if (n_keys < 0 || (n_keys > 0 && (!keys_dev || key_min > key_max || !shape_dev)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad cell table or output", fn);
    const bool stats = count_dev || sums_dev || bbox_dev;
    if (n_keys > 0 && stats && !(count_dev && sums_dev && bbox_dev))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: count, sums and bbox go together", fn);
    const size_t need = pxsom_region_shape_workspace_bytes(n_keys, key_min, key_max, flags);
    if (need && (!workspace_dev || workspace_bytes < need))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    const int tiles_x = (w + kTileW - 1) / kTileW;
    const int64_t blocks = (int64_t)((h + kTileH - 1) / kTileH) * tiles_x;
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: image too large", fn);
    if (n_keys == 0) return PXSOM_OK;

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_HIP_TRY(hipMemsetAsync(shape_dev, 0, (size_t)n_keys * 6 * sizeof(int64_t), st));
    unsigned long long *count = reinterpret_cast<unsigned long long *>(count_dev);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(sums_dev);
    if (stats) {
        hipLaunchKernelGGL(stats_init_kernel, dim3(pxsom::flat_grid(n_keys, 4)), dim3(256), 0, st, n_keys, count, sums,
                           bbox_dev);
        PXSOM_LAUNCH_CHECK("stats_init_kernel");
    }
    KeyTable t{keys_dev, nullptr, n_keys, key_min, 0};
    const size_t lut_b = need ? pxsom::dense_lut_bytes(n_keys, key_min, key_max) : 0;
    if (lut_b) {
        const int rc = build_lut(t, reinterpret_cast<int32_t *>(workspace_dev), lut_b, st);
        if (rc != PXSOM_OK) return rc;
    }
    unsigned long long *shape = reinterpret_cast<unsigned long long *>(shape_dev);
    pxsom::dispatch_label(seg_dtype, [&](auto ti) {
        typedef decltype(ti) TI;
        const TI *p = reinterpret_cast<const TI *>(seg_dev);
        if (stats) {
            PXSOM_TIMED_LAUNCH((shape_kernel<TI, true>), dim3((unsigned)blocks), dim3(256), 0, st, p, h, w, ld, t, tiles_x,
                               shape, count, sums, bbox_dev);
        } else {
            PXSOM_TIMED_LAUNCH((shape_kernel<TI, false>), dim3((unsigned)blocks), dim3(256), 0, st, p, h, w, ld, t,
                               tiles_x, shape, count, sums, bbox_dev);
        }
    });
    PXSOM_LAUNCH_CHECK("shape_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_region_hull(const void *seg_dev, int seg_dtype, int64_t ld, int h, int w,
                                   const int32_t *keys_dev, int64_t n_keys, const int64_t *count_dev,
                                   const int32_t *bbox_dev, double small_concavity_minimum, double max_compactness,
                                   double large_concavity_minimum, int64_t *hull_dev, int32_t *left_out_dev, void *stream)
{
    const char *fn = "pxsom_region_hull";
    if (!pxsom::is_label_dtype(seg_dtype)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad seg_dtype %d", fn, seg_dtype);
    if (h < 1 || w < 1 || ld < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad sizes (%d x %d, ld %lld)", fn, h, w, (long long)ld);
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null image", fn);
    if (n_keys < 0 || (n_keys > 0 && (!keys_dev || !count_dev || !bbox_dev || !hull_dev || !left_out_dev)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad cell table or outputs", fn);
    if (small_concavity_minimum != small_concavity_minimum || max_compactness != max_compactness ||
        large_concavity_minimum != large_concavity_minimum)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: NaN threshold", fn);
    const int64_t blocks = (n_keys + kHullWaves - 1) / kHullWaves;
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: too many cells", fn);
    if (n_keys == 0) return PXSOM_OK;

    HullArgs a;
    a.h = h;
    a.w = w;
    a.ld = ld;
    a.n = n_keys;
    a.keys = keys_dev;
    a.count = reinterpret_cast<const long long *>(count_dev);
    a.bbox = bbox_dev;
    a.small_min = small_concavity_minimum;
    a.max_compactness = max_compactness;
    a.large_min = large_concavity_minimum;
    a.hull = reinterpret_cast<long long *>(hull_dev);
    a.left_out = left_out_dev;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    pxsom::dispatch_label(seg_dtype, [&](auto ti) {
        typedef decltype(ti) TI;
        PXSOM_TIMED_LAUNCH((hull_kernel<TI>), dim3((unsigned)blocks), dim3(256), 0, st,
                           reinterpret_cast<const TI *>(seg_dev), a);
    });
    PXSOM_LAUNCH_CHECK("hull_kernel");
    return PXSOM_OK;
}
