// pxsom_watershed.hip -- K28: the marker watershed of fibre segmentation
// (ark.segmentation.fiber_segmentation.segment_fibers: `watershed(elevation_map, threshed)`), the priority flood of
// tests/watershed_reference.py computed in parallel rounds, exactly.
//
// The flood runs level by level and is a FIFO inside a level; a pixel takes the label of the first of its neighbours to be
// popped.  One round pops the whole frontier -- the labelled, not yet popped pixels of the current level h, in pop order:
//
//   claim_kernel          frontier element i claims each unlabelled 4-neighbour n (k = 0 .. 3: -W, -1, +1, +W) with
//                         atomicMin(claim[n], 8 i + k): the smallest key is the earliest push
//   descent (rare)        a claimed pixel below h is a basin the sequential flood fills at once, before the next pop of level
//                         h.  basin_mask_kernel marks {unlabelled, value < h}, pxsom_label_components finds its 4-connected
//                         components, basin_min_kernel gives each the smallest claim in it, basin_rim_kernel claims every
//                         unlabelled neighbour >= h of a claimed component with 8 i + 4 (after i's own pushes, before those of
//                         i + 1), basin_label_kernel labels the basins and the rim winners and numbers the latter per parent
//   label_count_kernel    element i labels the neighbours whose claim is still its own and counts, per block, the winners
//                         at level h (the next frontier) and above it (appended to the pending list)
//   scan_totals_kernel    one workgroup: exclusive scan of the block totals, the sizes the host reads
//   scatter_round_kernel  ordered emission: the block scan again, then each winner at its place -- by key, not sorted
//   rim_scatter_kernel    (descent rounds) the rim winners behind their parent's direct winners; equal keys in any order
//
// When the frontier runs empty the next level is the smallest pending value; its first frontier is the stable selection of
// the pending list (the markers in raster order, then every pixel appended since) by value == h: count_level_kernel,
// scan_totals_kernel, scatter_level_kernel.  The rounds are driven from the host: per round one 40-byte read-back (the
// next frontier's size, the pending size, whether that frontier touches a basin, the smallest pending value).  No kernel waits on
// another one; every pixel is popped once, so rounds and levels are each at most h w, and the entry returns an error past
// that instead of launching again.  Integer atomics only, and the labels do not depend on their order.
#include <climits>
#include <cstdint>

#include "pxsom_common.h"
#include "pxsom_plane.h"

namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kEmpty = ~0ull;               // no claim
constexpr long long kNoLevel = LLONG_MAX;                  // nothing pending
constexpr int kModeMarkers = 0, kModeLevel = 1, kModeRound = 2;

struct State {
    long long n_front;     // size of the frontier just written
    long long n_pend;      // size of the pending list
    long long descent;     // that frontier has an unlabelled neighbour below its level
    long long min_pend;    // the smallest pending value, kNoLevel without one
    long long labelled;    // pixels the flood has labelled so far
};

struct Plane {
    const int32_t *elev;
    int64_t lde;
    int32_t *out;
    int64_t ldo;
    int h, w;
};

__device__ __forceinline__ int64_t at(int p, int w, int64_t ld)
{
    const unsigned y = (unsigned)p / (unsigned)w;
    return (int64_t)y * ld + ((unsigned)p - y * (unsigned)w);
}

// the k-th 4-neighbour of pixel p = (y, x), -1 outside the plane: -W, -1, +1, +W
__device__ __forceinline__ int neighbour(int p, int y, int x, int k, int h, int w)
{
    if (k == 0) return y > 0 ? p - w : -1;
    if (k == 1) return x > 0 ? p - 1 : -1;
    if (k == 2) return x < w - 1 ? p + 1 : -1;
    return y < h - 1 ? p + w : -1;
}

__device__ __forceinline__ void claim_min(unsigned long long *claim, int n, unsigned long long key)
{
    __hip_atomic_fetch_min(&claim[n], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// exclusive scan of (a, b) over the workgroup's 256 threads, and the workgroup's totals
__device__ __forceinline__ void block_scan2(unsigned a, unsigned b, unsigned &ea, unsigned &eb, unsigned &ta, unsigned &tb)
{
    __shared__ unsigned sa[kBlock], sb[kBlock];
    const int t = threadIdx.x;
    sa[t] = a;
    sb[t] = b;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const unsigned xa = t >= off ? sa[t - off] : 0u, xb = t >= off ? sb[t - off] : 0u;
        __syncthreads();
        sa[t] += xa;
        sb[t] += xb;
        __syncthreads();
    }
    ea = sa[t] - a;
    eb = sb[t] - b;
    ta = sa[kBlock - 1];
    tb = sb[kBlock - 1];
    __syncthreads();
}

// a pixel that joins the pending list lowers the smallest pending value; most do not, and those skip the atomic
__device__ __forceinline__ void pend_min(State *st, int v)
{
    if ((long long)v < __hip_atomic_load(&st->min_pend, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_min(&st->min_pend, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a pixel that joins the frontier of level lev: does it touch an unlabelled pixel below lev?
__device__ __forceinline__ void flag_descent(const Plane &pl, int p, int lev, State *st)
{
    const int y = (int)((unsigned)p / (unsigned)pl.w), x = p - y * pl.w;
    bool below = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int n = neighbour(p, y, x, k, pl.h, pl.w);
        if (n >= 0 && pl.out[at(n, pl.w, pl.ldo)] == 0 && pl.elev[at(n, pl.w, pl.lde)] < lev) below = true;
    }
    if (below) st->descent = 1;
}

// ---- the start: out = markers, the pending list = the markers in raster order ---------------------------------------------
__global__ __launch_bounds__(kBlock) void count_markers_kernel(Plane pl, const int32_t *__restrict__ markers, int64_t ldm, int total,
                                                               unsigned *__restrict__ tot_a, unsigned *__restrict__ tot_b,
                                                               long long *__restrict__ block_min)
{
    __shared__ long long s_min;
    if (threadIdx.x == 0) s_min = kNoLevel;
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned b = 0;
    if (e < total) {
        const int m = markers[at((int)e, pl.w, ldm)];
        pl.out[at((int)e, pl.w, pl.ldo)] = m;
        if (m != 0) {
            b = 1;
            atomicMin(&s_min, (long long)pl.elev[at((int)e, pl.w, pl.lde)]);
        }
    }
    unsigned ea, eb, ta, tb;
    block_scan2(0u, b, ea, eb, ta, tb);
    if (threadIdx.x == 0) {
        tot_a[blockIdx.x] = 0;
        tot_b[blockIdx.x] = tb;
        block_min[blockIdx.x] = s_min;
    }
}

__global__ __launch_bounds__(kBlock) void scatter_markers_kernel(Plane pl, int total, const unsigned *__restrict__ tot_b,
                                                                 int *__restrict__ pend)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const unsigned b = e < total && pl.out[at((int)e, pl.w, pl.ldo)] != 0;
    unsigned ea, eb, ta, tb;
    block_scan2(0u, b, ea, eb, ta, tb);
    if (b) pend[tot_b[blockIdx.x] + eb] = (int)e;
}

// ---- a level's first frontier: the pending pixels of value lev, in order; the others stay pending, in order -----------------
__global__ __launch_bounds__(kBlock) void count_level_kernel(Plane pl, const int *__restrict__ pend, int n_pend, int lev,
                                                             unsigned *__restrict__ tot_a, unsigned *__restrict__ tot_b,
                                                             long long *__restrict__ block_min)
{
    __shared__ long long s_min;
    if (threadIdx.x == 0) s_min = kNoLevel;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned a = 0, b = 0;
    if (j < n_pend) {
        const int v = pl.elev[at(pend[j], pl.w, pl.lde)];
        a = v == lev;
        b = v != lev;                                          // (nothing pending lies below the smallest pending value)
        if (b) atomicMin(&s_min, (long long)v);
    }
    unsigned ea, eb, ta, tb;
    block_scan2(a, b, ea, eb, ta, tb);
    if (threadIdx.x == 0) {
        tot_a[blockIdx.x] = ta;
        tot_b[blockIdx.x] = tb;
        block_min[blockIdx.x] = s_min;
    }
}

__global__ __launch_bounds__(kBlock) void scatter_level_kernel(Plane pl, const int *__restrict__ pend, int n_pend, int lev,
                                                               const unsigned *__restrict__ tot_a, const unsigned *__restrict__ tot_b,
                                                               int *__restrict__ front, int *__restrict__ pend_next, State *st)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned a = 0, b = 0;
    int p = 0;
    if (j < n_pend) {
        p = pend[j];
        a = pl.elev[at(p, pl.w, pl.lde)] == lev;
        b = !a;
    }
    unsigned ea, eb, ta, tb;
    block_scan2(a, b, ea, eb, ta, tb);
    if (a) {
        front[tot_a[blockIdx.x] + ea] = p;
        flag_descent(pl, p, lev, st);
    }
    if (b) pend_next[tot_b[blockIdx.x] + eb] = p;
}

// ---- one round ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void claim_kernel(Plane pl, const int *__restrict__ front, int n_front,
                                                       unsigned long long *__restrict__ claim)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_front) return;
    const int p = front[i], y = (int)((unsigned)p / (unsigned)pl.w), x = p - y * pl.w;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int n = neighbour(p, y, x, k, pl.h, pl.w);
        if (n >= 0 && pl.out[at(n, pl.w, pl.ldo)] == 0) claim_min(claim, n, (unsigned long long)i * 8 + k);
    }
}

// Element i labels the neighbours it won and notes, two bits per neighbour, where each goes: 1 the next frontier (value
// == lev), 2 the pending list (value > lev).  A neighbour below lev belongs to a basin, which the descent kernels have
// labelled already; it goes nowhere.  rim_a / rim_b: the rim winners of i's basins, counted by basin_label_kernel.
__global__ __launch_bounds__(kBlock) void label_count_kernel(Plane pl, const int *__restrict__ front, int n_front, int lev,
                                                             unsigned long long *__restrict__ claim, uint8_t *__restrict__ codes,
                                                             const unsigned *__restrict__ rim_a, const unsigned *__restrict__ rim_b,
                                                             unsigned *__restrict__ tot_a, unsigned *__restrict__ tot_b)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned a = 0, b = 0;
    if (i < n_front) {
        const int p = front[i], y = (int)((unsigned)p / (unsigned)pl.w), x = p - y * pl.w;
        const int lab = pl.out[at(p, pl.w, pl.ldo)];
        unsigned code = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int n = neighbour(p, y, x, k, pl.h, pl.w);
            if (n < 0 || claim[n] != (unsigned long long)i * 8 + k) continue;
            claim[n] = kEmpty;
            const int v = pl.elev[at(n, pl.w, pl.lde)];
            if (v < lev) continue;
            pl.out[at(n, pl.w, pl.ldo)] = lab;
            if (v == lev) {
                code |= 1u << (2 * k);
                a++;
            } else {
                code |= 2u << (2 * k);
                b++;
            }
        }
        codes[i] = (uint8_t)code;
        if (rim_a) {
            a += rim_a[i];
            b += rim_b[i];
        }
    }
    unsigned ea, eb, ta, tb;
    block_scan2(a, b, ea, eb, ta, tb);
    if (threadIdx.x == 0) {
        tot_a[blockIdx.x] = ta;
        tot_b[blockIdx.x] = tb;
    }
}

// One workgroup: the block totals become exclusive offsets, and the state takes the sizes that the host reads.
__global__ __launch_bounds__(1024) void scan_totals_kernel(unsigned *__restrict__ tot_a, unsigned *__restrict__ tot_b,
                                                           const long long *__restrict__ block_min, int64_t nb, int mode, State *st)
{
    __shared__ unsigned sa[1024], sb[1024];
    __shared__ long long smin[1024];
    const int t = threadIdx.x;
    unsigned carry_a = 0, carry_b = 0;
    long long mn = kNoLevel;
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t j = base + t;
        const unsigned a = j < nb ? tot_a[j] : 0u, b = j < nb ? tot_b[j] : 0u;
        if (block_min && j < nb && block_min[j] < mn) mn = block_min[j];
        sa[t] = a;
        sb[t] = b;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const unsigned xa = t >= off ? sa[t - off] : 0u, xb = t >= off ? sb[t - off] : 0u;
            __syncthreads();
            sa[t] += xa;
            sb[t] += xb;
            __syncthreads();
        }
        if (j < nb) {
            tot_a[j] = carry_a + sa[t] - a;
            tot_b[j] = carry_b + sb[t] - b;
        }
        carry_a += sa[1023];
        carry_b += sb[1023];
        __syncthreads();
    }
    smin[t] = mn;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s && smin[t + s] < smin[t]) smin[t] = smin[t + s];
        __syncthreads();
    }
    if (t == 0) {
        st->n_front = carry_a;
        st->descent = 0;                                       // set by the scatter kernel that follows
        if (mode == kModeRound) {
            st->n_pend += carry_b;
            st->labelled += (long long)carry_a + carry_b;
        } else {
            st->n_pend = carry_b;
            st->min_pend = smin[0];
            if (mode == kModeMarkers) st->labelled = 0;
        }
    }
}

// Ordered emission of a round: element i's winners stand behind those of every element before it, its direct winners in
// the order k = 0 .. 3 and its rim winners behind them (their places are left in rim_a / rim_b for rim_scatter_kernel).
__global__ __launch_bounds__(kBlock) void scatter_round_kernel(Plane pl, const int *__restrict__ front, int n_front, int lev,
                                                               const uint8_t *__restrict__ codes, unsigned *__restrict__ rim_a,
                                                               unsigned *__restrict__ rim_b, const unsigned *__restrict__ tot_a,
                                                               const unsigned *__restrict__ tot_b, int *__restrict__ front_next,
                                                               int *__restrict__ pend, unsigned pend_base, State *st)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned a = 0, b = 0, code = 0;
    if (i < n_front) {
        code = codes[i];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned c = (code >> (2 * k)) & 3u;
            a += c == 1u;
            b += c == 2u;
        }
        if (rim_a) {
            a += rim_a[i];
            b += rim_b[i];
        }
    }
    unsigned ea, eb, ta, tb;
    block_scan2(a, b, ea, eb, ta, tb);
    if (i >= n_front) return;
    unsigned pos_a = tot_a[blockIdx.x] + ea, pos_b = pend_base + tot_b[blockIdx.x] + eb;
    if (code) {
        const int p = front[i], y = (int)((unsigned)p / (unsigned)pl.w), x = p - y * pl.w;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned c = (code >> (2 * k)) & 3u;
            if (!c) continue;
            const int n = neighbour(p, y, x, k, pl.h, pl.w);
            if (c == 1u) {
                front_next[pos_a++] = n;
                flag_descent(pl, n, lev, st);
            } else {
                pend[pos_b++] = n;
                pend_min(st, pl.elev[at(n, pl.w, pl.lde)]);
            }
        }
    }
    if (rim_a) {
        rim_a[i] = pos_a;
        rim_b[i] = pos_b;
    }
}

// ---- the descent path: whole-plane kernels, one thread per pixel ----------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void basin_mask_kernel(Plane pl, int total, int lev, uint8_t *__restrict__ fg)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    fg[e] = pl.out[at((int)e, pl.w, pl.ldo)] == 0 && pl.elev[at((int)e, pl.w, pl.lde)] < lev;
}

__global__ __launch_bounds__(kBlock) void basin_min_kernel(int total, const uint8_t *__restrict__ fg, const int32_t *__restrict__ comp,
                                                           const unsigned long long *__restrict__ claim,
                                                           unsigned long long *__restrict__ comp_min, int64_t capacity)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total || !fg[e]) return;
    const unsigned long long key = claim[e];
    const int c = comp[e];
    if (key != kEmpty && c > 0 && c < capacity) __hip_atomic_fetch_min(&comp_min[c], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void basin_rim_kernel(Plane pl, int total, int lev, const uint8_t *__restrict__ fg,
                                                           const int32_t *__restrict__ comp, const unsigned long long *__restrict__ comp_min,
                                                           int64_t capacity, unsigned long long *__restrict__ claim)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total || !fg[e]) return;
    const int c = comp[e];
    if (c <= 0 || c >= capacity) return;
    const unsigned long long cm = comp_min[c];
    if (cm == kEmpty) return;
    const int p = (int)e, y = (int)((unsigned)p / (unsigned)pl.w), x = p - y * pl.w;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int n = neighbour(p, y, x, k, pl.h, pl.w);
        if (n >= 0 && pl.out[at(n, pl.w, pl.ldo)] == 0 && pl.elev[at(n, pl.w, pl.lde)] >= lev) claim_min(claim, n, (cm >> 3) * 8 + 4);
    }
}

__global__ __launch_bounds__(kBlock) void basin_label_kernel(Plane pl, int total, int lev, const uint8_t *__restrict__ fg,
                                                             const int32_t *__restrict__ comp, const unsigned long long *__restrict__ comp_min,
                                                             int64_t capacity, const unsigned long long *__restrict__ claim,
                                                             const int *__restrict__ front, unsigned *__restrict__ rim_a,
                                                             unsigned *__restrict__ rim_b, unsigned *__restrict__ rim_off, State *st)
{
    __shared__ unsigned s_basin;
    if (threadIdx.x == 0) s_basin = 0;
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < total && pl.out[at((int)e, pl.w, pl.ldo)] == 0) {
        if (fg[e]) {
            const int c = comp[e];
            const unsigned long long cm = c > 0 && c < capacity ? comp_min[c] : kEmpty;
            if (cm != kEmpty) {
                pl.out[at((int)e, pl.w, pl.ldo)] = pl.out[at(front[cm >> 3], pl.w, pl.ldo)];
                atomicAdd(&s_basin, 1u);
            }
        } else {
            const unsigned long long key = claim[e];
            if (key != kEmpty && (key & 7) == 4) {
                const unsigned long long i = key >> 3;
                pl.out[at((int)e, pl.w, pl.ldo)] = pl.out[at(front[i], pl.w, pl.ldo)];
                rim_off[e] = atomicAdd(pl.elev[at((int)e, pl.w, pl.lde)] == lev ? &rim_a[i] : &rim_b[i], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_basin) atomicAdd(reinterpret_cast<unsigned long long *>(&st->labelled), (unsigned long long)s_basin);
}

__global__ __launch_bounds__(kBlock) void rim_scatter_kernel(Plane pl, int total, int lev, unsigned long long *__restrict__ claim,
                                                             const unsigned *__restrict__ rim_a, const unsigned *__restrict__ rim_b,
                                                             const unsigned *__restrict__ rim_off, int *__restrict__ front_next,
                                                             int *__restrict__ pend, State *st)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const unsigned long long key = claim[e];
    if (key == kEmpty || (key & 7) != 4) return;
    claim[e] = kEmpty;
    const unsigned long long i = key >> 3;
    const int v = pl.elev[at((int)e, pl.w, pl.lde)];
    if (v == lev) {
        front_next[rim_a[i] + rim_off[e]] = (int)e;
        flag_descent(pl, (int)e, lev, st);
    } else {
        pend[rim_b[i] + rim_off[e]] = (int)e;
        pend_min(st, v);
    }
}

// ---- the workspace ---------------------------------------------------------------------------------------------------------------
struct Layout {
    size_t claim, front[2], pend[2], codes, rim_a, rim_b, rim_off, tot_a, tot_b, block_min, state, fg, comp, comp_min, ccl_n, ccl_areas,
        ccl_ws, ccl_ws_bytes, total;
    int64_t comp_capacity;
};

Layout layout(int h, int w)
{
    Layout l{};
    const size_t n = (size_t)h * (size_t)w, nb = (n + kBlock - 1) / kBlock;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += pxsom::align_up(bytes, 256);
        return at;
    };
    l.comp_capacity = (int64_t)(n + 1) / 2 + 1;                // a 4-connected checkerboard has the most components
    l.claim = take(n * 8);
    l.front[0] = take(n * 4);
    l.front[1] = take(n * 4);
    l.pend[0] = take(n * 4);
    l.pend[1] = take(n * 4);
    l.codes = take(n);
    l.rim_a = take(n * 4);
    l.rim_b = take(n * 4);
    l.rim_off = take(n * 4);
    l.tot_a = take(nb * 4);
    l.tot_b = take(nb * 4);
    l.block_min = take(nb * 8);
    l.state = take(sizeof(State));
    l.fg = take(n);
    l.comp = take(n * 4);
    l.comp_min = take((size_t)l.comp_capacity * 8);
    l.ccl_n = take(4);
    l.ccl_areas = take(4);
    l.ccl_ws_bytes = pxsom_label_components_workspace_bytes(h, w);
    l.ccl_ws = take(l.ccl_ws_bytes);
    l.total = off;
    return l;
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

PXSOM_EXPORT size_t pxsom_watershed_workspace_bytes(int h, int w)
{
    if (pxsom_label_components_workspace_bytes(h, w) == 0) return 0;
    return layout(h, w).total;
}

PXSOM_EXPORT int pxsom_watershed(const int32_t *elev_dev, int64_t lde, const int32_t *markers_dev, int64_t ldm, int h, int w,
                                 int32_t *out_dev, int64_t ldo, void *workspace_dev, size_t workspace_bytes, int64_t *stats_host,
                                 void *stream)
{
    const char *fn = "pxsom_watershed";
    if (!elev_dev || !markers_dev || !out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if ((reinterpret_cast<uintptr_t>(elev_dev) & 3) || (reinterpret_cast<uintptr_t>(markers_dev) & 3) ||
        (reinterpret_cast<uintptr_t>(out_dev) & 3))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a plane is not 4-byte aligned", fn);
    if (h < 1 || w < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a %d x %d plane", fn, h, w);
    if (lde < w || ldm < w || ldo < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: row strides %lld / %lld / %lld < w=%d", fn, (long long)lde, (long long)ldm,
                           (long long)ldo, w);
    if (pxsom_label_components_workspace_bytes(h, w) == 0)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: %d x %d pixels are beyond what pxsom_label_components takes", fn, h, w);
    {   // the labels grow in out while both inputs are still read
        const size_t out_bytes = pxsom::plane_span_bytes(h, w, ldo, 4);
        if (pxsom::spans_overlap(out_dev, out_bytes, elev_dev, pxsom::plane_span_bytes(h, w, lde, 4)) ||
            pxsom::spans_overlap(out_dev, out_bytes, markers_dev, pxsom::plane_span_bytes(h, w, ldm, 4)))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: out overlaps an input", fn);
    }
    const Layout l = layout(h, w);
    if (!workspace_dev || workspace_bytes < l.total)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_dev ? workspace_bytes : (size_t)0,
                           l.total);
    if (reinterpret_cast<uintptr_t>(workspace_dev) & 15)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: the workspace is not 16-byte aligned", fn);

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_dev);
    unsigned long long *claim = reinterpret_cast<unsigned long long *>(ws + l.claim);
    int *front[2] = {reinterpret_cast<int *>(ws + l.front[0]), reinterpret_cast<int *>(ws + l.front[1])};
    int *pend[2] = {reinterpret_cast<int *>(ws + l.pend[0]), reinterpret_cast<int *>(ws + l.pend[1])};
    uint8_t *codes = reinterpret_cast<uint8_t *>(ws + l.codes);
    unsigned *rim_a = reinterpret_cast<unsigned *>(ws + l.rim_a), *rim_b = reinterpret_cast<unsigned *>(ws + l.rim_b);
    unsigned *rim_off = reinterpret_cast<unsigned *>(ws + l.rim_off);
    unsigned *tot_a = reinterpret_cast<unsigned *>(ws + l.tot_a), *tot_b = reinterpret_cast<unsigned *>(ws + l.tot_b);
    long long *block_min = reinterpret_cast<long long *>(ws + l.block_min);
    State *state = reinterpret_cast<State *>(ws + l.state);
    uint8_t *fg = reinterpret_cast<uint8_t *>(ws + l.fg);
    int32_t *comp = reinterpret_cast<int32_t *>(ws + l.comp);
    unsigned long long *comp_min = reinterpret_cast<unsigned long long *>(ws + l.comp_min);
    int32_t *ccl_n = reinterpret_cast<int32_t *>(ws + l.ccl_n), *ccl_areas = reinterpret_cast<int32_t *>(ws + l.ccl_areas);

    const Plane pl{elev_dev, lde, out_dev, ldo, h, w};
    const int total = h * w;
    const int64_t bound = (int64_t)total + 1;                  // every pixel is popped once: rounds, and levels, <= h w
    const unsigned plane_blocks = blocks_for(total);
    State host{};
    auto read_state = [&]() -> hipError_t {
        const hipError_t e = hipMemcpyAsync(&host, state, sizeof(State), hipMemcpyDeviceToHost, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    };

    PXSOM_HIP_TRY(hipMemsetAsync(claim, 0xff, (size_t)total * 8, st));
    hipLaunchKernelGGL(count_markers_kernel, dim3(plane_blocks), dim3(kBlock), 0, st, pl, markers_dev, ldm, total, tot_a, tot_b, block_min);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(1024), 0, st, tot_a, tot_b, block_min, (int64_t)plane_blocks, kModeMarkers, state);
    hipLaunchKernelGGL(scatter_markers_kernel, dim3(plane_blocks), dim3(kBlock), 0, st, pl, total, tot_b, pend[0]);
    PXSOM_LAUNCH_CHECK("pxsom_watershed start kernels");
    PXSOM_HIP_TRY(read_state());

    int64_t rounds = 0, levels = 0, descents = 0;
    int cur_p = 0, cur_f = 0;
    while (host.min_pend != kNoLevel) {
        if (++levels > bound) return pxsom::fail(PXSOM_ERR_HIP, "%s: internal error: more than %lld levels", fn, (long long)bound);
        if (host.n_pend < 1 || host.n_pend > total || host.min_pend < INT32_MIN || host.min_pend > INT32_MAX)
            return pxsom::fail(PXSOM_ERR_HIP, "%s: internal error: pending list of %lld, level %lld", fn, (long long)host.n_pend,
                               (long long)host.min_pend);
        const int lev = (int)host.min_pend, n_pend = (int)host.n_pend;
        const unsigned pb = blocks_for(n_pend);
        hipLaunchKernelGGL(count_level_kernel, dim3(pb), dim3(kBlock), 0, st, pl, pend[cur_p], n_pend, lev, tot_a, tot_b, block_min);
        hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(1024), 0, st, tot_a, tot_b, block_min, (int64_t)pb, kModeLevel, state);
        hipLaunchKernelGGL(scatter_level_kernel, dim3(pb), dim3(kBlock), 0, st, pl, pend[cur_p], n_pend, lev, tot_a, tot_b, front[cur_f],
                           pend[cur_p ^ 1], state);
        PXSOM_LAUNCH_CHECK("pxsom_watershed level kernels");
        PXSOM_HIP_TRY(read_state());
        cur_p ^= 1;

        while (host.n_front > 0) {
            if (++rounds > bound) return pxsom::fail(PXSOM_ERR_HIP, "%s: internal error: more than %lld rounds", fn, (long long)bound);
            if (host.n_front > total || host.n_pend < 0 || host.n_pend > total)
                return pxsom::fail(PXSOM_ERR_HIP, "%s: internal error: frontier of %lld, pending list of %lld", fn,
                                   (long long)host.n_front, (long long)host.n_pend);
            const int n_front = (int)host.n_front;
            const unsigned fb = blocks_for(n_front);
            const bool descent = host.descent != 0;
            hipLaunchKernelGGL(claim_kernel, dim3(fb), dim3(kBlock), 0, st, pl, front[cur_f], n_front, claim);
            if (descent) {
                descents++;
                hipLaunchKernelGGL(basin_mask_kernel, dim3(plane_blocks), dim3(kBlock), 0, st, pl, total, lev, fg);
                if (const int rc = pxsom_label_components(fg, h, w, w, 1, 0, comp, w, ccl_n, ccl_areas, 1, ws + l.ccl_ws, l.ccl_ws_bytes, stream))
                    return rc;
                PXSOM_HIP_TRY(hipMemsetAsync(comp_min, 0xff, (size_t)l.comp_capacity * 8, st));
                PXSOM_HIP_TRY(hipMemsetAsync(rim_a, 0, (size_t)n_front * 4, st));
                PXSOM_HIP_TRY(hipMemsetAsync(rim_b, 0, (size_t)n_front * 4, st));
                hipLaunchKernelGGL(basin_min_kernel, dim3(plane_blocks), dim3(kBlock), 0, st, total, fg, comp, claim, comp_min, l.comp_capacity);
                hipLaunchKernelGGL(basin_rim_kernel, dim3(plane_blocks), dim3(kBlock), 0, st, pl, total, lev, fg, comp, comp_min,
                                   l.comp_capacity, claim);
                hipLaunchKernelGGL(basin_label_kernel, dim3(plane_blocks), dim3(kBlock), 0, st, pl, total, lev, fg, comp, comp_min,
                                   l.comp_capacity, claim, front[cur_f], rim_a, rim_b, rim_off, state);
            }
            unsigned *ra = descent ? rim_a : nullptr, *rb = descent ? rim_b : nullptr;
            hipLaunchKernelGGL(label_count_kernel, dim3(fb), dim3(kBlock), 0, st, pl, front[cur_f], n_front, lev, claim, codes, ra, rb,
                               tot_a, tot_b);
            hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(1024), 0, st, tot_a, tot_b, (const long long *)nullptr, (int64_t)fb,
                               kModeRound, state);
            hipLaunchKernelGGL(scatter_round_kernel, dim3(fb), dim3(kBlock), 0, st, pl, front[cur_f], n_front, lev, codes, ra, rb, tot_a,
                               tot_b, front[cur_f ^ 1], pend[cur_p], (unsigned)host.n_pend, state);
            if (descent)
                hipLaunchKernelGGL(rim_scatter_kernel, dim3(plane_blocks), dim3(kBlock), 0, st, pl, total, lev, claim, rim_a, rim_b, rim_off,
                                   front[cur_f ^ 1], pend[cur_p], state);
            PXSOM_LAUNCH_CHECK("pxsom_watershed round kernels");
            PXSOM_HIP_TRY(read_state());
            cur_f ^= 1;
        }
    }
    if (stats_host) {
        stats_host[0] = rounds;
        stats_host[1] = levels;
        stats_host[2] = descents;
        stats_host[3] = host.labelled;
    }
    return PXSOM_OK;
}
