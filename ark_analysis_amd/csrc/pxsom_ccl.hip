// pxsom_ccl.hip -- object masks on gfx950 (K16): connected-component labelling and the passes around it.
//
//   pxsom_label_components          skimage.measure.label / scipy.ndimage.label of a binary plane (4- or 8-neighbourhood),
//                                   with the component count and the area table
//   pxsom_components_select         remove_small_holes' fill / the area filter of _create_object_mask, from the area table
//   pxsom_binarize_plane            the three foreground predicates of _create_object_mask
//   pxsom_label_regions             skimage.measure.label(img, background=0) of an integer label plane (K18): regions of
//                                   equal non-zero value; stages 1 and 2 in valued forms, stages 3 and 4 as they are
// (The blur of _create_object_mask is pxsom_gaussian_blur_plane_mode of pxsom_pre.hip.)
//
// Labelling is union-find on linear pixel indices, parent <= child everywhere, so the root of a component IS its first pixel
// in raster order -- ranking the roots by index gives skimage's numbering.  Four stages:
//   1. tile_label_kernel     one 64 x 64 tile per workgroup in LDS: a row of the tile is one wave, the wave's ballot gives
//                            every pixel its run start; runs are joined to the row above with LDS atomicMin; the flattened
//                            tile is written out as global parents
//   2. border_merge_kernel   the pixels of tile edges join their neighbours across the edge with global atomicMin
//   3. flatten_count_kernel  every pixel gets its root; roots are counted per 256 pixels, ccl_scan_kernel turns the counts
//                            into offsets, rank_roots_kernel writes rank + 1 at every root
//   4. finish_labels_kernel  every other pixel copies its root's label; areas by int32 atomic adds: one per workgroup for
//                            the label its 4096 pixels start with, one per run of equal labels in a wave for the others
// Integer arithmetic only: whatever the order of the atomics, the final partition, the roots and so the labels are the same.
#include "pxsom_common.h"
#include "pxsom_plane.h"

namespace {

constexpr int kTile = 64;          // tile edge == wave width: lane <-> tile column
constexpr int kChunk = 256;        // pixels per workgroup of the flat passes

__device__ __forceinline__ int ld_relaxed(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int *parent, int p)
{
    int q = ld_relaxed(parent + p);
    while (q != p) {
        p = q;
        q = ld_relaxed(parent + p);
    }
    return p;
}

// Joins the sets of a and b (both foreground).  The larger root is hung under the smaller with atomicMin; if another
// thread got there first, its value takes the larger root's place and the join goes on from there.
__device__ __forceinline__ void uf_union(int *parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(256) void tile_label_kernel(const uint8_t *__restrict__ src, int64_t ld, int h, int w, int invert,
                                                         int conn8, int *__restrict__ parent, int tiles_x, int64_t ntiles)
{
    __shared__ int lab[kTile * kTile];
    __shared__ unsigned long long rowmask[kTile];
    const int64_t tile = xcd_contiguous(blockIdx.x, ntiles);   // neighbouring tiles go to one XCD
    if (tile >= ntiles) return;
    const int ty0 = (int)(tile / tiles_x) * kTile, tx0 = (int)(tile % tiles_x) * kTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = tx0 + lane;

    // run starts: lane's run begins after the highest background lane below it
    for (int r = wave; r < kTile; r += 4) {
        const int y = ty0 + r;
        bool fg = false;
        if (y < h && x < w) fg = (src[(int64_t)y * ld + x] != 0) != (invert != 0);
        const unsigned long long m = __ballot(fg);
        if (lane == 0) rowmask[r] = m;
        const unsigned long long below = ~m & ((1ull << lane) - 1ull);     // background lanes left of this one
        const int start = below ? 64 - __clzll((long long)below) : 0;
        lab[r * kTile + lane] = fg ? r * kTile + start : -1;
    }
    __syncthreads();

    // join to the row above.  A pixel whose left neighbour is foreground leaves to it what that neighbour also touches.
    for (int r = wave; r < kTile; r += 4) {
        if (r == 0) continue;
        const unsigned long long m = rowmask[r], up = rowmask[r - 1];
        if (!((m >> lane) & 1ull)) continue;
        const bool u = (up >> lane) & 1ull;
        const bool ul = lane > 0 && ((up >> (lane - 1)) & 1ull);
        const bool ur = lane < 63 && ((up >> (lane + 1)) & 1ull);
        const bool left = lane > 0 && ((m >> (lane - 1)) & 1ull);
        const int p = r * kTile + lane, q = p - kTile;
        if (conn8) {
            if (u) {
                if (!left) uf_union(lab, p, q);
            } else {
                if (ul && !left) uf_union(lab, p, q - 1);
                if (ur) uf_union(lab, p, q + 1);
            }
        } else if (u && !(left && ul)) {
            uf_union(lab, p, q);
        }
    }
    __syncthreads();

    for (int r = wave; r < kTile; r += 4) {
        const int y = ty0 + r;
        if (y >= h || x >= w) continue;
        const int p = r * kTile + lane;
        int root = -1;
        if (lab[p] >= 0) {
            const int lr = uf_find(lab, p);
            root = (ty0 + lr / kTile) * w + tx0 + lr % kTile;
        }
        parent[(int64_t)y * w + x] = root;
    }
}

__global__ __launch_bounds__(256) void border_merge_kernel(int *__restrict__ parent, int h, int w, int conn8, int64_t n_rows,
                                                           int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (i < n_rows) {   // first row of a tile below the top: up, up-left, up-right lie across the edge
        const int y = (int)(i / w + 1) * kTile, x = (int)(i % w);
        const int p = y * w + x, q = p - w;
        if (ld_relaxed(parent + p) < 0) return;
        if (ld_relaxed(parent + q) >= 0) {
            uf_union(parent, p, q);      // up-left and up-right hang on `up` by their own row
        } else if (conn8) {
            if (x > 0 && ld_relaxed(parent + q - 1) >= 0) uf_union(parent, p, q - 1);
            if (x < w - 1 && ld_relaxed(parent + q + 1) >= 0) uf_union(parent, p, q + 1);
        }
        return;
    }
    // first column of a tile right of the left edge: left, and the two diagonals that cross this edge alone
    const int64_t j = i - n_rows;
    const int x = (int)(j / h + 1) * kTile, y = (int)(j % h);
    const int p = y * w + x;
    const bool here = ld_relaxed(parent + p) >= 0, left = ld_relaxed(parent + p - 1) >= 0;
    if (here && left) uf_union(parent, p, p - 1);
    if (conn8 && y > 0 && y % kTile != 0) {      // (on a tile's first row the row pass has both diagonals)
        const int q = p - w;
        if (here && !left && ld_relaxed(parent + q - 1) >= 0) uf_union(parent, p, q - 1);
        if (left && !here && ld_relaxed(parent + q) >= 0) uf_union(parent, p - 1, q);
    }
}

// ---- regions of equal value (K18): stages 1 and 2 where every join also tests value(p) == value(q) ---------------------
// The shortcuts of the binary kernels hold once "foreground" reads "has this pixel's value": two horizontal neighbours
// of one value are one run, so what a same-valued left neighbour also touches in the row above is left to it.
template <typename T>
__global__ __launch_bounds__(256) void tile_label_valued_kernel(const T *__restrict__ src, int64_t ld, int h, int w, int conn8,
                                                                int *__restrict__ parent, int tiles_x, int64_t ntiles)
{
    __shared__ int lab[kTile * kTile];
    __shared__ T val[kTile * kTile];
    const int64_t tile = xcd_contiguous(blockIdx.x, ntiles);
    if (tile >= ntiles) return;
    const int ty0 = (int)(tile / tiles_x) * kTile, tx0 = (int)(tile % tiles_x) * kTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = tx0 + lane;

    // run starts: a non-zero lane whose left neighbour holds another value; a lane's run begins at the highest start
    // at or below it
    for (int r = wave; r < kTile; r += 4) {
        const int y = ty0 + r;
        T v = 0;
        if (y < h && x < w) v = src[(int64_t)y * ld + x];
        val[r * kTile + lane] = v;
        const long long wide = (long long)v;               // (every label dtype widens without two values meeting)
        const long long left = __shfl_up(wide, 1);
        const bool fg = v != 0;
        const unsigned long long starts = __ballot(fg && (lane == 0 || left != wide));
        const unsigned long long upto = starts & (lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull);
        lab[r * kTile + lane] = fg ? r * kTile + 63 - __builtin_clzll(upto | 1ull) : -1;   // (a foreground lane: upto != 0)
    }
    __syncthreads();

    for (int r = wave; r < kTile; r += 4) {
        if (r == 0) continue;
        const int p = r * kTile + lane, q = p - kTile;
        const T v = val[p];
        if (v == 0) continue;
        const bool u = val[q] == v;
        const bool ul = lane > 0 && val[q - 1] == v;
        const bool ur = lane < 63 && val[q + 1] == v;
        const bool left = lane > 0 && val[p - 1] == v;
        if (conn8) {
            if (u) {
                if (!left) uf_union(lab, p, q);
            } else {
                if (ul && !left) uf_union(lab, p, q - 1);
                if (ur) uf_union(lab, p, q + 1);
            }
        } else if (u && !(left && ul)) {
            uf_union(lab, p, q);
        }
    }
    __syncthreads();

    for (int r = wave; r < kTile; r += 4) {
        const int y = ty0 + r;
        if (y >= h || x >= w) continue;
        const int p = r * kTile + lane;
        int root = -1;
        if (lab[p] >= 0) {
            const int lr = uf_find(lab, p);
            root = (ty0 + lr / kTile) * w + tx0 + lr % kTile;
        }
        parent[(int64_t)y * w + x] = root;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void border_merge_valued_kernel(const T *__restrict__ src, int64_t ld, int *__restrict__ parent,
                                                                  int h, int w, int conn8, int64_t n_rows, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (i < n_rows) {   // first row of a tile below the top
        const int y = (int)(i / w + 1) * kTile, x = (int)(i % w);
        const int p = y * w + x, q = p - w;
        const T *row = src + (int64_t)y * ld, *above = row - ld;
        const T v = row[x];
        if (v == 0) return;
        if (above[x] == v) {
            uf_union(parent, p, q);      // an up-left or up-right of this value is in `up`'s run
        } else if (conn8) {
            if (x > 0 && above[x - 1] == v) uf_union(parent, p, q - 1);
            if (x < w - 1 && above[x + 1] == v) uf_union(parent, p, q + 1);
        }
        return;
    }
    // first column of a tile right of the left edge
    const int64_t j = i - n_rows;
    const int x = (int)(j / h + 1) * kTile, y = (int)(j % h);
    const int p = y * w + x;
    const T *row = src + (int64_t)y * ld;
    const T here = row[x], left = row[x - 1];
    if (here != 0 && here == left) uf_union(parent, p, p - 1);
    if (conn8 && y > 0 && y % kTile != 0 && here != left) {      // (equal: each reaches the other's diagonal through it)
        const T *above = row - ld;
        if (here != 0 && above[x - 1] == here) uf_union(parent, p, p - w - 1);
        if (left != 0 && above[x] == left) uf_union(parent, p - 1, p - w);
    }
}

// roots of the chunk's pixels, in raster order: this thread's is number `rank` of `count`
__device__ __forceinline__ void chunk_rank(bool is_root, int *wave_counts, int &rank, int &count)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(is_root);
    if (lane == 0) wave_counts[wave] = __popcll(m);
    __syncthreads();
    rank = __popcll(m & ((1ull << lane) - 1ull));
    count = 0;
    for (int v = 0; v < kChunk / 64; v++) {
        if (v < wave) rank += wave_counts[v];
        count += wave_counts[v];
    }
}

__global__ __launch_bounds__(kChunk) void flatten_count_kernel(int *parent, int total, unsigned *counts)
{
    __shared__ int wave_counts[kChunk / 64];
    const int64_t e = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    bool is_root = false;
    if (e < total) {
        const int p = (int)e, q = ld_relaxed(parent + p);
        if (q >= 0) {
            const int r = q == p ? p : uf_find(parent, q);
            // an ancestor replaced by the root while other workgroups walk the array: a reader of either finds the root
            if (r != q) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            is_root = r == p;
        }
    }
    int rank, count;
    chunk_rank(is_root, wave_counts, rank, count);
    if (threadIdx.x == 0) counts[blockIdx.x] = (unsigned)count;
}

// counts[0 .. n) -> exclusive prefix sums in place, the total to *n_out.  One workgroup; thread t owns a run of `per` counts.
__global__ __launch_bounds__(1024) void ccl_scan_kernel(unsigned *__restrict__ counts, int64_t n, int32_t *__restrict__ n_out)
{
    __shared__ unsigned sums[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    unsigned s = 0;
    for (int64_t i = lo; i < hi; i++) s += counts[i];
    sums[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned add = t >= d ? sums[t - d] : 0u;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    unsigned run = sums[t] - s;
    for (int64_t i = lo; i < hi; i++) {
        const unsigned c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (t == 1023) *n_out = (int32_t)sums[1023];
}

__global__ __launch_bounds__(kChunk) void rank_roots_kernel(const int *__restrict__ parent, int total, int w,
                                                            const unsigned *__restrict__ offsets, int32_t *__restrict__ labels,
                                                            int64_t ldo)
{
    __shared__ int wave_counts[kChunk / 64];
    const int64_t e = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    const bool is_root = e < total && parent[e] == (int)e;
    int rank, count;
    chunk_rank(is_root, wave_counts, rank, count);
    if (is_root) labels[(e / w) * ldo + e % w] = (int32_t)(offsets[blockIdx.x] + (unsigned)rank + 1u);
}

// A workgroup takes kFinishSpan consecutive pixels.  The label of its first pixel (often the background, or a component
// that covers the span) is counted in registers and LDS and reaches the area table as ONE add per workgroup; every other
// label costs one add per run of equal labels among a wave's consecutive pixels.
constexpr int kFinishSpan = 16 * kChunk;

__global__ __launch_bounds__(kChunk) void finish_labels_kernel(const int *__restrict__ parent, int total, int w,
                                                               int32_t *__restrict__ labels, int64_t ldo,
                                                               int32_t *__restrict__ areas, int64_t capacity)
{
    __shared__ int span_count;
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t)blockIdx.x * kFinishSpan;
    if (threadIdx.x == 0) span_count = 0;
    int32_t first = 0;                                   // (roots were written by rank_roots_kernel)
    {
        const int r = parent[e0];                        // e0 < total: the grid has no empty workgroup
        if (r >= 0) first = labels[(int64_t)(r / w) * ldo + r % w];
    }
    int mine = 0;                                        // the wave's pixels that carry `first` (same in every lane)
    for (int it = 0; it < kFinishSpan / kChunk; it++) {
        const int64_t e = e0 + (int64_t)it * kChunk + threadIdx.x;
        const bool valid = e < total;
        int32_t lab = 0;
        if (valid) {
            const int r = parent[e];
            if (r >= 0) lab = labels[(int64_t)(r / w) * ldo + r % w];
            if (r != (int)e) labels[(e / w) * ldo + e % w] = lab;
        }
        const bool is_first = valid && lab == first;
        const unsigned long long firsts = __ballot(is_first);
        mine += __popcll(firsts);
        const int32_t prev = __shfl_up(lab, 1);
        const bool leader = valid && !is_first && (lane == 0 || prev != lab);
        // a run ends at the next leader, at a pixel of `first` or past the image
        const unsigned long long stops = __ballot(leader) | firsts | ~__ballot(valid);
        if (leader) {
            const unsigned long long above = lane == 63 ? 0ull : stops >> (lane + 1);
            const int run = above ? __ffsll((long long)above) : 64 - lane;
            if (lab < capacity) atomicAdd(areas + lab, run);
        }
    }
    __syncthreads();
    if (lane == 0 && mine) atomicAdd(&span_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && span_count && first < capacity) atomicAdd(areas + first, span_count);
}

__global__ __launch_bounds__(256) void select_fill_kernel(const uint8_t *__restrict__ fg, int64_t ldf,
                                                          const int32_t *__restrict__ labels, int64_t ldl,
                                                          const int32_t *__restrict__ areas, int64_t capacity, int h, int w,
                                                          int64_t below, uint8_t *__restrict__ out, int64_t ldo)
{
    const int64_t total = (int64_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t y = e / w, x = e - y * w;
        const int32_t lab = labels[y * ldl + x];
        bool on = fg[y * ldf + x] != 0;
        if (!on && lab > 0 && lab < capacity) on = areas[lab] < below;
        out[y * ldo + x] = on ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void select_keep_kernel(const int32_t *__restrict__ labels, int64_t ldl,
                                                          const int32_t *__restrict__ areas, int64_t capacity, int h, int w,
                                                          int64_t lo, int64_t hi, int32_t *__restrict__ out, int64_t ldo)
{
    const int64_t total = (int64_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t y = e / w, x = e - y * w;
        const int32_t lab = labels[y * ldl + x];
        bool keep = false;
        if (lab > 0 && lab < capacity) {
            const int64_t a = areas[lab];
            keep = lo <= a && a <= hi;
        }
        out[y * ldo + x] = keep ? lab : 0;
    }
}

#pragma clang fp contract(off)

// the comparisons widen float32 exactly: what numpy compares in binary32 compares the same in binary64
template <typename T>
__global__ __launch_bounds__(256) void binarize_kernel(const T *__restrict__ plane, const T *__restrict__ local, int64_t total,
                                                       int w, int mode, double level, uint8_t *__restrict__ out, int64_t ldo)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const double v = (double)plane[e];
        bool on;
        if (mode == PXSOM_BIN_LOCAL) on = v > (double)local[e];
        else if (mode == PXSOM_BIN_LEVEL) on = !(v < level) && v > 0.0;
        else on = v > 0.0;
        const int64_t y = e / w;
        out[y * ldo + (e - y * w)] = on ? 1 : 0;
    }
}

#pragma clang fp contract(fast)

inline int64_t ccl_chunks(int64_t total) { return (total + kChunk - 1) / kChunk; }

}  // namespace

PXSOM_EXPORT size_t pxsom_label_components_workspace_bytes(int h, int w)
{
    if (h < 1 || w < 1 || (int64_t)h * w > INT32_MAX) return 0;
    const int64_t total = (int64_t)h * w;
    return pxsom::align_up((size_t)total * sizeof(int), 256) + pxsom::align_up((size_t)ccl_chunks(total) * sizeof(unsigned), 256);
}

PXSOM_EXPORT int pxsom_label_components(const uint8_t *fg_dev, int h, int w, int64_t ld, int connectivity, int invert,
                                        int32_t *labels_dev, int64_t ldo, int32_t *n_dev, int32_t *areas_dev,
                                        int64_t capacity, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (h < 1 || w < 1 || ld < w || ldo < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_components: bad size or stride (h=%d w=%d ld=%lld ldo=%lld)", h, w,
                           (long long)ld, (long long)ldo);
    if (connectivity != 1 && connectivity != 2)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_components: connectivity %d is not 1 or 2", connectivity);
    if ((invert != 0 && invert != 1) || capacity < 1)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_components: bad invert flag or capacity");
    if (!fg_dev || !labels_dev || !n_dev || !areas_dev || !workspace_dev)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_components: null pointer");
    if ((int64_t)h * w > INT32_MAX)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_label_components: %d x %d pixels are beyond int32", h, w);
    if (workspace_bytes < pxsom_label_components_workspace_bytes(h, w))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_components: workspace of %zu bytes, %zu needed", workspace_bytes,
                           pxsom_label_components_workspace_bytes(h, w));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int total = h * w;
    int *parent = static_cast<int *>(workspace_dev);
    unsigned *counts = reinterpret_cast<unsigned *>(static_cast<char *>(workspace_dev) + pxsom::align_up((size_t)total * sizeof(int), 256));
    const int64_t chunks = ccl_chunks(total);
    const int tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    const int64_t ntiles = (int64_t)tiles_x * tiles_y;

    PXSOM_HIP_TRY(hipMemsetAsync(areas_dev, 0, (size_t)capacity * sizeof(int32_t), st));
    hipLaunchKernelGGL(tile_label_kernel, dim3((unsigned)((ntiles + 7) / 8 * 8)), dim3(256), 0, st, fg_dev, ld, h, w, invert,
                       connectivity == 2 ? 1 : 0, parent, tiles_x, ntiles);
    const int64_t n_rows = (int64_t)(tiles_y - 1) * w, n_cols = (int64_t)(tiles_x - 1) * h;
    if (n_rows + n_cols > 0)
        hipLaunchKernelGGL(border_merge_kernel, dim3((unsigned)((n_rows + n_cols + 255) / 256)), dim3(256), 0, st, parent, h, w,
                           connectivity == 2 ? 1 : 0, n_rows, n_rows + n_cols);
    hipLaunchKernelGGL(flatten_count_kernel, dim3((unsigned)chunks), dim3(kChunk), 0, st, parent, total, counts);
    hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(1024), 0, st, counts, chunks, n_dev);
    hipLaunchKernelGGL(rank_roots_kernel, dim3((unsigned)chunks), dim3(kChunk), 0, st, parent, total, w, counts, labels_dev, ldo);
    hipLaunchKernelGGL(finish_labels_kernel, dim3((unsigned)(((int64_t)total + kFinishSpan - 1) / kFinishSpan)), dim3(kChunk), 0, st, parent, total, w, labels_dev, ldo,
                       areas_dev, capacity);
    PXSOM_LAUNCH_CHECK("pxsom_label_components kernels");
    return PXSOM_OK;
}

PXSOM_EXPORT size_t pxsom_label_regions_workspace_bytes(int h, int w) { return pxsom_label_components_workspace_bytes(h, w); }

PXSOM_EXPORT int pxsom_label_regions(const void *seg_dev, int dtype, int h, int w, int64_t ld, int connectivity,
                                     int32_t *labels_dev, int64_t ldo, int32_t *n_dev, int32_t *areas_dev, int64_t capacity,
                                     void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (h < 1 || w < 1 || ld < w || ldo < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_regions: bad size or stride (h=%d w=%d ld=%lld ldo=%lld)", h, w,
                           (long long)ld, (long long)ldo);
    if (!pxsom::is_label_dtype(dtype))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_regions: dtype code %d is not a label dtype (%d .. %d)", dtype,
                           PXSOM_SEG_U8, PXSOM_SEG_I64);
    if (connectivity != 1 && connectivity != 2)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_regions: connectivity %d is not 1 or 2", connectivity);
    if (capacity < 1)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_regions: capacity %lld is below 1", (long long)capacity);
    if (!seg_dev || !labels_dev || !n_dev || !areas_dev || !workspace_dev)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_regions: null pointer");
    if ((int64_t)h * w > INT32_MAX)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_label_regions: %d x %d pixels are beyond int32", h, w);
    if (workspace_bytes < pxsom_label_regions_workspace_bytes(h, w))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_label_regions: workspace of %zu bytes, %zu needed", workspace_bytes,
                           pxsom_label_regions_workspace_bytes(h, w));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int total = h * w;
    int *parent = static_cast<int *>(workspace_dev);
    unsigned *counts = reinterpret_cast<unsigned *>(static_cast<char *>(workspace_dev) + pxsom::align_up((size_t)total * sizeof(int), 256));
    const int64_t chunks = ccl_chunks(total);
    const int tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    const int64_t ntiles = (int64_t)tiles_x * tiles_y;
    const int conn8 = connectivity == 2 ? 1 : 0;
    const int64_t n_rows = (int64_t)(tiles_y - 1) * w, n_cols = (int64_t)(tiles_x - 1) * h;

    PXSOM_HIP_TRY(hipMemsetAsync(areas_dev, 0, (size_t)capacity * sizeof(int32_t), st));
    pxsom::dispatch_label(dtype, [&](auto tag) {
        using T = decltype(tag);
        const T *src = static_cast<const T *>(seg_dev);
        hipLaunchKernelGGL(tile_label_valued_kernel<T>, dim3((unsigned)((ntiles + 7) / 8 * 8)), dim3(256), 0, st, src, ld, h, w,
                           conn8, parent, tiles_x, ntiles);
        if (n_rows + n_cols > 0)
            hipLaunchKernelGGL(border_merge_valued_kernel<T>, dim3((unsigned)((n_rows + n_cols + 255) / 256)), dim3(256), 0, st,
                               src, ld, parent, h, w, conn8, n_rows, n_rows + n_cols);
        return 0;
    });
    hipLaunchKernelGGL(flatten_count_kernel, dim3((unsigned)chunks), dim3(kChunk), 0, st, parent, total, counts);
    hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(1024), 0, st, counts, chunks, n_dev);
    hipLaunchKernelGGL(rank_roots_kernel, dim3((unsigned)chunks), dim3(kChunk), 0, st, parent, total, w, counts, labels_dev, ldo);
    hipLaunchKernelGGL(finish_labels_kernel, dim3((unsigned)(((int64_t)total + kFinishSpan - 1) / kFinishSpan)), dim3(kChunk), 0, st,
                       parent, total, w, labels_dev, ldo, areas_dev, capacity);
    PXSOM_LAUNCH_CHECK("pxsom_label_regions kernels");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_components_select(int mode, const uint8_t *fg_dev, int64_t ldf, const int32_t *labels_dev, int64_t ldl,
                                         const int32_t *areas_dev, int64_t capacity, int h, int w, int64_t area_lo,
                                         int64_t area_hi, void *out_dev, int64_t ldo, void *stream)
{
    if (mode != PXSOM_SELECT_FILL && mode != PXSOM_SELECT_KEEP)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_components_select: mode %d", mode);
    if (h < 1 || w < 1 || ldl < w || ldo < w || capacity < 1 || (mode == PXSOM_SELECT_FILL && ldf < w))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_components_select: bad size, stride or capacity");
    if (!labels_dev || !areas_dev || !out_dev || (mode == PXSOM_SELECT_FILL && !fg_dev))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_components_select: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int grid = pxsom::flat_grid((int64_t)h * w);
    if (mode == PXSOM_SELECT_FILL)
        hipLaunchKernelGGL(select_fill_kernel, dim3(grid), dim3(256), 0, st, fg_dev, ldf, labels_dev, ldl, areas_dev, capacity, h, w,
                           area_hi, static_cast<uint8_t *>(out_dev), ldo);
    else
        hipLaunchKernelGGL(select_keep_kernel, dim3(grid), dim3(256), 0, st, labels_dev, ldl, areas_dev, capacity, h, w, area_lo,
                           area_hi, static_cast<int32_t *>(out_dev), ldo);
    PXSOM_LAUNCH_CHECK("pxsom_components_select kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_binarize_plane(const void *plane_dev, int dtype, int h, int w, int mode, double level,
                                      const void *local_dev, uint8_t *out_dev, int64_t ldo, void *stream)
{
    if (!plane_dev || !out_dev || h < 1 || w < 1 || ldo < w || (dtype != PXSOM_SEG_F32 && dtype != PXSOM_SEG_F64))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_binarize_plane: bad arguments");
    if ((mode != PXSOM_BIN_POSITIVE && mode != PXSOM_BIN_LEVEL && mode != PXSOM_BIN_LOCAL) || (mode == PXSOM_BIN_LOCAL && !local_dev))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_binarize_plane: bad mode %d or no local plane", mode);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t total = (int64_t)h * w;
    const int grid = pxsom::flat_grid(total);
    if (dtype == PXSOM_SEG_F32)
        hipLaunchKernelGGL(binarize_kernel<float>, dim3(grid), dim3(256), 0, st, static_cast<const float *>(plane_dev),
                           static_cast<const float *>(local_dev), total, w, mode, level, out_dev, ldo);
    else
        hipLaunchKernelGGL(binarize_kernel<double>, dim3(grid), dim3(256), 0, st, static_cast<const double *>(plane_dev),
                           static_cast<const double *>(local_dev), total, w, mode, level, out_dev, ldo);
    PXSOM_LAUNCH_CHECK("binarize_kernel");
    return PXSOM_OK;
}
