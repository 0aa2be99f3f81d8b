// pxsom_merge.hip -- merging ez_seg object masks into the cell segmentation on gfx950 (K18): the passes around the
// labelling of pxsom_ccl.hip (pxsom_label_regions).
//
//   pxsom_pair_overlaps    the sorted list (a, b, pixels) of the label pairs that two int32 label planes share
//   pxsom_merge_apply      the write pass: merged and remaining planes from the winner / removed tables of the cells
//
// pxsom_pair_overlaps never builds the n_a x n_b table.  A "run" is a stretch of pixels of one pair (a != 0, b != 0,
// both within their label ranges) inside one row and inside one aligned group of 64 pixels of the flat raster order
// (a wave's pixels): a pure function of the image.
//   1. count_runs_kernel    counts the runs (a ballot per wave, one int32 atomic per wave): no more distinct pairs than runs
//   2. insert_runs_kernel   only if runs <= capacity: one insertion per run, with its length, into an open-addressing table
//                           of >= 2 * capacity slots (64-bit compare-and-swap on the key, int32 add on the count) --
//                           the table is at most half full by construction, whatever the labels are
//   3. bitonic_step_kernel  sorts the slots by key (a << 32 | b, empty slots last): the order no longer depends on which
//                           insertion came first
//   4. emit_pairs_kernel    writes the occupied slots as rows and the count
// Integer atomics only: the same input gives the same bytes on every run.
#include "pxsom_common.h"
#include "pxsom_pairtable.h"
#include "pxsom_plane.h"

namespace {

// the pair of pixel e as a table key, 0 when either label is 0 or outside 1 .. n
__device__ __forceinline__ unsigned long long pair_key(const int32_t *__restrict__ a, int64_t lda, const int32_t *__restrict__ b,
                                                       int64_t ldb, int w, int64_t e, int32_t n_a, int32_t n_b)
{
    const int64_t y = e / w, x = e - y * w;
    const int32_t va = a[y * lda + x], vb = b[y * ldb + x];
    if (va < 1 || va > n_a || vb < 1 || vb > n_b) return 0ull;
    return ((unsigned long long)(uint32_t)va << 32) | (uint32_t)vb;
}

// does a run begin at pixel e (lane e % 64 of its wave)?  `key` is e's, non-zero
__device__ __forceinline__ bool run_begins(const int32_t *__restrict__ a, int64_t lda, const int32_t *__restrict__ b, int64_t ldb,
                                           int w, int64_t e, int32_t n_a, int32_t n_b, unsigned long long key)
{
    if ((e & 63) == 0 || e % w == 0) return true;
    return pair_key(a, lda, b, ldb, w, e - 1, n_a, n_b) != key;
}

__global__ __launch_bounds__(256) void count_runs_kernel(const int32_t *__restrict__ a, int64_t lda, const int32_t *__restrict__ b,
                                                         int64_t ldb, int w, int64_t total, int32_t n_a, int32_t n_b,
                                                         int32_t *__restrict__ runs)
{
    const int64_t e0 = (int64_t)blockIdx.x * kRunSpan;
    int mine = 0;                                          // the wave's runs (same in every lane)
    for (int it = 0; it < kRunSpan / 256; it++) {
        const int64_t e = e0 + (int64_t)it * 256 + threadIdx.x;
        bool begins = false;
        if (e < total) {
            const unsigned long long key = pair_key(a, lda, b, ldb, w, e, n_a, n_b);
            begins = key != 0ull && run_begins(a, lda, b, ldb, w, e, n_a, n_b, key);
        }
        mine += __popcll(__ballot(begins));
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(runs, mine);
}

__global__ __launch_bounds__(256) void insert_runs_kernel(const int32_t *__restrict__ a, int64_t lda, const int32_t *__restrict__ b,
                                                          int64_t ldb, int w, int64_t total, int32_t n_a, int32_t n_b,
                                                          const int32_t *__restrict__ runs, int64_t capacity,
                                                          unsigned long long *__restrict__ keys, int32_t *__restrict__ counts,
                                                          int64_t slots, int32_t *__restrict__ n_pairs)
{
    if ((int64_t)*runs > capacity) return;                 // (uniform) more insertions than the table was sized for: none is made
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t)blockIdx.x * kRunSpan;
    for (int it = 0; it < kRunSpan / 256; it++) {
        const int64_t e = e0 + (int64_t)it * 256 + threadIdx.x;
        unsigned long long key = 0ull;
        if (e < total) key = pair_key(a, lda, b, ldb, w, e, n_a, n_b);
        const bool begins = key != 0ull && run_begins(a, lda, b, ldb, w, e, n_a, n_b, key);
        // a run ends at the next beginning, at a pixel without a pair or past the image
        const unsigned long long stops = __ballot(begins || key == 0ull);
        if (!begins) continue;
        const unsigned long long above = lane == 63 ? 0ull : stops >> (lane + 1);
        const int run = above ? __ffsll((long long)above) : 64 - lane;
        table_add(keys, counts, slots, key, run, n_pairs);
    }
}

// one compare-exchange step of the bitonic network over `slots` (a power of two) entries: ascending by key
__global__ __launch_bounds__(256) void bitonic_step_kernel(unsigned long long *__restrict__ keys, int32_t *__restrict__ counts,
                                                           int64_t slots, int64_t k, int64_t j)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < slots / 2; t += (int64_t)gridDim.x * 256) {
        const int64_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;     // the pair (i, i ^ j) with bit j clear in i
        const unsigned long long klo = keys[lo], khi = keys[hi];
        const bool ascending = (lo & k) == 0;
        if ((klo > khi) == ascending && klo != khi) {
            keys[lo] = khi;
            keys[hi] = klo;
            const int32_t c = counts[lo];
            counts[lo] = counts[hi];
            counts[hi] = c;
        }
    }
}

__global__ __launch_bounds__(256) void emit_pairs_kernel(const unsigned long long *__restrict__ keys,
                                                         const int32_t *__restrict__ counts, int64_t slots, int64_t capacity,
                                                         int32_t *__restrict__ pairs, int32_t *__restrict__ n_dev)
{
    const bool fits = (int64_t)n_dev[1] <= capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0 && !fits) n_dev[0] = -1;
    if (!fits) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots && i < capacity; i += (int64_t)gridDim.x * 256) {
        const unsigned long long key = keys[i];
        if (key == kEmpty) continue;                       // (sorted: the occupied slots come first)
        pairs[3 * i] = (int32_t)(key >> 32);
        pairs[3 * i + 1] = (int32_t)(key & 0xffffffffull);
        pairs[3 * i + 2] = counts[i];
    }
}

__global__ __launch_bounds__(256) void merge_apply_kernel(const int32_t *__restrict__ a, int64_t lda, const int32_t *__restrict__ b,
                                                          int64_t ldb, int h, int w, const int32_t *__restrict__ winner,
                                                          const int32_t *__restrict__ removed, int64_t table,
                                                          int32_t *__restrict__ merged, int64_t ldm,
                                                          int32_t *__restrict__ remaining, int64_t ldr)
{
    const int64_t total = (int64_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t y = e / w, x = e - y * w;
        const int32_t vb = b[y * ldb + x];
        int32_t win = 0, gone = 0;
        if (vb >= 0 && vb < table) {
            win = winner[vb];
            gone = removed[vb];
        }
        merged[y * ldm + x] = win != 0 ? win : a[y * lda + x];
        remaining[y * ldr + x] = gone ? 0 : vb;
    }
}

}  // namespace

PXSOM_EXPORT size_t pxsom_pair_overlaps_workspace_bytes(int64_t capacity)
{
    if (capacity < 1 || capacity > kMaxPairCapacity) return 0;
    return pair_table_bytes(capacity);
}

PXSOM_EXPORT int pxsom_pair_overlaps(const int32_t *a_dev, int64_t lda, const int32_t *b_dev, int64_t ldb, int h, int w,
                                     int32_t n_a, int32_t n_b, int32_t *pairs_dev, int64_t capacity, int32_t *n_dev,
                                     void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (h < 1 || w < 1 || lda < w || ldb < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_pair_overlaps: bad size or stride (h=%d w=%d lda=%lld ldb=%lld)", h, w,
                           (long long)lda, (long long)ldb);
    if ((int64_t)h * w > INT32_MAX)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_pair_overlaps: %d x %d pixels are beyond the limit %d", h, w, INT32_MAX);
    if (n_a < 0 || n_b < 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_pair_overlaps: label counts %d, %d are below 0", n_a, n_b);
    if (!a_dev || !b_dev || !n_dev)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_pair_overlaps: null pointer");
    const bool count_only = pairs_dev == nullptr;
    if (!count_only) {
        if (capacity < 1 || capacity > kMaxPairCapacity)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_pair_overlaps: capacity %lld is outside 1 .. %lld", (long long)capacity,
                               (long long)kMaxPairCapacity);
        if (!workspace_dev || workspace_bytes < pxsom_pair_overlaps_workspace_bytes(capacity))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_pair_overlaps: workspace of %zu bytes, %zu needed", workspace_bytes,
                               pxsom_pair_overlaps_workspace_bytes(capacity));
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t total = (int64_t)h * w;
    const unsigned spans = (unsigned)((total + kRunSpan - 1) / kRunSpan);

    PXSOM_HIP_TRY(hipMemsetAsync(n_dev, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(count_runs_kernel, dim3(spans), dim3(256), 0, st, a_dev, lda, b_dev, ldb, w, total, n_a, n_b, n_dev + 1);
    if (!count_only) {
        const int64_t slots = pair_slots(capacity);
        unsigned long long *keys = static_cast<unsigned long long *>(workspace_dev);
        int32_t *counts = pair_table_counts(keys, slots);
        PXSOM_HIP_TRY(hipMemsetAsync(keys, 0xFF, (size_t)slots * sizeof(unsigned long long), st));    // every slot kEmpty
        PXSOM_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)slots * sizeof(int32_t), st));
        hipLaunchKernelGGL(insert_runs_kernel, dim3(spans), dim3(256), 0, st, a_dev, lda, b_dev, ldb, w, total, n_a, n_b,
                           n_dev + 1, capacity, keys, counts, slots, n_dev);
        const int grid = pxsom::flat_grid(slots / 2);
        for (int64_t k = 2; k <= slots; k <<= 1)
            for (int64_t j = k >> 1; j > 0; j >>= 1)
                hipLaunchKernelGGL(bitonic_step_kernel, dim3(grid), dim3(256), 0, st, keys, counts, slots, k, j);
        hipLaunchKernelGGL(emit_pairs_kernel, dim3(pxsom::flat_grid(std::min(slots, capacity))), dim3(256), 0, st, keys, counts,
                           slots, capacity, pairs_dev, n_dev);
    }
    PXSOM_LAUNCH_CHECK("pxsom_pair_overlaps kernels");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_merge_apply(const int32_t *a_dev, int64_t lda, const int32_t *b_dev, int64_t ldb, int h, int w,
                                   const int32_t *winner_dev, const int32_t *removed_dev, int64_t table, int32_t *merged_dev,
                                   int64_t ldm, int32_t *remaining_dev, int64_t ldr, void *stream)
{
    if (h < 1 || w < 1 || lda < w || ldb < w || ldm < w || ldr < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_merge_apply: bad size or stride (h=%d w=%d, strides %lld %lld %lld %lld)", h,
                           w, (long long)lda, (long long)ldb, (long long)ldm, (long long)ldr);
    if (table < 1 || table > (int64_t)INT32_MAX + 1)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_merge_apply: %lld table entries are outside 1 .. %lld", (long long)table,
                           (long long)INT32_MAX + 1);
    if (!a_dev || !b_dev || !winner_dev || !removed_dev || !merged_dev || !remaining_dev)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_merge_apply: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(merge_apply_kernel, dim3(pxsom::flat_grid((int64_t)h * w)), dim3(256), 0, st, a_dev, lda, b_dev, ldb, h, w,
                       winner_dev, removed_dev, table, merged_dev, ldm, remaining_dev, ldr);
    PXSOM_LAUNCH_CHECK("merge_apply_kernel");
    return PXSOM_OK;
}
