// pxsom_nucsplit.hip -- splitting nuclei that reach past their cell on gfx950 (K21): the two device passes of
// segmentation_utils.split_large_nuclei (the choice between them is made on the host over per-cell tables).
//
//   pxsom_nuclear_overlaps   per nucleus its pixels, per cell the nucleus with the most pixels inside it and that count
//   pxsom_split_apply        the write pass: the nuclear plane with the chosen (cell, nucleus) overlaps renumbered
//
// Both planes are read in their own label dtype with their own row stride; a label names a cell (a nucleus) through the
// K10 key table (pxsom_keytable.h: a dense LUT or a binary search, identical results), 0 and every label outside the
// table are no cell (no nucleus).  No index planes are written and no n_cells x n_nuc table is built:
//   1. count_kernel    counts the RUNS of the image: stretches of one (cell label, nucleus label) pair, both non-zero,
//                      inside a row and inside an aligned group of 64 pixels (a ballot per wave, one int32 atomic per wave)
//   2. init_kernel     zeroes the areas and the per-cell maxima
//   3. insert_kernel   one table insertion per run whose labels are both in their key table (pxsom_pairtable.h), keyed
//                      (cell index << 32 | nucleus index), and one 64-bit add to the nucleus's area per stretch of equal
//                      nuclear labels in the wave's 64 pixels
//   4. sweep_kernel    every occupied slot: a 64-bit atomicMax on its cell's word with (pixels << 32 | ~nucleus index) --
//                      the maximum does not depend on the order, and the complement lets the smaller nucleus win a tie
//   5. finish_kernel   unpacks the maxima into best_dev and writes the pair count
// Kernels 2 - 5 do nothing when the runs exceed the capacity the table was sized for (n_dev[0] = -1).  Integer atomics
// only: the same input gives the same bytes on every run and for every grid.
#include <climits>

#include "pxsom_common.h"
#include "pxsom_keytable.h"
#include "pxsom_pairtable.h"

namespace {

// one label plane: the element of pixel (y, x) is at y * ld + x, of a PXSOM_SEG_U8 .. PXSOM_SEG_I64 dtype
struct LabelPlane {
    const void *p;
    int64_t ld;
    int dtype;
};

// (the dtype is uniform over the launch: a scalar branch)
__device__ __forceinline__ int64_t load_label(const LabelPlane &s, int64_t at)
{
    switch (s.dtype) {
    case PXSOM_SEG_U8: return (int64_t) static_cast<const uint8_t *>(s.p)[at];
    case PXSOM_SEG_I16: return (int64_t) static_cast<const int16_t *>(s.p)[at];
    case PXSOM_SEG_U16: return (int64_t) static_cast<const uint16_t *>(s.p)[at];
    case PXSOM_SEG_I32: return (int64_t) static_cast<const int32_t *>(s.p)[at];
    case PXSOM_SEG_U32: return (int64_t) static_cast<const uint32_t *>(s.p)[at];
    default: return static_cast<const int64_t *>(s.p)[at];
    }
}

__device__ __forceinline__ void store_label(void *p, int dtype, int64_t at, int64_t v)
{
    switch (dtype) {
    case PXSOM_SEG_U8: static_cast<uint8_t *>(p)[at] = (uint8_t)v; break;
    case PXSOM_SEG_I16: static_cast<int16_t *>(p)[at] = (int16_t)v; break;
    case PXSOM_SEG_U16: static_cast<uint16_t *>(p)[at] = (uint16_t)v; break;
    case PXSOM_SEG_I32: static_cast<int32_t *>(p)[at] = (int32_t)v; break;
    case PXSOM_SEG_U32: static_cast<uint32_t *>(p)[at] = (uint32_t)v; break;
    default: static_cast<int64_t *>(p)[at] = v; break;
    }
}

// index of a label in its key table: -1 for the background, for a value no int32 holds and for a label not in the table
__device__ __forceinline__ int64_t label_index(const KeyTable &t, int64_t label)
{
    if (label == 0 || label < (int64_t)INT32_MIN || label > (int64_t)INT32_MAX) return -1;
    const int64_t i = find_key(t, (int32_t)label);
    return i < t.n_keys ? i : -1;                          // (a LUT holds only indices below n_keys: a second fence)
}

// the two labels of the wave's pixel e and where its runs begin
struct Pixel {
    int64_t cell, nuc;     // 0 past the image
    bool pair_begins;      // a run of a non-zero (cell, nucleus) label pair begins here
    bool nuc_begins;       // a stretch of one nuclear label (0 included) begins here
};

__device__ __forceinline__ Pixel read_pixel(const LabelPlane &cell, const LabelPlane &nuc, int w, int64_t total, int64_t e, int lane)
{
    Pixel px;
    px.cell = px.nuc = 0;
    bool row_start = false;
    if (e < total) {
        const int64_t y = e / w, x = e - y * w;
        px.cell = load_label(cell, y * cell.ld + x);
        px.nuc = load_label(nuc, y * nuc.ld + x);
        row_start = x == 0;
    }
    const int64_t left_cell = __shfl_up(px.cell, 1, 64), left_nuc = __shfl_up(px.nuc, 1, 64);
    px.nuc_begins = lane == 0 || left_nuc != px.nuc;
    px.pair_begins = px.cell != 0 && px.nuc != 0 && (px.nuc_begins || row_start || left_cell != px.cell);
    return px;
}

__global__ __launch_bounds__(256) void count_kernel(LabelPlane cell, LabelPlane nuc, int w, int64_t total, int32_t *__restrict__ runs)
{
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t)blockIdx.x * kRunSpan;
    int mine = 0;                                          // the wave's runs (same in every lane)
    for (int it = 0; it < kRunSpan / 256; it++) {
        const Pixel px = read_pixel(cell, nuc, w, total, e0 + (int64_t)it * 256 + threadIdx.x, lane);
        mine += __popcll(__ballot(px.pair_begins));
    }
    if (lane == 0 && mine) atomicAdd(runs, mine);
}

__global__ __launch_bounds__(256) void init_kernel(const int32_t *__restrict__ runs, int64_t capacity,
                                                   unsigned long long *__restrict__ area, int64_t n_nuc,
                                                   unsigned long long *__restrict__ top, int64_t n_cells)
{
    if ((int64_t)*runs > capacity) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_nuc + n_cells; i += (int64_t)gridDim.x * 256) {
        if (i < n_nuc) area[i] = 0ull;
        else top[i - n_nuc] = 0ull;
    }
}

// pixels from `lane` to the next set bit of `stops` above it, or to the end of the wave
__device__ __forceinline__ int stretch(unsigned long long stops, int lane)
{
    const unsigned long long above = lane == 63 ? 0ull : stops >> (lane + 1);
    return above ? __ffsll((long long)above) : 64 - lane;
}

__global__ __launch_bounds__(256) void insert_kernel(LabelPlane cell, LabelPlane nuc, int w, int64_t total, KeyTable tc, KeyTable tn,
                                                     const int32_t *__restrict__ runs, int64_t capacity,
                                                     unsigned long long *__restrict__ keys, int32_t *__restrict__ counts,
                                                     int64_t slots, int32_t *__restrict__ n_pairs,
                                                     unsigned long long *__restrict__ area)
{
    if ((int64_t)*runs > capacity) return;                 // (uniform) more insertions than the table was sized for: none is made
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t)blockIdx.x * kRunSpan;
    for (int it = 0; it < kRunSpan / 256; it++) {
        const int64_t e = e0 + (int64_t)it * 256 + threadIdx.x;
        const Pixel px = read_pixel(cell, nuc, w, total, e, lane);
        // a stretch of a nuclear label ends where the next begins (a pixel past the image reads 0: it ends one too); a run
        // of a pair also at a pixel without a pair
        const unsigned long long nuc_stops = __ballot(px.nuc_begins);
        const unsigned long long pair_stops = __ballot(px.pair_begins || px.cell == 0 || px.nuc == 0);
        const bool count_area = px.nuc_begins && px.nuc != 0;
        if (!count_area && !px.pair_begins) continue;
        const int64_t j = label_index(tn, px.nuc);
        if (j < 0) continue;
        if (count_area) atomicAdd(area + j, (unsigned long long)stretch(nuc_stops, lane));
        if (!px.pair_begins) continue;
        const int64_t c = label_index(tc, px.cell);
        if (c < 0) continue;
        table_add(keys, counts, slots, ((unsigned long long)c << 32) | (unsigned long long)j, stretch(pair_stops, lane), n_pairs);
    }
}

__global__ __launch_bounds__(256) void sweep_kernel(const int32_t *__restrict__ runs, int64_t capacity,
                                                    const unsigned long long *__restrict__ keys,
                                                    const int32_t *__restrict__ counts, int64_t slots,
                                                    unsigned long long *__restrict__ top, int64_t n_cells)
{
    if ((int64_t)*runs > capacity) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256) {
        const unsigned long long key = keys[i];
        if (key == kEmpty) continue;
        const int64_t c = (int64_t)(key >> 32);
        const uint32_t j = (uint32_t)(key & 0xffffffffull);
        if (c < n_cells) atomicMax(top + c, ((unsigned long long)(uint32_t)counts[i] << 32) | (unsigned long long)(uint32_t)~j);
    }
}

__global__ __launch_bounds__(256) void finish_kernel(int64_t capacity, const unsigned long long *__restrict__ top, int64_t n_cells,
                                                     int32_t *__restrict__ best, int32_t *__restrict__ n_dev)
{
    const bool fits = (int64_t)n_dev[1] <= capacity;
    if (!fits) {
        if (blockIdx.x == 0 && threadIdx.x == 0) n_dev[0] = -1;
        return;
    }
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_cells; c += (int64_t)gridDim.x * 256) {
        const unsigned long long t = top[c];               // 0: no pair (a pair has at least one pixel)
        best[2 * c] = t ? (int32_t)~(uint32_t)(t & 0xffffffffull) : -1;
        best[2 * c + 1] = (int32_t)(t >> 32);
    }
}

struct ApplyArgs {
    LabelPlane cell, nuc;
    void *out;
    int64_t ldo;
    int h, w;
    const int32_t *chosen;       // [n_cells] index of the nucleus the cell splits
    const int64_t *cell_value;   // [n_cells] the new label of the overlap, -1: the cell splits nothing
    const int64_t *nuc_value;    // [n_nuc] what a nucleus's other pixels become
};

__global__ __launch_bounds__(256) void apply_kernel(ApplyArgs a, KeyTable tc, KeyTable tn)
{
    const int64_t total = (int64_t)a.h * a.w;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t y = e / a.w, x = e - y * a.w;
        const int64_t vn = load_label(a.nuc, y * a.nuc.ld + x);
        int64_t v = vn;                                    // a label in no key table is copied through
        const int64_t j = label_index(tn, vn);
        if (j >= 0) {
            v = a.nuc_value[j];
            const int64_t c = label_index(tc, load_label(a.cell, y * a.cell.ld + x));
            if (c >= 0 && (int64_t)a.chosen[c] == j) {
                const int64_t split = a.cell_value[c];
                if (split >= 0) v = split;
            }
        }
        store_label(a.out, a.nuc.dtype, y * a.ldo + x, v);
    }
}

size_t lut_bytes(int64_t n_keys, int32_t key_min, int32_t key_max, int flags)
{
    return (flags & PXSOM_NUCSPLIT_FORCE_SEARCH) ? 0 : pxsom::dense_lut_bytes(n_keys, key_min, key_max);
}

struct Layout {
    size_t cell_lut, nuc_lut, top, table, total;
    size_t cell_lut_b, nuc_lut_b;
};

// capacity 0: the layout of pxsom_split_apply (the two LUTs only)
Layout layout(int64_t capacity, int64_t n_cells, int32_t cell_min, int32_t cell_max, int64_t n_nuc, int32_t nuc_min,
              int32_t nuc_max, int flags)
{
    Layout L;
    size_t at = 0;
    L.cell_lut_b = lut_bytes(n_cells, cell_min, cell_max, flags);
    L.cell_lut = at;
    at += pxsom::align_up(L.cell_lut_b, 256);
    L.nuc_lut_b = lut_bytes(n_nuc, nuc_min, nuc_max, flags);
    L.nuc_lut = at;
    at += pxsom::align_up(L.nuc_lut_b, 256);
    L.top = L.table = at;
    if (capacity > 0) {
        at += pxsom::align_up((size_t)std::max<int64_t>(n_cells, 1) * sizeof(unsigned long long), 256);
        L.table = at;
        at += pair_table_bytes(capacity);
    }
    L.total = at;
    return L;
}

// what both entries check the same way; 0 or the error code
int check_planes(const char *fn, const void *cell_dev, int cell_dtype, int64_t ldc, const void *nuc_dev, int nuc_dtype, int64_t ldn,
                 int h, int w, const int32_t *cell_keys_dev, int64_t n_cells, int32_t cell_min, int32_t cell_max,
                 const int32_t *nuc_keys_dev, int64_t n_nuc, int32_t nuc_min, int32_t nuc_max, int flags)
{
    if (!pxsom::is_label_dtype(cell_dtype) || !pxsom::is_label_dtype(nuc_dtype))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: label dtypes %d, %d are outside %d .. %d", fn, cell_dtype, nuc_dtype,
                           PXSOM_SEG_U8, PXSOM_SEG_I64);
    if (h < 1 || w < 1 || ldc < w || ldn < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad size or stride (h=%d w=%d ldc=%lld ldn=%lld)", fn, h, w, (long long)ldc,
                           (long long)ldn);
    if ((int64_t)h * w > INT32_MAX)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: %d x %d pixels are beyond the limit %d", fn, h, w, INT32_MAX);
    if (flags & ~PXSOM_NUCSPLIT_FORCE_SEARCH) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: unknown flags %d", fn, flags);
    if (n_cells < 0 || n_nuc < 0 || n_cells > INT32_MAX || n_nuc > INT32_MAX)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: key counts %lld, %lld are outside 0 .. %d", fn, (long long)n_cells,
                           (long long)n_nuc, INT32_MAX);
    if ((n_cells > 0 && (!cell_keys_dev || cell_min > cell_max)) || (n_nuc > 0 && (!nuc_keys_dev || nuc_min > nuc_max)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null key table or key_min > key_max", fn);
    if (!cell_dev || !nuc_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null plane", fn);
    return PXSOM_OK;
}

int build_tables(KeyTable &tc, KeyTable &tn, const Layout &L, char *ws, hipStream_t st)
{
    if (L.cell_lut_b) {
        const int rc = build_lut(tc, reinterpret_cast<int32_t *>(ws + L.cell_lut), L.cell_lut_b, st);
        if (rc != PXSOM_OK) return rc;
    }
    if (L.nuc_lut_b) {
        const int rc = build_lut(tn, reinterpret_cast<int32_t *>(ws + L.nuc_lut), L.nuc_lut_b, st);
        if (rc != PXSOM_OK) return rc;
    }
    return PXSOM_OK;
}

}  // namespace

PXSOM_EXPORT size_t pxsom_nuclear_overlaps_workspace_bytes(int64_t capacity, int64_t n_cells, int32_t cell_min, int32_t cell_max,
                                                           int64_t n_nuc, int32_t nuc_min, int32_t nuc_max, int flags)
{
    if (capacity < 1 || capacity > kMaxPairCapacity || n_cells < 0 || n_nuc < 0 || n_cells > INT32_MAX || n_nuc > INT32_MAX)
        return 0;
    return layout(capacity, n_cells, cell_min, cell_max, n_nuc, nuc_min, nuc_max, flags).total;
}

PXSOM_EXPORT int pxsom_nuclear_overlaps(const void *cell_dev, int cell_dtype, int64_t ldc, const void *nuc_dev, int nuc_dtype,
                                        int64_t ldn, int h, int w, const int32_t *cell_keys_dev, int64_t n_cells,
                                        int32_t cell_min, int32_t cell_max, const int32_t *nuc_keys_dev, int64_t n_nuc,
                                        int32_t nuc_min, int32_t nuc_max, int64_t *area_dev, int32_t *best_dev,
                                        int64_t capacity, int32_t *n_dev, void *workspace_dev, size_t workspace_bytes,
                                        int flags, void *stream)
{
    const char *fn = "pxsom_nuclear_overlaps";
    const int bad = check_planes(fn, cell_dev, cell_dtype, ldc, nuc_dev, nuc_dtype, ldn, h, w, cell_keys_dev, n_cells, cell_min,
                                 cell_max, nuc_keys_dev, n_nuc, nuc_min, nuc_max, flags);
    if (bad != PXSOM_OK) return bad;
    if (!n_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null n_dev", fn);
    const bool count_only = area_dev == nullptr && best_dev == nullptr;
    Layout L{};
    if (!count_only) {
        if (!area_dev || !best_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: area_dev and best_dev go together", fn);
        if (capacity < 1 || capacity > kMaxPairCapacity)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: capacity %lld is outside 1 .. %lld", fn, (long long)capacity,
                               (long long)kMaxPairCapacity);
        L = layout(capacity, n_cells, cell_min, cell_max, n_nuc, nuc_min, nuc_max, flags);
        if (!workspace_dev || workspace_bytes < L.total)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, L.total);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t total = (int64_t)h * w;
    const unsigned spans = (unsigned)((total + kRunSpan - 1) / kRunSpan);
    const LabelPlane cell{cell_dev, ldc, cell_dtype}, nuc{nuc_dev, ldn, nuc_dtype};

    PXSOM_HIP_TRY(hipMemsetAsync(n_dev, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(count_kernel, dim3(spans), dim3(256), 0, st, cell, nuc, w, total, n_dev + 1);
    if (!count_only) {
        char *ws = static_cast<char *>(workspace_dev);
        KeyTable tc{cell_keys_dev, nullptr, n_cells, cell_min, 0}, tn{nuc_keys_dev, nullptr, n_nuc, nuc_min, 0};
        const int rc = build_tables(tc, tn, L, ws, st);
        if (rc != PXSOM_OK) return rc;
        const int64_t slots = pair_slots(capacity);
        unsigned long long *top = reinterpret_cast<unsigned long long *>(ws + L.top);
        unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + L.table);
        int32_t *counts = pair_table_counts(keys, slots);
        unsigned long long *area = reinterpret_cast<unsigned long long *>(area_dev);
        PXSOM_HIP_TRY(hipMemsetAsync(keys, 0xFF, (size_t)slots * sizeof(unsigned long long), st));    // every slot kEmpty
        PXSOM_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)slots * sizeof(int32_t), st));
        hipLaunchKernelGGL(init_kernel, dim3(pxsom::flat_grid(n_nuc + n_cells, 4)), dim3(256), 0, st, n_dev + 1, capacity, area,
                           n_nuc, top, n_cells);
        hipLaunchKernelGGL(insert_kernel, dim3(spans), dim3(256), 0, st, cell, nuc, w, total, tc, tn, n_dev + 1, capacity, keys,
                           counts, slots, n_dev, area);
        hipLaunchKernelGGL(sweep_kernel, dim3(pxsom::flat_grid(slots)), dim3(256), 0, st, n_dev + 1, capacity, keys, counts, slots,
                           top, n_cells);
        hipLaunchKernelGGL(finish_kernel, dim3(pxsom::flat_grid(n_cells, 4)), dim3(256), 0, st, capacity, top, n_cells, best_dev,
                           n_dev);
    }
    PXSOM_LAUNCH_CHECK("pxsom_nuclear_overlaps kernels");
    return PXSOM_OK;
}

PXSOM_EXPORT size_t pxsom_split_apply_workspace_bytes(int64_t n_cells, int32_t cell_min, int32_t cell_max, int64_t n_nuc,
                                                      int32_t nuc_min, int32_t nuc_max, int flags)
{
    if (n_cells < 0 || n_nuc < 0 || n_cells > INT32_MAX || n_nuc > INT32_MAX) return 0;
    return layout(0, n_cells, cell_min, cell_max, n_nuc, nuc_min, nuc_max, flags).total;
}

PXSOM_EXPORT int pxsom_split_apply(const void *cell_dev, int cell_dtype, int64_t ldc, const void *nuc_dev, int nuc_dtype,
                                   int64_t ldn, int h, int w, const int32_t *cell_keys_dev, int64_t n_cells, int32_t cell_min,
                                   int32_t cell_max, const int32_t *nuc_keys_dev, int64_t n_nuc, int32_t nuc_min,
                                   int32_t nuc_max, const int32_t *chosen_dev, const int64_t *cell_value_dev,
                                   const int64_t *nuc_value_dev, void *out_dev, int64_t ldo, void *workspace_dev,
                                   size_t workspace_bytes, int flags, void *stream)
{
    const char *fn = "pxsom_split_apply";
    const int bad = check_planes(fn, cell_dev, cell_dtype, ldc, nuc_dev, nuc_dtype, ldn, h, w, cell_keys_dev, n_cells, cell_min,
                                 cell_max, nuc_keys_dev, n_nuc, nuc_min, nuc_max, flags);
    if (bad != PXSOM_OK) return bad;
    if (ldo < w) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: output stride %lld is below the width %d", fn, (long long)ldo, w);
    if (!out_dev || (n_cells > 0 && (!chosen_dev || !cell_value_dev)) || (n_nuc > 0 && !nuc_value_dev))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null output or table", fn);
    const Layout L = layout(0, n_cells, cell_min, cell_max, n_nuc, nuc_min, nuc_max, flags);
    if (L.total > 0 && (!workspace_dev || workspace_bytes < L.total))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, L.total);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    KeyTable tc{cell_keys_dev, nullptr, n_cells, cell_min, 0}, tn{nuc_keys_dev, nullptr, n_nuc, nuc_min, 0};
    const int rc = build_tables(tc, tn, L, static_cast<char *>(workspace_dev), st);
    if (rc != PXSOM_OK) return rc;
    ApplyArgs a;
    a.cell = LabelPlane{cell_dev, ldc, cell_dtype};
    a.nuc = LabelPlane{nuc_dev, ldn, nuc_dtype};
    a.out = out_dev;
    a.ldo = ldo;
    a.h = h;
    a.w = w;
    a.chosen = chosen_dev;
    a.cell_value = cell_value_dev;
    a.nuc_value = nuc_value_dev;
    hipLaunchKernelGGL(apply_kernel, dim3(pxsom::flat_grid((int64_t)h * w)), dim3(256), 0, st, a, tc, tn);
    PXSOM_LAUNCH_CHECK("apply_kernel");
    return PXSOM_OK;
}
