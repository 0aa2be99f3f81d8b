// pxsom_segmask.hip -- cell cluster masks on gfx950 (K10): border erosion + label -> value lookup over a segmentation image.
//
//   pxsom_segmask   find_boundaries(seg, connectivity, mode "thick" / "inner") + np.where(edges == 0, seg, 0)  (erode_mask)
//                   then mapping.get((int32)label, unassigned) (relabel_segmentation) and the output cast
//                   (ark/utils/data_utils.py:70-84, 204-335 of the reference)
//
// One fused pass over the tile of pxsom_plane.h, which K29 shares.  A block is 4 waves; each wave owns 256 columns x
// kTileRowsPerWave rows, every lane 4 consecutive pixels of a row (one 4-, 8-, 16- or 32-byte load per row, one packed
// store per row).  With erosion a wave loads
// kTileRowsPerWave + 2 rows up front (the one-row halo above and below comes from L1 / L2: it is the neighbouring wave's or
// block's own row, read there in the same sweep, so HBM sees each input byte about once); the left / right halo column
// comes from the neighbouring lane by a cross-lane shuffle, and only lanes 0 and 63 load one extra element per row.
// No LDS staging: the halo re-read is 2 of 6 rows and served by the caches, and the shuffle replaces the LDS round trip
// (DESIGN.md K10 has the numbers).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "pxsom_common.h"
#include "pxsom_keytable.h"

namespace {

template <typename TV>
struct Table {
    KeyTable k;              // k.n_keys < 0: no lookup
    const TV *values;
    TV unassigned;
};

template <typename TV, typename TI>
__device__ __forceinline__ TV lookup(const Table<TV> &t, TI label)
{
    const int64_t idx = find_key(t.k, (int32_t)(int64_t)label);   // numpy astype(np.int32): two's-complement wrap
    return idx >= 0 ? t.values[idx] : t.unassigned;
}

template <typename TI, typename TO, typename TV>
__device__ __forceinline__ TO finish(const Table<TV> &t, TI label)
{
    if (t.k.n_keys < 0) return (TO)label;   // no lookup: the (eroded) label, cast as numpy casts
    return (TO)lookup<TV, TI>(t, label);
}

template <typename TI, typename TO, typename TV>
__global__ __launch_bounds__(256) void segmask_kernel(const TI *__restrict__ seg, int h, int w, int64_t ld, int erode_mode,
                                                      int conn8, int64_t background, Table<TV> table, TO *__restrict__ out,
                                                      int64_t ldo, bool vec_in, bool vec_out, int col_blocks)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bx = (int)(blockIdx.x % (unsigned)col_blocks), by = (int)(blockIdx.x / (unsigned)col_blocks);
    const int row0 = by * kTileBlockRows + wave * kTileRowsPerWave;
    if (row0 >= h) return;                                   // whole wave: the shuffles below stay inside live waves
    const int c0 = bx * kTileWaveCols + lane * 4;
    const int rows = min(kTileRowsPerWave, h - row0);

    if (erode_mode == PXSOM_SEG_ERODE_NONE) {
        TI v[kTileRowsPerWave][4];
#pragma unroll
        for (int i = 0; i < kTileRowsPerWave; i++) load4(seg, ld, min(row0 + i, h - 1), c0, w, vec_in, v[i]);
#pragma unroll
        for (int i = 0; i < kTileRowsPerWave; i++) {
            if (i >= rows) break;
            TO o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = finish<TI, TO, TV>(table, v[i][k]);
            store4(out, ldo, row0 + i, c0, w, vec_out, o);
        }
        return;
    }

    // load_halo_tile (pxsom_plane.h) written out: through the helper every instantiation came out with 2 to 4 fewer VGPRs and
    // other scheduling, and at 2048 x 2048 three of four cases measured 0.2 - 0.4 % beyond the parent's own run-to-run spread
    // (profiles/plane_shared/README.md).  This form compiles to the code it had.
    constexpr int kL = kTileHaloRows;
    TI v[kL][4], left[kL], right[kL];
#pragma unroll
    for (int i = 0; i < kL; i++) load4(seg, ld, min(max(row0 - 1 + i, 0), h - 1), c0, w, vec_in, v[i]);
#pragma unroll
    for (int i = 0; i < kL; i++) {
        left[i] = shfl_up1(v[i][3]);     // lane - 1's last pixel
        right[i] = shfl_down1(v[i][0]);  // lane + 1's first pixel
    }
    if (lane == 0 || lane == 63) {       // the halo column of the wave's tile: one element per row, from L1 / L2
        const int cc = lane == 0 ? max(c0 - 1, 0) : min(c0 + 4, w - 1);
#pragma unroll
        for (int i = 0; i < kL; i++) {
            const TI x = seg[(int64_t)min(max(row0 - 1 + i, 0), h - 1) * ld + cc];
            if (lane == 0) left[i] = x;
            else right[i] = x;
        }
    }
#pragma unroll
    for (int i = 1; i <= kTileRowsPerWave; i++) {
        if (i > rows) break;
        TO o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const TI c = v[i][k];
            const TI l0 = k == 0 ? left[i - 1] : v[i - 1][k - 1], r0 = k == 3 ? right[i - 1] : v[i - 1][k + 1];
            const TI l1 = k == 0 ? left[i] : v[i][k - 1], r1 = k == 3 ? right[i] : v[i][k + 1];
            const TI l2 = k == 0 ? left[i + 1] : v[i + 1][k - 1], r2 = k == 3 ? right[i + 1] : v[i + 1][k + 1];
            bool edge = (v[i - 1][k] != c) | (v[i + 1][k] != c) | (l1 != c) | (r1 != c);
            if (conn8) edge |= (l0 != c) | (r0 != c) | (l2 != c) | (r2 != c);
            if (erode_mode == PXSOM_SEG_ERODE_INNER) edge &= (int64_t)c != background;
            o[k] = finish<TI, TO, TV>(table, edge ? (TI)0 : c);
        }
        store4(out, ldo, row0 + i - 1, c0, w, vec_out, o);
    }
}

struct Launch {
    const void *seg;
    int h, w;
    int64_t ld;
    int erode_mode, conn8;
    int64_t background;
    KeyTable keys;
    const void *values;
    double unassigned;
    void *out;
    int64_t ldo;
    hipStream_t st;
};

template <typename TI, typename TO>
int launch_typed(const Launch &a)
{
    typedef typename std::conditional<std::is_same<TO, double>::value, double, int32_t>::type TV;
    const Table<TV> t{a.keys, reinterpret_cast<const TV *>(a.values), (TV)a.unassigned};
    const bool vec_in = rows_aligned4(a.seg, a.ld, sizeof(TI)), vec_out = rows_aligned4(a.out, a.ldo, sizeof(TO));
    const int col_blocks = (a.w + kTileWaveCols - 1) / kTileWaveCols;
    const int64_t blocks = (int64_t)col_blocks * ((a.h + kTileBlockRows - 1) / kTileBlockRows);
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_segmask: image too large");
    PXSOM_TIMED_LAUNCH((segmask_kernel<TI, TO, TV>), dim3((unsigned)blocks), dim3(256), 0, a.st,
                       reinterpret_cast<const TI *>(a.seg), a.h, a.w, a.ld, a.erode_mode, a.conn8, a.background, t,
                       reinterpret_cast<TO *>(a.out), a.ldo, vec_in, vec_out, col_blocks);
    PXSOM_LAUNCH_CHECK("segmask_kernel");
    return PXSOM_OK;
}

template <typename TI>
int launch_in(const Launch &a, int out_dtype, int seg_dtype)
{
    if (out_dtype == seg_dtype) return launch_typed<TI, TI>(a);
    if (out_dtype == PXSOM_SEG_I16) return launch_typed<TI, int16_t>(a);
    if (out_dtype == PXSOM_SEG_I32) return launch_typed<TI, int32_t>(a);
    return launch_typed<TI, double>(a);
}

}  // namespace

PXSOM_EXPORT size_t pxsom_segmask_workspace_bytes(int64_t n_keys, int32_t key_min, int32_t key_max)
{
    return pxsom::dense_lut_bytes(n_keys, key_min, key_max);
}

PXSOM_EXPORT int pxsom_segmask(const void *seg_dev, int seg_dtype, int h, int w, int64_t ld, int erode_mode,
                               int connectivity, int64_t background, const int32_t *keys_dev, const void *values_dev,
                               int64_t n_keys, int32_t key_min, int32_t key_max, double unassigned, void *out_dev,
                               int out_dtype, int64_t ldo, void *workspace_dev, size_t workspace_bytes, int flags,
                               void *stream)
{
    const char *fn = "pxsom_segmask";
    if (!pxsom::is_label_dtype(seg_dtype))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad seg_dtype %d", fn, seg_dtype);
    if (out_dtype != seg_dtype && out_dtype != PXSOM_SEG_I16 && out_dtype != PXSOM_SEG_I32 && out_dtype != PXSOM_SEG_F64)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad out_dtype %d", fn, out_dtype);
    if (erode_mode < PXSOM_SEG_ERODE_NONE || erode_mode > PXSOM_SEG_ERODE_INNER)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad erode_mode %d", fn, erode_mode);
    if (erode_mode != PXSOM_SEG_ERODE_NONE && connectivity < 1)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: connectivity %d < 1", fn, connectivity);
    if (h < 1 || w < 1 || ld < w || ldo < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad sizes (%d x %d, ld %lld, ldo %lld)", fn, h, w, (long long)ld,
                           (long long)ldo);
    if (flags & ~PXSOM_SEGMASK_FORCE_SEARCH) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: unknown flags %d", fn, flags);
    if (!seg_dev || !out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null image", fn);
    if (n_keys > 0 && (!keys_dev || !values_dev || key_min > key_max))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad table (null, or key_min > key_max)", fn);
    if (n_keys >= 0 && out_dtype != PXSOM_SEG_F64 &&
        !(std::isfinite(unassigned) && unassigned == std::floor(unassigned) && unassigned >= -2147483648.0 &&
          unassigned <= 2147483647.0))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: unassigned %g is not an int32 value", fn, unassigned);
    if (erode_mode != PXSOM_SEG_ERODE_NONE) {   // erosion reads neighbours another block may already have written
        if (pxsom::spans_overlap(seg_dev, pxsom::plane_span_bytes(h, w, ld, pxsom::plane_dtype_bytes(seg_dtype)), out_dev,
                                 pxsom::plane_span_bytes(h, w, ldo, pxsom::plane_dtype_bytes(out_dtype))))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: out overlaps seg under erosion", fn);
    }
    const size_t need = n_keys > 0 && !(flags & PXSOM_SEGMASK_FORCE_SEARCH)
                            ? pxsom_segmask_workspace_bytes(n_keys, key_min, key_max) : 0;
    if (need > 0 && (!workspace_dev || workspace_bytes < need))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);

    Launch a;
    a.seg = seg_dev;
    a.h = h;
    a.w = w;
    a.ld = ld;
    a.erode_mode = erode_mode;
    a.conn8 = connectivity >= 2;
    a.background = background;
    a.keys = KeyTable{keys_dev, nullptr, n_keys < 0 ? -1 : n_keys, key_min, 0};
    a.values = values_dev;
    a.unassigned = unassigned;
    a.out = out_dev;
    a.ldo = ldo;
    a.st = reinterpret_cast<hipStream_t>(stream);
    if (need > 0) {
        const int rc = build_lut(a.keys, static_cast<int32_t *>(workspace_dev), need, a.st);
        if (rc != PXSOM_OK) return rc;
    }
    return pxsom::dispatch_label(seg_dtype, [&](auto ti) { return launch_in<decltype(ti)>(a, out_dtype, seg_dtype); });
}
