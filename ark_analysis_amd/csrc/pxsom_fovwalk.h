// pxsom_fovwalk.h -- what the per-cell kernels over FOVs share: the pair test (K13 neighbour counts, K20 close-pair
// counts), the walk over FOVs (K20) and the walk over the type runs of FOVs (K13, K14 nearest-cell means).
//
// One thread owns one query cell (coordinates in registers); a workgroup of 256 owns 256 consecutive rows and visits
// every FOV those rows touch (for_each_fov), taking the FOV's cells as candidates in tiles of 256 staged in LDS.  Every
// lane reads the same candidate (one 16-byte broadcast read, no bank conflict).  Memory safety does not depend on the
// device-side inputs: for_each_fov (and the same loop in walk_fov_runs) clamps the FOV offsets to [0, n], so a body that
// indexes the cell arrays inside [beg, end) stays inside them whatever seg holds.
//
// walk_fov_runs (K13, K14).  The caller hands the cells of a FOV sorted by type, so the candidates of one type are one
// run: what a run gathers lives in the policy's registers and one value per run is stored when the run ends.  Where runs
// begin is known per tile from one ballot per wave at staging time (a 64-bit mask per 64 candidates), so the loop over a
// run carries no type test.  The run boundaries are the same for every lane: no atomics, no LDS counters, any number of
// types.  Each thread writes every column of its own row exactly once -- the fill value between the runs it met, after
// the last one, and for a row no FOV holds -- so the caller need not clear the output.  A type outside [0, n_types) or
// out of order is never stored (its row is then wrong, not its neighbours' memory).
//
// The walk counts, per run, the candidates that count for the policy P, which gives
//   void begin_run()                a run opens: forget the last one
//   void candidates(double xi, double yi, const double2 *c, int p, int q, int &count)
//                                   the run's next candidates, c[p .. q) in LDS; adds to `count` those that count (the
//                                   policy owns this loop, and so its unroll factor)
//   T    end_run(int count)         the run's value
#pragma once
#include "pxsom_common.h"

namespace {

constexpr int kBlock = 256;   // threads per workgroup = query rows per workgroup = candidates per tile
constexpr int kWave = 64;

template <typename T>
struct RowWriter {
    T *row;         // out + i * n_types; touched only when `live`
    int n_types;
    int next;       // columns [0, next) are written
    bool live;
    T fill;         // for the types the cell's FOV lacks

    // `fill` for [next, t), then `v` at column t; t is the same for every lane
    __device__ __forceinline__ void put(int t, T v)
    {
        if (!live || t < next || t >= n_types) return;
        for (int u = next; u < t; ++u) row[u] = fill;
        row[t] = v;
        next = t + 1;
    }
    __device__ __forceinline__ void finish()
    {
        if (!live) return;
        for (int u = next; u < n_types; ++u) row[u] = fill;
        next = n_types;
    }
};

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// s = fl(fl(dx * dx) + fl(dy * dy)): binary64, one IEEE operation per statement, no contraction
__device__ __forceinline__ double squared_distance(double xi, double yi, double2 cj)
{
#pragma clang fp contract(off)
    const double dx = xi - cj.x;
    const double dy = yi - cj.y;
    const double px = dx * dx;
    const double py = dy * dy;
    return px + py;
}

// The pair test: float32(sqrt(s)) < distlim and (SELF or != 0), with the thresholds of som_device.neighbor_thresholds
template <bool SELF>
__device__ __forceinline__ bool pair_is_close(double xi, double yi, double2 cj, double s_lim, double s_zero)
{
    const double s = squared_distance(xi, yi, cj);
    if constexpr (SELF) {
        (void)s_zero;
        return s < s_lim;
    } else {
        return s < s_lim && s > s_zero;
    }
}

// The workgroup's rows [r0, r1) and the thread's query cell, row i (coordinates 0 without a row)
struct BlockRows {
    int64_t r0, r1, i;
    bool has_row;
    double xi, yi;
};

__device__ __forceinline__ BlockRows load_block_rows(const double2 *__restrict__ xy, int64_t n)
{
    BlockRows b;
    b.r0 = (int64_t)blockIdx.x * kBlock;
    b.r1 = b.r0 + kBlock < n ? b.r0 + kBlock : n;
    b.i = b.r0 + threadIdx.x;
    b.has_row = b.i < n;
    b.xi = b.yi = 0.0;
    if (b.has_row) {
        const double2 q = xy[b.i];
        b.xi = q.x;
        b.yi = q.y;
    }
    return b;
}

// body(f, beg, end, mine) for every FOV f holding one of the workgroup's rows: its cells are rows [beg, end), not empty,
// inside [0, n]; `mine`: the thread's row is one of them.  All threads take the same trips: body may __syncthreads().
template <typename Body>
__device__ __forceinline__ void for_each_fov(const int64_t *__restrict__ seg, int64_t n_fovs, int64_t n,
                                             const BlockRows &rows, Body body)
{
    // the first FOV that ends beyond r0
    int64_t lo = 0, hi = n_fovs;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (seg[mid + 1] > rows.r0) hi = mid; else lo = mid + 1;
    }
    for (int64_t f = lo; f < n_fovs; ++f) {
        const int64_t beg = clamp_i64(seg[f], 0, n);
        const int64_t end = clamp_i64(seg[f + 1], beg, n);
        if (beg >= rows.r1) break;
        if (end <= rows.r0 || end == beg) continue;
        body(f, beg, end, rows.has_row && rows.i >= beg && rows.i < end);
    }
}

// cand, ctype, run_start: the calling kernel's LDS, [kBlock], [kBlock] and [kBlock / kWave]
template <typename T, typename P>
__device__ __forceinline__ void walk_fov_runs(const double2 *__restrict__ xy, const int32_t *__restrict__ type,
                                              const int64_t *__restrict__ seg, int64_t n_fovs, int64_t n, int n_types,
                                              T fill, T *__restrict__ out_rows, double2 *cand, int32_t *ctype,
                                              unsigned long long *run_start, P &run)
{
    const int tid = threadIdx.x;
    // load_block_rows and for_each_fov, written out: through them the compiler schedules K13's loop otherwise and the
    // kernel measured 3 - 6 % slower; like this K13 and K14 are the code they were.  Keep them in step.
    const int64_t r0 = (int64_t)blockIdx.x * kBlock;
    const int64_t r1 = r0 + kBlock < n ? r0 + kBlock : n;
    const int64_t i = r0 + tid;
    const bool has_row = i < n;
    double xi = 0.0, yi = 0.0;
    if (has_row) {
        const double2 q = xy[i];
        xi = q.x;
        yi = q.y;
    }
    RowWriter<T> out{has_row ? out_rows + i * n_types : nullptr, n_types, 0, has_row, fill};

    int64_t lo = 0, hi = n_fovs;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (seg[mid + 1] > r0) hi = mid; else lo = mid + 1;
    }
    for (int64_t f = lo; f < n_fovs; ++f) {
        const int64_t beg = clamp_i64(seg[f], 0, n);
        const int64_t end = clamp_i64(seg[f + 1], beg, n);
        if (beg >= r1) break;
        if (end <= r0 || end == beg) continue;
        const bool mine = has_row && i >= beg && i < end;
        int cur = -1, c = 0;   // the open run's type and how many of its candidates counted
        for (int64_t base = beg; base < end; base += kBlock) {
            const int tile_n = end - base < kBlock ? (int)(end - base) : kBlock;
            __syncthreads();   // the previous tile has been read
            bool starts = false;
            if (tid < tile_n) {
                const int64_t j = base + tid;
                const int32_t t = type[j];
                cand[tid] = xy[j];
                ctype[tid] = t;
                starts = j == beg || type[j - 1] != t;
            }
            const unsigned long long m = __ballot(starts);
            if ((tid & (kWave - 1)) == 0) run_start[tid / kWave] = m;
            __syncthreads();
            for (int w0 = 0; w0 < tile_n; w0 += kWave) {
                const unsigned long long full = run_start[w0 / kWave];
                const unsigned long long mask =
                    ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(full >> 32)) << 32) |
                    (unsigned)__builtin_amdgcn_readfirstlane((int)full);
                const int cnt = tile_n - w0 < kWave ? tile_n - w0 : kWave;
                int p = 0;
                while (p < cnt) {
                    if ((mask >> p) & 1ull) {
                        if (mine && cur >= 0) out.put(cur, run.end_run(c));
                        cur = __builtin_amdgcn_readfirstlane(ctype[w0 + p]);
                        c = 0;
                        run.begin_run();
                    }
                    const unsigned long long rest = p + 1 < kWave ? mask >> (p + 1) : 0ull;
                    int q = rest ? p + 1 + __builtin_ctzll(rest) : kWave;
                    q = q < cnt ? q : cnt;
                    run.candidates(xi, yi, cand + w0, p, q, c);
                    p = q;
                }
            }
        }
        if (mine && cur >= 0) out.put(cur, run.end_run(c));
    }
    out.finish();
}

// The check the entries with the pair test share (K13, K20)
[[maybe_unused]] int check_pair_test(const char *fn, int self_neighbor, double s_lim, double s_zero)
{
    if (self_neighbor != 0 && self_neighbor != 1)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: self_neighbor=%d is not 0 or 1", fn, self_neighbor);
    if (s_lim != s_lim || s_zero != s_zero) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a threshold is NaN", fn);
    return PXSOM_OK;
}

// The argument checks the entries share, with the entry's `own` checks (a callable returning a status) in their place
// between the sizes and the pointers.  PXSOM_OK with *blocks = 0: nothing to launch (n == 0).
template <typename Own>
int check_cell_args(const char *fn, const double *xy_dev, const int32_t *type_dev, const int64_t *seg_dev, int64_t n_fovs,
                    int64_t n, int n_types, const void *out_dev, unsigned *blocks, Own own)
{
    *blocks = 0;
    if (n < 0 || n_fovs < 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld, n_fovs=%lld", fn, (long long)n, (long long)n_fovs);
    if (n_types < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_types=%d < 1", fn, n_types);
    const int rc = own();
    if (rc != PXSOM_OK) return rc;
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null seg", fn);
    if (n == 0) return PXSOM_OK;
    if (!xy_dev || !type_dev || !out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
    if (reinterpret_cast<uintptr_t>(xy_dev) % sizeof(double2) != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: xy is not 16-byte aligned", fn);
    const int64_t nb = (n + kBlock - 1) / kBlock;
    if (nb > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld too large", fn, (long long)n);
    *blocks = (unsigned)nb;
    return PXSOM_OK;
}

}  // namespace
