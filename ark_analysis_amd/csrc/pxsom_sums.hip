// pxsom_sums.hip -- K8, per-cluster sums on gfx950 (pxsom_cluster_sums, pxsom_pair_histogram; the accumulation half of the
// batch rule).  pxsom_cluster_sums replaces the pandas groupby-sum of compute_pixel_cluster_channel_avg.  Three kernels, chosen
// by shape in cluster_sums_typed: wave-private LDS tables with two channels per lane (first below), the same with one channel
// per lane (cluster_sums_private_kernel), and a workgroup table updated with LDS atomics (cluster_sums_kernel).
//
// Two channels per lane.  Same scheme as cluster_sums_private_kernel: every wave owns a [k + 1, c] binary64 table
// and updates it with plain read / add / write, the lanes of one instruction touching distinct words unless
// two of its rows carry the same label (then the group is applied row by row).  Here a lane holds a channel
// PAIR: c / 2 lanes per row, RPI = 64 / (c / 2) rows per instruction (5 at c = 22 instead of 2), one 8-byte
// load and one ds_read_b128 / ds_write_b128 per lane and group.  That kernel was bound by its instruction
// count (one dword per lane: the load stream alone ran at 4.6 TB/s); this one issues 2.5x fewer per row.
// With more rows per instruction a repeat inside a group is likelier (10 % at K = 100, RPI = 5), so groups
// are not paired up: one group = one unit.
#include <algorithm>

#include "pxsom_assign.h"
#include "pxsom_common.h"
#include "pxsom_sums.h"

namespace pxsom {
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));

template <typename T>
struct PairBits;
template <>
struct PairBits<float> {
    typedef u2 type;
    static __device__ __forceinline__ type load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
    {
        return __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    }
    static __device__ __forceinline__ d2 widen(type v)
    {
        return d2{(double)__uint_as_float(v[0]), (double)__uint_as_float(v[1])};
    }
};
template <>
struct PairBits<_Float16> {
    typedef unsigned type;
    static __device__ __forceinline__ type load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
    {
        return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
    }
    static __device__ __forceinline__ d2 widen(type v)
    {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 h = __builtin_bit_cast(h2, v);
        return d2{(double)h[0], (double)h[1]};
    }
};

template <>
struct PairBits<double> {
    typedef unsigned type __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ type load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
    {
        return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    }
    static __device__ __forceinline__ d2 widen(type v) { return __builtin_bit_cast(d2, v); }
};

template <typename T, int RPI, bool COUNT_F64>
__global__ __launch_bounds__(256) void cluster_sums_pairs_kernel(const T *__restrict__ x, int64_t n, int c,
                                                                 int64_t ldx, const int32_t *__restrict__ labels,
                                                                 int k, double *sums, unsigned long long *counts,
                                                                 int64_t rows_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    typedef typename PairBits<T>::type bits_t;
    constexpr int U = sizeof(T) == 8 ? 16 : 32;   // groups per tile == loads in flight per lane
    constexpr int TR = RPI * U;             // rows per tile
    constexpr int RL = 64 / RPI * RPI;      // rows per label register (whole groups)
    constexpr int NL = (TR + RL - 1) / RL;  // label registers per tile
    const int tid = threadIdx.x, bd = blockDim.x, lane = tid & 63, nwv = bd >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tstride = (k + 1) * c + 128;  // doubles per wave table (+ a spare pair per lane)
    double *all = reinterpret_cast<double *>(smem_raw);
    double *tbl = all + (size_t)wv * tstride;
    unsigned *cnt = reinterpret_cast<unsigned *>(all + (size_t)nwv * tstride);  // [k], shared by the waves
    for (int e = tid; e < nwv * tstride; e += bd) all[e] = 0.0;
    for (int e = tid; e < k; e += bd) cnt[e] = 0u;
    __syncthreads();

    const int pairs = c >> 1;
    const int slot = lane / pairs, pr = lane - slot * pairs;
    const bool active = slot < RPI;
    const unsigned lane_off = active ? (unsigned)((slot * ldx + 2 * pr) * (int64_t)sizeof(T)) : 0u;  // bytes
    const int64_t gw = (int64_t)blockIdx.x * nwv + wv;
    const int64_t ra = gw * rows_per_wave;
    const int64_t rb = ra + rows_per_wave < n ? ra + rows_per_wave : n;
    if (ra < rb) {  // wave-uniform
        // whole groups end at row `lim` (relative to ra); the rows behind it (last wave only) are added one by
        // one.  Every load is unconditional with a clamped, wave-uniform row (see cluster_sums_private_kernel).
        const int span = (int)(rb - ra), lim = span - span % RPI;
        const int last = (int)(n - 1 - ra);
        const unsigned gstep = (unsigned)(RPI * ldx * (int64_t)sizeof(T));
        const unsigned safe = (unsigned)((ra + RPI <= n ? 0 : n - RPI - ra) * ldx * (int64_t)sizeof(T));
        const __amdgpu_buffer_rsrc_t xres =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(x + ra * ldx), 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t lres =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(labels + ra), 0, 0x7fffffff, 0x00020000);
        auto load_labels = [&](int rel0, int(&lv)[NL]) {
#pragma unroll
            for (int i = 0; i < NL; i++) {
                const int r = rel0 + i * RL + lane;
                const int lb = __builtin_amdgcn_raw_buffer_load_b32(lres, (r < last ? r : last) * 4, 0, 0) - 1;
                // '&', not '&&': a short-circuit lets the compiler sink the load into a branch
                const bool ok = (r < lim) & (lane < RL) & (i * RL + lane < TR) & ((unsigned)lb < (unsigned)k);
                lv[i] = ok ? lb : k;
            }
        };
        auto load_val = [&](int rel, unsigned off) -> bits_t {
            return PairBits<T>::load(xres, lane_off, rel + RPI <= lim ? off : safe);
        };
        // a label repeated inside a group: that group is applied row by row.  (Rounds by occurrence index --
        // as many as the most frequent label has rows in the group -- were measured: no faster.)
        auto clash_mask = [&](int lab) -> unsigned long long {
            if (RPI == 1) return 0ull;
            const int base = lane / RPI * RPI, pos = lane - base;
            bool cl = false;
#pragma unroll
            for (int d = 1; d < RPI; d++) {
                const int p = pos + d < RPI ? pos + d : pos + d - RPI;
                cl = cl | (__shfl(lab, base + p) == lab);  // every lane takes part in every exchange
            }
            return __ballot(cl && lab != k && lane < RL);
        };
        bits_t val[U];
        int lv_cur[NL], lv_nxt[NL], lv_far[NL];   // labels two tiles ahead, requested before the tile's values
        load_labels(0, lv_cur);
        load_labels(TR, lv_nxt);
        {
            unsigned off = 0;
#pragma unroll
            for (int g = 0; g < U; g++, off += gstep) val[g] = load_val(g * RPI, off);
        }
        // byte address of this lane's pair in the table row of a label: tbl + (label * c + 2 pr) * 8
        char *const lane_word = reinterpret_cast<char *>(tbl) + (active ? 2 * pr : (k + 1) * c + 2 * lane) * 8;
        unsigned tile_off = TR * gstep / RPI;
        for (int rel0 = 0; rel0 < lim; rel0 += TR, tile_off += TR * gstep / RPI) {
            load_labels(rel0 + 2 * TR, lv_far);
            unsigned long long cm[NL];
            int row_bytes[NL];
#pragma unroll
            for (int i = 0; i < NL; i++) {
                if (lv_cur[i] < k) atomicAdd(&cnt[lv_cur[i]], 1u);
                cm[i] = clash_mask(lv_cur[i]);
                row_bytes[i] = (int)__umul24(lv_cur[i], c * 8);
            }
            int word[U];
#pragma unroll
            for (int g = 0; g < U; g++) {
                const int r = g * RPI;
                const int rb8 = __shfl(row_bytes[r / RL], r % RL + slot);
                word[g] = active ? rb8 : 0;
            }
            unsigned off = tile_off;
#pragma unroll
            for (int g = 0; g < U; g++) {
                d2 *const wp = reinterpret_cast<d2 *>(lane_word + word[g]);
                const d2 v = PairBits<T>::widen(val[g]);
                val[g] = load_val(rel0 + TR + g * RPI, off);  // this register's load for the next tile
                off += gstep;
                if (!((cm[g * RPI / RL] >> (g * RPI % RL)) & ((1ull << RPI) - 1))) {
                    *wp = *wp + v;
                } else {
                    // one row at a time.  The fences keep the RPI predicated updates apart: to the compiler they
                    // are mutually exclusive branches of one thread, which it may fold into a single update
#pragma unroll
                    for (int s = 0; s < RPI; s++) {
                        if (slot == s) *wp = *wp + v;
                        __builtin_amdgcn_wave_barrier();
                        asm volatile("" ::: "memory");
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NL; i++) {
                lv_cur[i] = lv_nxt[i];
                lv_nxt[i] = lv_far[i];
            }
        }
        for (int64_t r = ra + lim; r < rb; r++) {  // fewer than RPI rows
            const int lb = labels[r] - 1;
            if ((unsigned)lb < (unsigned)k) {
                if (lane < c) tbl[lb * c + lane] += (double)x[r * ldx + lane];
                if (lane == 0) atomicAdd(&cnt[lb], 1u);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < k * c; e += bd) {
        double v = 0.0;
        for (int w = 0; w < nwv; w++) v += all[(size_t)w * tstride + e];
        if (v != 0.0) __hip_atomic_fetch_add(&sums[e], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int e = tid; e < k; e += bd)
        if (cnt[e]) {
            if constexpr (COUNT_F64)
                __hip_atomic_fetch_add(reinterpret_cast<double *>(counts) + e, (double)cnt[e], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            else
                atomicAdd(&counts[e], (unsigned long long)cnt[e]);
        }
}

template <typename T, int RPI, bool COUNT_F64>
bool launch_pairs(const T *x, int64_t n, int c, int64_t ldx, const int32_t *labels, int k, double *sums, void *counts,
                  hipStream_t st, int nwv, int blocks_per_cu)
{
    const size_t tbytes = ((size_t)(k + 1) * c + 128) * 8;
    const size_t lds = tbytes * nwv + (size_t)k * 4;
    if (lds > 159 * 1024) return false;
    constexpr int TR = RPI * (sizeof(T) == 8 ? 16 : 32);
    const int64_t max_waves = (int64_t)device_cu_count() * blocks_per_cu * nwv;
    int64_t rows_per_wave = (n + max_waves - 1) / max_waves;
    if (rows_per_wave < 4 * TR) rows_per_wave = 4 * TR;
    rows_per_wave = (rows_per_wave + TR - 1) / TR * TR;
    if ((rows_per_wave + 1024) * ldx * (int64_t)sizeof(T) >= (1ll << 31)) return false;   // 32-bit buffer offsets
    const int64_t waves = (n + rows_per_wave - 1) / rows_per_wave;
    const int64_t grid = (waves + nwv - 1) / nwv;
    auto kern = cluster_sums_pairs_kernel<T, RPI, COUNT_F64>;
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
        return false;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * nwv), lds, st, x, n, c, ldx, labels, k, sums,
                       reinterpret_cast<unsigned long long *>(counts), rows_per_wave);
    return true;
}

template <typename T, int RPI>
bool launch_pairs_counts(const T *x, int64_t n, int c, int64_t ldx, const int32_t *labels, int k, double *sums,
                         void *counts, bool counts_f64, hipStream_t st, int nwv, int blocks_per_cu)
{
    return counts_f64 ? launch_pairs<T, RPI, true>(x, n, c, ldx, labels, k, sums, counts, st, nwv, blocks_per_cu)
                      : launch_pairs<T, RPI, false>(x, n, c, ldx, labels, k, sums, counts, st, nwv, blocks_per_cu);
}

}  // namespace

template <typename T>
bool launch_sums_pairs(const T *x, int64_t n, int c, int64_t ldx, const int32_t *labels, int k, double *sums,
                       void *counts, bool counts_f64, hipStream_t st, int nwv, int blocks_per_cu)
{
    if (c % 2 || ldx % 2 || c < 14 || c > 64 || reinterpret_cast<uintptr_t>(x) % (2 * sizeof(T))) return false;
    const int rpi = 64 / (c / 2);
#define PXSOM_PAIRS(R) return launch_pairs_counts<T, R>(x, n, c, ldx, labels, k, sums, counts, counts_f64, st, nwv, blocks_per_cu)
    if (rpi >= 8) PXSOM_PAIRS(8);
    if (rpi >= 5) PXSOM_PAIRS(5);
    if (rpi == 4) PXSOM_PAIRS(4);
    if (rpi == 3) PXSOM_PAIRS(3);
    PXSOM_PAIRS(2);
#undef PXSOM_PAIRS
}

template bool launch_sums_pairs<float>(const float *, int64_t, int, int64_t, const int32_t *, int, double *, void *, bool,
                                       hipStream_t, int, int);
template bool launch_sums_pairs<_Float16>(const _Float16 *, int64_t, int, int64_t, const int32_t *, int, double *, void *,
                                          bool, hipStream_t, int, int);
template bool launch_sums_pairs<double>(const double *, int64_t, int, int64_t, const int32_t *, int, double *, void *, bool,
                                        hipStream_t, int, int);

}  // namespace pxsom

// (the kernels below keep the global unnamed namespace: their symbol names are what profiles and traces were recorded with)
namespace {

// ------------------------------------------------------------------------------------------------
// per-cluster sums/counts.  Each workgroup owns a contiguous row range and a private binary64
// table in LDS (ds_add_f64), flushed once with global_atomic_add_f64.
// Loads are flat-coalesced: lane e reads element e of the row range.
// ------------------------------------------------------------------------------------------------
// How a value joins the workgroup's table.  binary32 / binary64 rows: ds_add_f64.  binary16 rows: every binary16 number is
// an integer multiple of 2^-24 below 2^16, so v * 2^24 is an integer below 2^40 and the table holds exact 64-bit
// fixed-point sums (ds_add_u64: 5.8 lane-atomics per clock per CU against 3.0 for ds_add_f64,
// scripts/ubench/lds_atomic_rate.hip -- this kernel is bound by that rate).  Exact and order-independent: equal to the
// oracle's binary64 sum whenever that one is exact too (sums below 2^29).  Infinities / NaNs go straight to the global
// binary64 table, where they poison the sum as they do in the oracle.
template <typename T>
struct TableAdd {
    static constexpr bool kFixed = false;
    static __device__ __forceinline__ void add(double *ls, size_t slot, T v, double *, size_t = 0)
    {
        __hip_atomic_fetch_add(ls + slot, (double)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    static __device__ __forceinline__ double value(const double *ls, size_t slot) { return ls[slot]; }
};
template <>
struct TableAdd<_Float16> {
    static constexpr bool kFixed = true;
    static __device__ __forceinline__ void add(double *ls, size_t slot, _Float16 v, double *global_sums, size_t global_slot)
    {
        const unsigned b = __builtin_bit_cast(unsigned short, v);
        const unsigned e = (b >> 10) & 31u, m = b & 1023u;
        if (e == 31u) {   // inf / NaN
            __hip_atomic_fetch_add(global_sums + global_slot, (double)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        const unsigned long long q = e ? (unsigned long long)(1024u + m) << (e - 1u) : (unsigned long long)m;
        const unsigned long long sq = (b & 0x8000u) ? 0ull - q : q;   // two's complement
        if (sq)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(ls) + slot, sq, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    static __device__ __forceinline__ double value(const double *ls, size_t slot)
    {
        return (double)reinterpret_cast<const long long *>(ls)[slot] * 0x1p-24;
    }
};

constexpr int kSumsSpare = 16;   // table slots behind the last cluster: where elements without a valid label go

template <typename T, bool COUNT_F64, int NT>
__global__ __launch_bounds__(NT) void cluster_sums_kernel(const T *__restrict__ x, int64_t n, int c,
                                                           int64_t ldx, const int32_t *__restrict__ labels,
                                                           int k, double *sums, unsigned long long *counts,
                                                           int64_t rows_per_block, int use_lds, double qmagic, int cs, pxsom::RowView rv)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    // table row stride cs (words): c, or c padded to an odd number -- the lanes of a ds_add hit rows of unrelated labels, and with
    // an even stride those fall on a fraction of the banks (c = 40: stride 80 dwords, four bank groups in all)
    double *ls = reinterpret_cast<double *>(smem_raw);                 // [k*cs] + kSumsSpare slots nobody reads
    unsigned *lc = reinterpret_cast<unsigned *>(ls + (size_t)k * cs + kSumsSpare);   // [k]
    const int tid = threadIdx.x;
    if (use_lds) {
        for (int e = tid; e < k * cs + kSumsSpare; e += NT) ls[e] = 0.0;
        for (int e = tid; e < k; e += NT) lc[e] = 0u;
        __syncthreads();
    }
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    int64_t r1 = r0 + rows_per_block;
    if (r1 > n) r1 = n;
    // contiguous fp32 rows (ldx == c): the row range is one flat array -- 16-byte loads, 4 per thread in
    // flight (a dword per lane keeps too few bytes in flight for HBM: measured 1.8 TB/s at 10 M rows)
    bool done = false;
    if constexpr (sizeof(T) <= 4) {
        // contiguous fp32 / fp16 rows: VEC = 16 / sizeof(T) elements per load
        constexpr int VEC = 16 / (int)sizeof(T);
        // (a scheduled step's rows where they lie, pxsom::RowView: rows of whole vectors only -- the host sees to it --, a vector's
        // address from its row's place in the caller's matrix instead of from the flat range)
        const bool viewed = rv.gw > 1;
        if (use_lds && ldx == c && r0 < r1 &&
            ((reinterpret_cast<uintptr_t>(x) + (viewed ? (size_t)0 : (size_t)r0 * c * sizeof(T))) & 15) == 0) {
            typedef unsigned u4 __attribute__((ext_vector_type(4)));
            const T *xb = x + r0 * c;
            const int64_t total = (r1 - r0) * c, nvec = total / VEC;
            // (row, channel) of a thread's vector advance by NT*VEC elements per load: no division in the loop
            int64_t vrow = ((int64_t)VEC * tid) / c;
            int vch = (int)((int64_t)VEC * tid - vrow * c);
            const int drow = (NT * VEC) / c, dch = (NT * VEC) % c;
            if (c >= VEC) {
                // A 16-byte vector spans at most two rows: both labels are requested up front, unconditionally (clamped
                // row), and every element picks its own -- no load behind a divergent branch (such a load gets its
                // s_waitcnt right behind it: one serialised L2 round trip per vector, which held this kernel at a
                // quarter of the LDS atomic rate)
                const int64_t last_row = r1 - r0 - 1;
                const bool rows_of_vectors = c % VEC == 0;   // (wave-uniform)
                for (int64_t v0 = tid; v0 < nvec; v0 += 4 * NT) {
                    T val[4][VEC];
                    int lab_a[4], lab_b[4], ch0[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int64_t v = v0 + u * NT;
                        const bool ok = v < nvec;
                        const int64_t row = vrow < last_row ? vrow : last_row, row2 = vrow + 1 < last_row ? vrow + 1 : last_row;
                        const u4 raw = *reinterpret_cast<const u4 *>(viewed ? x + rv.offset(r0 + row, c) + (ok ? vch : 0) : xb + VEC * (ok ? v : nvec - 1));
                        __builtin_memcpy(val[u], &raw, 16);
                        // (rows of whole vectors never look at the second label: its load is the third of every four vector-memory
                        // instructions of this loop)
                        const int la = labels[r0 + row] - 1, lb2 = rows_of_vectors ? -1 : labels[r0 + row2] - 1;
                        lab_a[u] = ok ? la : -1;
                        lab_b[u] = (ok && vrow + 1 <= last_row) ? lb2 : -1;
                        ch0[u] = vch;
                        vrow += drow;
                        vch += dch;
                        if (vch >= c) {
                            vch -= c;
                            vrow++;
                        }
                    }
                    // Round 5: rows of a whole number of vectors (c % VEC == 0: 40 binary16 channels, 100 binary32 columns): a vector lies
                    // in ONE row, so its eight (four) adds go to consecutive words of one table row -- no per-element choice between two
                    // labels, no test for zero (a zero adds nothing), the element's place in the instruction's offset field.  Timing builds
                    // had shown what bounds this kernel: not HBM (0.353 ms of 0.402 without its loads), not the LDS atomics (0.364 without
                    // them), but the dozen vector instructions per ELEMENT around them (profiles/r05/sums_loads_in_flight.txt).
                    if (rows_of_vectors) {
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const bool ok_a = (unsigned)lab_a[u] < (unsigned)k;
                            const int base = ok_a ? lab_a[u] * cs + ch0[u] : k * cs;
                            bool plain = true;
                            if constexpr (TableAdd<T>::kFixed) {
                                unsigned raw[4], reach = 0u;
                                __builtin_memcpy(raw, val[u], 16);
#pragma unroll
                                for (int d = 0; d < 4; d++) reach |= (raw[d] & 0x7fff7fffu) + 0x04000400u;
                                plain = (reach & 0x80008000u) == 0u;   // (no Inf / NaN among the eight)
                                if (plain) {
                                    unsigned long long *tp = reinterpret_cast<unsigned long long *>(ls) + base;
#pragma unroll
                                    for (int i = 0; i < VEC; i++) {
                                        const double shifted = (double)val[u][i] + 0x1.8p+28;
                                        __hip_atomic_fetch_add(tp + i, (unsigned long long)__double_as_longlong(shifted) - 0x41B8000000000000ull,
                                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                    }
                                }
                            } else {
                                if (ok_a) {
                                    double *tp = ls + base;
#pragma unroll
                                    for (int i = 0; i < VEC; i++)
                                        __hip_atomic_fetch_add(tp + i, (double)val[u][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                            }
                            if (plain) {
                                if (ok_a && ch0[u] == 0) atomicAdd(&lc[lab_a[u]], 1u);
                            } else if (ok_a) {
#pragma unroll
                                for (int i = 0; i < VEC; i++) {
                                    TableAdd<T>::add(ls, (size_t)lab_a[u] * cs + ch0[u] + i, val[u][i], sums, (size_t)lab_a[u] * c + ch0[u] + i);
                                    if (ch0[u] + i == 0) atomicAdd(&lc[lab_a[u]], 1u);
                                }
                            }
                        }
                        continue;
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        bool plain = false;
                        if constexpr (TableAdd<T>::kFixed) {
                            // binary16, no Inf / NaN among the eight (the usual vector): branch-free.  v + 1.5 * 2^28 is
                            // exact and lies in [2^28, 2^29), where one ulp is 2^-24: its bit pattern minus the
                            // constant's IS v * 2^24 in two's complement (the constant's low word is zero: one
                            // subtraction on the high word).  Elements without a valid label go to the spare slots.
                            // (an exponent field of all ones <=> magnitude >= 0x7c00 <=> magnitude + 0x0400 reaches bit 15;
                            // both halves of a word at once, no carry between them)
                            unsigned raw[4], reach = 0u;
                            __builtin_memcpy(raw, val[u], 16);
#pragma unroll
                            for (int d = 0; d < 4; d++) reach |= (raw[d] & 0x7fff7fffu) + 0x04000400u;
                            plain = (reach & 0x80008000u) == 0u;
                            if (plain) {
                                const bool ok_a = (unsigned)lab_a[u] < (unsigned)k, ok_b = (unsigned)lab_b[u] < (unsigned)k;
                                const int base_a = ok_a ? lab_a[u] * cs + ch0[u] : k * cs;
                                const int base_b = ok_b ? lab_b[u] * cs + ch0[u] - c : k * cs;
                                unsigned long long *table = reinterpret_cast<unsigned long long *>(ls);
#pragma unroll
                                for (int i = 0; i < VEC; i++) {
                                    const double shifted = (double)val[u][i] + 0x1.8p+28;
                                    const unsigned long long q =
                                        (unsigned long long)__double_as_longlong(shifted) - 0x41B8000000000000ull;
                                    const int slot = (ch0[u] + i >= c ? base_b : base_a) + i;
                                    if (q) __hip_atomic_fetch_add(table + slot, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                                if (ok_a && ch0[u] == 0) atomicAdd(&lc[lab_a[u]], 1u);        // the vector starts a row,
                                if (ok_b && ch0[u] + VEC > c) atomicAdd(&lc[lab_b[u]], 1u);   // or the next row starts inside it
                            }
                        }
                        if (!plain) {
#pragma unroll
                            for (int i = 0; i < VEC; i++) {
                                const bool wrapped = ch0[u] + i >= c;
                                const int lb = wrapped ? lab_b[u] : lab_a[u];
                                const int ch = ch0[u] + i - (wrapped ? c : 0);
                                if (lb >= 0 && lb < k) {
                                    TableAdd<T>::add(ls, (size_t)lb * cs + ch, val[u][i], sums, (size_t)lb * c + ch);
                                    if (ch == 0) atomicAdd(&lc[lb], 1u);
                                }
                            }
                        }
                    }
                }
            } else
            for (int64_t v0 = tid; v0 < nvec; v0 += 4 * NT) {
                T val[4][VEC];
                int lab[4][VEC], chn[4][VEC];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int64_t v = v0 + u * NT;
                    const bool ok = v < nvec;
                    const u4 raw = ok ? *reinterpret_cast<const u4 *>(xb + VEC * v) : u4{0u, 0u, 0u, 0u};
                    __builtin_memcpy(val[u], &raw, 16);
                    int64_t row = vrow;
                    int ch = vch;
                    vrow += drow;
                    vch += dch;
                    if (vch >= c) {
                        vch -= c;
                        vrow++;
                    }
                    int lb = ok ? labels[r0 + row] - 1 : -1;
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        chn[u][i] = ch;
                        lab[u][i] = lb;
                        if (++ch == c) {
                            ch = 0;
                            row++;
                            lb = (ok && r0 + row < r1) ? labels[r0 + row] - 1 : -1;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        const int lb = lab[u][i];
                        if (lb >= 0 && lb < k) {
                            TableAdd<T>::add(ls, (size_t)lb * cs + chn[u][i], val[u][i], sums, (size_t)lb * c + chn[u][i]);
                            if (chn[u][i] == 0) atomicAdd(&lc[lb], 1u);
                        }
                    }
            }
            // the (total % VEC) trailing elements of the range
            for (int64_t e = nvec * VEC + tid; e < total; e += NT) {
                const int64_t row = e / c;
                const int ch = (int)(e - row * c), lb = labels[r0 + row] - 1;
                if (lb >= 0 && lb < k) {
                    TableAdd<T>::add(ls, (size_t)lb * cs + ch, xb[e], sums, (size_t)lb * c + ch);
                    if (ch == 0) atomicAdd(&lc[lb], 1u);
                }
            }
            done = true;
        }
    }
    if (r0 < r1 && !done) {
        // element e of the range <-> (row r0 + e / c, channel e % c); advance by 256 per element,
        // four elements in flight per thread (loads issued before the dependent atomics)
        const int64_t total = (r1 - r0) * c;
        int64_t row = r0 + tid / c;
        int ch = tid % c;
        const int drow = NT / c, dch = NT % c;
        for (int64_t e = tid; e < total; e += 4 * NT) {
            int cc[4], lab[4];
            T v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                cc[u] = ch;
                const bool ok = e + NT * u < total;
                lab[u] = ok ? labels[row] - 1 : -1;
                v[u] = ok ? x[row * ldx + ch] : (T)0;
                row += drow;
                ch += dch;
                if (ch >= c) {
                    ch -= c;
                    row += 1;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if constexpr (sizeof(T) == 8) v[u] = pxsom_bmu::qround(v[u], qmagic);   // binary64 rows of a reproducible run
                if (lab[u] >= 0 && lab[u] < k) {
                    if (use_lds) {
                        TableAdd<T>::add(ls, (size_t)lab[u] * cs + cc[u], v[u], sums, (size_t)lab[u] * c + cc[u]);
                        if (cc[u] == 0) atomicAdd(&lc[lab[u]], 1u);
                    } else {
                        __hip_atomic_fetch_add(&sums[(size_t)lab[u] * c + cc[u]], (double)v[u], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                        if (cc[u] == 0) {
                            if constexpr (COUNT_F64)
                                __hip_atomic_fetch_add(reinterpret_cast<double *>(counts) + lab[u], 1.0, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
                            else
                                atomicAdd(&counts[lab[u]], 1ull);
                        }
                    }
                }
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        int node = tid / c, j = tid - node * c;   // element e <-> (node, channel), advanced without a division per element
        const int dnode = NT / c, dj = NT % c;
        for (int e = tid; e < k * c; e += NT) {
            const double v = TableAdd<T>::value(ls, (size_t)node * cs + j);
            if (v != 0.0) __hip_atomic_fetch_add(&sums[e], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            node += dnode;
            j += dj;
            if (j >= c) {
                j -= c;
                node++;
            }
        }
        for (int e = tid; e < k; e += NT)
            if (lc[e]) {
                if constexpr (COUNT_F64)
                    __hip_atomic_fetch_add(reinterpret_cast<double *>(counts) + e, (double)lc[e], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                else
                    atomicAdd(&counts[e], (unsigned long long)lc[e]);
            }
    }
}

// ------------------------------------------------------------------------------------------------
// per-cluster sums, wave-private tables: LDS binary64 atomics retire about one lane per clock per CU, which
// holds the atomic kernel above at ~2.5 TB/s.  Here every wave owns a [k + 1, c] table in LDS and updates
// it with plain read / add / write: RPI = 64 / c rows per instruction, lane <-> (row slot, channel), so the
// lanes of one instruction touch distinct words unless two of its rows carry the same label.  Two groups
// (2 * RPI rows, a "unit") are applied together -- both reads, both adds, both writes -- when no label
// repeats inside the unit; the test is one ballot per 64 labels (each lane compares its row's label with
// the others of its unit), read per unit as a few bits of a scalar mask.  A unit with a repeat is applied
// row by row.  LDS executes a wave's accesses in order, so the writes of one unit precede the reads of
// the next without any wait.  Rows outside [ra, rb) and labels outside 1..k go to the spare row k; lanes
// past RPI * c to spare words behind the table.
// Loads: one tile (RPI * U rows) ahead, each value register re-issued for the next tile right after its
// use (U dword buffer loads in flight per lane, scalar group offset); labels two tiles ahead.  Measured
// (10x10 x 22, 4.2 M float32 rows): 110 us against 160 us for the atomic kernel; the load stream alone
// runs at ~4.7 TB/s in this one-dword-per-lane shape (82 us), the table updates add the rest.
// ------------------------------------------------------------------------------------------------
template <typename T, int RPI, bool COUNT_F64>
__global__ __launch_bounds__(256) void cluster_sums_private_kernel(const T *__restrict__ x, int64_t n, int c,
                                                                   int64_t ldx,
                                                                   const int32_t *__restrict__ labels, int k,
                                                                   double *sums, unsigned long long *counts,
                                                                   int64_t rows_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int U = sizeof(T) == 8 ? 16 : 32;  // groups per tile == loads in flight per lane (56: no gain)
    constexpr int TR = RPI * U;                  // rows per tile (<= 128)
    constexpr int SG = 2 * RPI;                  // rows of two groups: the unit whose labels are compared
    constexpr int RL = 64 / SG * SG;             // rows per label register (whole units)
    constexpr int NL = (TR + RL - 1) / RL;       // label registers per tile
    const int tid = threadIdx.x, bd = blockDim.x, lane = tid & 63, nwv = bd >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // keeps the row arithmetic on the scalar unit
    const int tstride = (k + 1) * c + 64;        // doubles per wave table
    double *all = reinterpret_cast<double *>(smem_raw);
    double *tbl = all + (size_t)wv * tstride;
    unsigned *cnt = reinterpret_cast<unsigned *>(all + (size_t)nwv * tstride);  // [k], shared by the waves
    for (int e = tid; e < nwv * tstride; e += bd) all[e] = 0.0;
    for (int e = tid; e < k; e += bd) cnt[e] = 0u;
    __syncthreads();

    const int slot = lane / c, ch = lane - slot * c;
    const bool active = slot < RPI;
    const unsigned lane_off = active ? (unsigned)((slot * ldx + ch) * (int64_t)sizeof(T)) : 0u;  // bytes
    const int spare = (k + 1) * c + lane;  // lanes past RPI * c: a word of their own behind the table
    const int64_t gw = (int64_t)blockIdx.x * nwv + wv;
    const int64_t ra = gw * rows_per_wave;
    const int64_t rb = ra + rows_per_wave < n ? ra + rows_per_wave : n;
    if (ra < rb) {  // wave-uniform
        // Whole groups end at row `lim` (relative to ra); the (n - ra) % RPI rows behind it (last wave only)
        // are added one by one.  Every load is unconditional with a clamped, wave-uniform row (groups past
        // the end re-read the rows at `safe`): a load behind a branch costs an s_waitcnt vmcnt(0) per group.
        const int span = (int)(rb - ra), lim = span - span % RPI;
        const int last = (int)(n - 1 - ra);  // last row of the matrix, relative
        // buffer loads: wave-uniform descriptor + 32-bit lane offset + scalar group offset (no 64-bit
        // address arithmetic per load).  The launcher keeps a wave's byte range below 2^31.
        const unsigned gstep = (unsigned)(RPI * ldx * (int64_t)sizeof(T));  // bytes from one group to the next
        const unsigned safe = (unsigned)((ra + RPI <= n ? 0 : n - RPI - ra) * ldx * (int64_t)sizeof(T));
        const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<T *>(x + ra * ldx), 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t lres = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<int32_t *>(labels + ra), 0, 0x7fffffff, 0x00020000);
        auto load_labels = [&](int rel0, int(&lv)[NL]) {
#pragma unroll
            for (int i = 0; i < NL; i++) {
                const int r = rel0 + i * RL + lane;
                const int lb = __builtin_amdgcn_raw_buffer_load_b32(lres, (r < last ? r : last) * 4, 0, 0) - 1;
                // '&', not '&&': a short-circuit lets the compiler sink the load into a branch
                const bool ok = (r < lim) & (lane < RL) & (i * RL + lane < TR) & ((unsigned)lb < (unsigned)k);
                lv[i] = ok ? lb : k;
            }
        };
        auto load_val = [&](int rel, unsigned off) -> T {  // group at relative row rel, byte offset off
            const unsigned so = rel + RPI <= lim ? off : safe;
            if constexpr (sizeof(T) == 8) {
                typedef unsigned u2 __attribute__((ext_vector_type(2)));
                const u2 raw = __builtin_amdgcn_raw_buffer_load_b64(xres, lane_off, so, 0);
                return __builtin_bit_cast(T, raw);
            } else if constexpr (sizeof(T) == 4) {
                return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(xres, lane_off, so, 0));
            } else {
                return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(xres, lane_off, so, 0));
            }
        };
        // labels shared inside a unit of 2 groups: such a unit is applied row by row
        auto clash_mask = [&](int lab) -> unsigned long long {
            const int base = lane / SG * SG, pos = lane - base;
            bool cl = false;
#pragma unroll
            for (int d = 1; d < SG; d++) {
                const int p = pos + d < SG ? pos + d : pos + d - SG;
                cl = cl | (__shfl(lab, base + p) == lab);  // every lane takes part in every exchange
            }
            return __ballot(cl && lab != k && lane < RL);
        };
        T val[U];
        // labels travel two tiles ahead and are requested BEFORE the tile's value loads, so waiting for
        // them never drains the value loads behind them (vmcnt counts in issue order)
        int lv_cur[NL], lv_nxt[NL], lv_far[NL];
        load_labels(0, lv_cur);
        load_labels(TR, lv_nxt);
        {
            unsigned off = 0;
#pragma unroll
            for (int g = 0; g < U; g++, off += gstep) val[g] = load_val(g * RPI, off);
        }
        // byte address of this lane's word in the table row of a label: tbl + (label * c + ch) * 8
        char *const lane_word = reinterpret_cast<char *>(tbl) + (active ? ch : spare) * 8;
        unsigned tile_off = TR * gstep / RPI;  // byte offset of the next tile
        for (int rel0 = 0; rel0 < lim; rel0 += TR, tile_off += TR * gstep / RPI) {
            load_labels(rel0 + 2 * TR, lv_far);
            unsigned long long cm[NL];
            int row_bytes[NL];  // label * c * 8 of the rows this lane holds
#pragma unroll
            for (int i = 0; i < NL; i++) {
                if (lv_cur[i] < k) atomicAdd(&cnt[lv_cur[i]], 1u);
                cm[i] = clash_mask(lv_cur[i]);
                row_bytes[i] = (int)__umul24(lv_cur[i], c * 8);
            }
            // every group's table address for this lane, one exchange each, all issued before the first use
            int word[U];
#pragma unroll
            for (int g = 0; g < U; g++) {
                const int r = g * RPI;
                const int rb8 = __shfl(row_bytes[r / RL], r % RL + slot);
                word[g] = active ? rb8 : 0;
            }
            unsigned off = tile_off;
#pragma unroll
            for (int g = 0; g < U; g += 2) {
                double *const w0 = reinterpret_cast<double *>(lane_word + word[g]);
                double *const w1 = reinterpret_cast<double *>(lane_word + word[g + 1]);
                const double v0 = (double)val[g], v1 = (double)val[g + 1];
                val[g] = load_val(rel0 + TR + g * RPI, off);  // these registers' loads for the next tile
                val[g + 1] = load_val(rel0 + TR + (g + 1) * RPI, off + gstep);
                off += 2 * gstep;
                if (!((cm[g * RPI / RL] >> (g * RPI % RL)) & ((1ull << SG) - 1))) {  // no row of the unit flagged
                    const double a = *w0, b = *w1;
                    *w0 = a + v0;
                    *w1 = b + v1;
                } else {
                    // one row at a time.  The fences keep the predicated updates apart: to the compiler they are
                    // mutually exclusive branches of one thread, which it may fold into a single update
#pragma unroll
                    for (int s = 0; s < RPI; s++) {
                        if (slot == s) *w0 += v0;
                        __builtin_amdgcn_wave_barrier();
                        asm volatile("" ::: "memory");
                    }
#pragma unroll
                    for (int s = 0; s < RPI; s++) {
                        if (slot == s) *w1 += v1;
                        __builtin_amdgcn_wave_barrier();
                        asm volatile("" ::: "memory");
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NL; i++) {
                lv_cur[i] = lv_nxt[i];
                lv_nxt[i] = lv_far[i];
            }
        }
        for (int64_t r = ra + lim; r < rb; r++) {  // fewer than RPI rows
            const int lb = labels[r] - 1;
            if ((unsigned)lb < (unsigned)k) {
                if (lane < c) tbl[lb * c + lane] += (double)x[r * ldx + lane];
                if (lane == 0) atomicAdd(&cnt[lb], 1u);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < k * c; e += bd) {
        double v = 0.0;
        for (int w = 0; w < nwv; w++) v += all[(size_t)w * tstride + e];
        if (v != 0.0) __hip_atomic_fetch_add(&sums[e], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int e = tid; e < k; e += bd)
        if (cnt[e]) {
            if constexpr (COUNT_F64)
                __hip_atomic_fetch_add(reinterpret_cast<double *>(counts) + e, (double)cnt[e], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            else
                atomicAdd(&counts[e], (unsigned long long)cnt[e]);
        }
}

// wave-private form when c <= 64 and at least one wave's table fits the CU; *handled says whether it ran
template <typename T, int RPI, bool COUNT_F64>
int launch_sums_private(const T *x, int64_t n, int c, int64_t ldx, const int32_t *labels, int k, double *sums,
                        int64_t *counts, hipStream_t st, int nwv, int blocks_per_cu)
{
    const size_t tbytes = ((size_t)(k + 1) * c + 64) * 8;
    const size_t lds = tbytes * nwv + (size_t)k * 4;
    constexpr int TR = RPI * (sizeof(T) == 8 ? 16 : 32);
    const int64_t max_waves = (int64_t)pxsom::device_cu_count() * blocks_per_cu * nwv;
    // every wave gets whole tiles, and enough of them to pay for its share of the final merge
    int64_t rows_per_wave = (n + max_waves - 1) / max_waves;
    if (rows_per_wave < 8 * TR) rows_per_wave = 8 * TR;
    rows_per_wave = (rows_per_wave + TR - 1) / TR * TR;
    const int64_t waves = (n + rows_per_wave - 1) / rows_per_wave;
    const int64_t grid = (waves + nwv - 1) / nwv;
    auto kern = cluster_sums_private_kernel<T, RPI, COUNT_F64>;
    if (lds > 48 * 1024)
        PXSOM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * nwv), lds, st, x, n, c, ldx, labels, k, sums,
                       reinterpret_cast<unsigned long long *>(counts), rows_per_wave);
    PXSOM_LAUNCH_CHECK("cluster_sums_private_kernel");
    return PXSOM_OK;
}

// Wave-private tables (cluster_sums_private_kernel, the pairs kernel): how many waves of a workgroup get one (0: the shape has no
// such route) and how many workgroups a CU holds.
inline int sums_private_waves(int c, int k, int *per_cu_out = nullptr)
{
    int nwv = 0, per_cu = 1;
    if (c >= 13 && c <= 64) {
        const size_t tbytes = ((size_t)(k + 1) * c + 64) * 8, budget = 160 * 1024 - 1024;
        if (8 * tbytes + (size_t)k * 8 <= budget) nwv = 4, per_cu = 2;
        else if (4 * tbytes + (size_t)k * 4 <= budget) nwv = 4;
        else if (2 * tbytes + (size_t)k * 4 <= budget) nwv = 2;
    }
    if (per_cu_out) *per_cu_out = per_cu;
    return nwv;
}

}  // namespace

namespace pxsom {

// The shapes whose sums kernel reads a scheduled step's rows where they lie (pxsom::RowView): cluster_sums_kernel's flat route
// with rows of whole 16-byte vectors -- binary32 / binary16 rows, contiguous in the caller's matrix, table in LDS -- and no
// wave-private route for the shape (those kernels address flat ranges; large inputs of 13 - 64 channels go there when their tables
// fit: config 5's 400 x 40 table does not).
template <typename T>
bool sums_take_views(const T *x, int c, int64_t ldx, int k)
{
    if (sizeof(T) > 4) return false;
    const int vec = 16 / (int)sizeof(T);
    const size_t lds_odd = ((size_t)k * (c | 1) + kSumsSpare) * 8 + (size_t)k * 4;
    return sums_private_waves(c, k) == 0 && c >= vec && c % vec == 0 && ldx == c && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
           std::min(lds_odd, ((size_t)k * c + kSumsSpare) * 8 + (size_t)k * 4) <= 150 * 1024;
}

// qmagic != 0 (binary64 rows of a reproducible training run, include/pxsom.h): values are rounded to the run's quantum
// as they are added; only the atomic kernel knows how.
template <typename T, bool COUNT_F64>
int cluster_sums_typed(const T *x, int64_t n, int c, int64_t ldx, const int32_t *labels, int k, double *sums,
                       int64_t *counts, hipStream_t st, double qmagic)
{
    if (sizeof(T) != 8) qmagic = 0.0;
    if (pxsom::row_view_active() && !sums_take_views<T>(x, c, ldx, k))
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "cluster sums: a row view on a shape whose kernel does not take views");
    // wave-private tables (see cluster_sums_private_kernel): 13 <= c <= 64 (RPI = 64 / c <= 4 rows per
    // instruction, fewer idle lanes than channels), at least two tables per CU, an input big enough to
    // fill them, and a wave's byte range addressable by the 32-bit buffer offsets.  Measured against the
    // atomic kernel below on 2-4 M rows: 1.4-1.9x faster there, slower outside (c <= 8, one table per CU).
    if (c >= 13 && c <= 64 && n >= 32768 && qmagic == 0.0) {
        int per_cu = 1;
        const int nwv = sums_private_waves(c, k, &per_cu);
        const int64_t waves = (int64_t)pxsom::device_cu_count() * per_cu * (nwv ? nwv : 1);
        const bool addressable = ((n + waves - 1) / waves + 1024) * ldx * (int64_t)sizeof(T) < (1ll << 31);
        if (nwv && addressable) {
            // two channels per lane where the rows allow pair loads (pxsom_sums.hip): 2.5x fewer instructions per row
            if (pxsom::launch_sums_pairs<T>(x, n, c, ldx, labels, k, sums, counts, COUNT_F64, st, nwv, per_cu)) {
                PXSOM_LAUNCH_CHECK("cluster_sums_pairs_kernel");
                return PXSOM_OK;
            }
            switch (64 / c) {
                case 1: return launch_sums_private<T, 1, COUNT_F64>(x, n, c, ldx, labels, k, sums, counts, st, nwv, per_cu);
                case 2: return launch_sums_private<T, 2, COUNT_F64>(x, n, c, ldx, labels, k, sums, counts, st, nwv, per_cu);
                case 3: return launch_sums_private<T, 3, COUNT_F64>(x, n, c, ldx, labels, k, sums, counts, st, nwv, per_cu);
                default: return launch_sums_private<T, 4, COUNT_F64>(x, n, c, ldx, labels, k, sums, counts, st, nwv, per_cu);
            }
        }
    }
    // table row stride: odd when the padded table still fits (bank spread of the LDS atomics), else c
    const size_t lds_odd = ((size_t)k * (c | 1) + kSumsSpare) * 8 + (size_t)k * 4;
    const int cs = lds_odd <= 150 * 1024 ? (c | 1) : c;
    const size_t lds = ((size_t)k * cs + kSumsSpare) * 8 + (size_t)k * 4;
    const int use_lds = lds <= 150 * 1024;
    const int cus = pxsom::device_cu_count();
    // small inputs are latency-bound per workgroup, so they are spread wide: 64 rows per workgroup (measured on
    // config 4's 15.6 K-row training steps, ms per 64-step pass: 32 rows 6.09, 64 rows 5.86, 128 rows 6.08, 512 rows 9.5)
    constexpr int rows_per_wg = 64;
    const int wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (size_t)(158 * 1024) / std::max<size_t>(lds, 1)));
    int64_t grid = std::min<int64_t>((n + rows_per_wg - 1) / rows_per_wg, (int64_t)cus * wg_per_cu);
    if (grid < 1) grid = 1;
    // (multiples of 16 rows keep every workgroup's range 16-byte aligned for the vector loads)
    const int64_t rows_per_block = ((n + grid - 1) / grid + 15) / 16 * 16;
    // one table per CU (K = 400 x C = 40: 128 KB): 16 waves share it, so that enough loads and LDS atomics are in
    // flight; small tables keep 4-wave workgroups (several per CU)
    const bool wide = use_lds && lds > 64 * 1024 && n >= 65536;
    auto kern = wide ? cluster_sums_kernel<T, COUNT_F64, 1024> : cluster_sums_kernel<T, COUNT_F64, 256>;
    if (use_lds && lds > 48 * 1024)
        PXSOM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(wide ? 1024 : 256), use_lds ? lds : 0, st, x, n, c, ldx, labels, k,
                       sums, reinterpret_cast<unsigned long long *>(counts), rows_per_block, use_lds, qmagic, cs, pxsom::current_row_view());
    PXSOM_LAUNCH_CHECK("cluster_sums_kernel");
    return PXSOM_OK;
}

#define PXSOM_INSTANTIATE_SUMS(T)                                                                                              \
    template bool sums_take_views<T>(const T *, int, int64_t, int);                                                            \
    template int cluster_sums_typed<T, false>(const T *, int64_t, int, int64_t, const int32_t *, int, double *, int64_t *,     \
                                              hipStream_t, double);                                                            \
    template int cluster_sums_typed<T, true>(const T *, int64_t, int, int64_t, const int32_t *, int, double *, int64_t *,      \
                                             hipStream_t, double);
PXSOM_INSTANTIATE_SUMS(float)
PXSOM_INSTANTIATE_SUMS(double)
PXSOM_INSTANTIATE_SUMS(_Float16)
#undef PXSOM_INSTANTIATE_SUMS

}  // namespace pxsom

PXSOM_EXPORT int pxsom_cluster_sums(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype,
                                    const int32_t *labels_dev, int k, double *sums_dev, int64_t *counts_dev,
                                    void *stream)
{
    int rc = pxsom::check_matrix("pxsom_cluster_sums", x_dev, n, c, ldx, dtype);
    if (rc) return rc;
    if (k < 1 || k > PXSOM_MAX_NODES)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_cluster_sums: k=%d outside [1, %d]", k, PXSOM_MAX_NODES);
    if (!sums_dev || !counts_dev || (n > 0 && !labels_dev))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_cluster_sums: null pointer");
    if (n == 0) return PXSOM_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_DISPATCH_DTYPE(dtype, x_dev, xp, pxsom::cluster_sums_typed<T>(xp, n, c, ldx, labels_dev, k, sums_dev, counts_dev, st));
}

// cell x pixel-cluster counts (create_c2pc_data's groupby + pivot): plain global int64 atomics.  The bins
// of one cell are nb consecutive words and neighbouring pixels mostly belong to the same cell, so the
// atomics of a wave land in a few cache lines; the kernel is bound by reading the two label vectors.
__global__ __launch_bounds__(256) void pair_histogram_kernel(const int32_t *__restrict__ a,
                                                             const int32_t *__restrict__ b, int64_t n,
                                                             int64_t na, int nb, unsigned long long *hist)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t ai = a[i], bi = b[i];
        if (ai >= 0 && ai < na && bi >= 0 && bi < nb) atomicAdd(&hist[(int64_t)ai * nb + bi], 1ull);
    }
}

PXSOM_EXPORT int pxsom_pair_histogram(const int32_t *a_dev, const int32_t *b_dev, int64_t n, int64_t na, int nb,
                                      int64_t *hist_dev, void *stream)
{
    if (n < 0 || na < 1 || nb < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_pair_histogram: bad sizes");
    if (!hist_dev || (n > 0 && (!a_dev || !b_dev)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_pair_histogram: null pointer");
    if (n == 0) return PXSOM_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t grid = std::min<int64_t>((n + 255) / 256, (int64_t)pxsom::device_cu_count() * 16);
    hipLaunchKernelGGL(pair_histogram_kernel, dim3((unsigned)grid), dim3(256), 0, st, a_dev, b_dev, n, na, nb,
                       reinterpret_cast<unsigned long long *>(hist_dev));
    PXSOM_LAUNCH_CHECK("pair_histogram_kernel");
    return PXSOM_OK;
}
