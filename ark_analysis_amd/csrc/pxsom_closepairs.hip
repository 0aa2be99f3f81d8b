// pxsom_closepairs.hip -- close-pair counts between cell sets, straight from the centroids (K20).
//
// reference: ark/analysis/spatial_analysis_utils.py compute_close_cell_num over the float32 distance matrix that
// calc_dist_matrix writes (per pair of markers or phenotypes (j, k): the matrix binarised with < dist_lim and > 0,
// subset to the rows positive for j and the columns positive for k, summed), and the target / reference interaction
// totals of ark/analysis/neighborhood_analysis.py compute_mixing_score.  A cell may sit in many sets at once, so a set is
// a bit of a 64-bit membership mask.  For every FOV f
//   out[f, s, t] = #{ordered pairs (a, b) of cells of f : bit s of member_q[a], bit t of member_c[b], the pair counts}
// with K13's pair test, pair_is_close of pxsom_fovwalk.h.  Neither the N x N matrix nor an N x sets table is built.
//
// Shape.  for_each_fov of pxsom_fovwalk.h (one thread one query cell, a workgroup of 256 owns 256 consecutive rows and
// visits every FOV those rows touch), the FOV's cells as candidates in tiles of 256 staged in LDS, every lane reading the
// same candidate, with the set arithmetic bit-sliced so that it stays out of the loop over candidates:
//   - at staging each wave transposes the masks of its 64 candidates with one ballot per column set: cplane[t] is the
//     64-bit word that says which of the 64 candidates are in set t (bits at or above n_sets_c are never looked at);
//   - the loop over 64 candidates only gathers the lane's 64 pair tests into a 64-bit word `close`;
//   - then count[t] += popcount(close & cplane[t]) for every column set: four 32-bit integer operations per set per 64
//     candidates, the counters in registers (the kernel is instantiated for up to 8, 32 and 64 column sets);
//   - when the FOV's walk ends the lanes put their counters into LDS rows (odd stride) and one ballot per row set gives
//     qplane[s], the lanes of the workgroup that are cells of this FOV in set s; wave w sums, for s = w, w + 4, ... and
//     one column per lane, the rows named by qplane[s], and adds what is not zero to out with a 64-bit integer atomic.
// Per-lane counters are 32-bit (at most the cells of a FOV; the entry refuses n >= 2^31), the sums over lanes and out are
// 64-bit.  Integer additions only, so out does not depend on the grid or on the order of the atomics.
//
// Memory safety: the argument of pxsom_fovwalk.h for the cell arrays; every index into out is built from f < n_fovs,
// s < n_sets_q and t < n_sets_c, and mask bits above the set counts select nothing.
#include "pxsom_common.h"
#include "pxsom_fovwalk.h"

namespace {

constexpr int kWaves = kBlock / kWave;
constexpr int kMaxSets = 64;

// NCAP: how many column-set counters a lane keeps (n_sets_c <= NCAP).  The counters go to LDS CB columns at a time.
template <bool SELF, int NCAP>
__global__ __launch_bounds__(kBlock) void close_pair_counts_kernel(const double2 *__restrict__ xy,
                                                                   const unsigned long long *__restrict__ member_q,
                                                                   const unsigned long long *__restrict__ member_c,
                                                                   const int64_t *__restrict__ seg, int64_t n_fovs,
                                                                   int64_t n, int n_sets_q, int n_sets_c, double s_lim,
                                                                   double s_zero, unsigned long long *__restrict__ out)
{
    constexpr int CB = NCAP < 32 ? NCAP : 32;   // columns per pass of the reduction
    constexpr int STRIDE = CB + 1;              // odd: lane l writes word l * STRIDE + j, one bank per lane
    constexpr int PARTS = kWave / CB;           // a wave's lanes split the 256 rows into PARTS groups, CB columns each
    constexpr int WORDS = 8 / PARTS;            // 32-bit words of a query plane per group (8 words name 256 rows)
    constexpr int PASSES = (NCAP + CB - 1) / CB;
    static_assert(NCAP % 8 == 0 && NCAP <= kMaxSets && kWave % CB == 0 && 8 % PARTS == 0, "close_pair_counts layout");

    __shared__ double2 cand[kBlock];
    __shared__ unsigned long long cplane[kWaves * kMaxSets];   // [wave of candidates][column set]
    __shared__ uint32_t qplane[kMaxSets * 8];                  // [row set][32 rows of the workgroup per word]
    __shared__ uint32_t sums[kBlock * STRIDE];

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid / kWave;
    const BlockRows rows = load_block_rows(xy, n);
    const double xi = rows.xi, yi = rows.yi;
    const unsigned long long mq = rows.has_row ? member_q[rows.i] : 0ull;

    for_each_fov(seg, n_fovs, n, rows,
                 [&](int64_t f, int64_t beg, int64_t end, bool mine) __attribute__((always_inline)) {
        uint32_t count[NCAP];
#pragma unroll
        for (int t = 0; t < NCAP; ++t) count[t] = 0u;

        for (int64_t base = beg; base < end; base += kBlock) {
            const int tile_n = end - base < kBlock ? (int)(end - base) : kBlock;
            __syncthreads();   // the previous tile, and the previous FOV's reduction, have been read
            double2 c = make_double2(0.0, 0.0);
            unsigned long long m = 0ull;   // past the tile's end: in no set
            if (tid < tile_n) {
                c = xy[base + tid];
                m = member_c[base + tid];
            }
            cand[tid] = c;
            unsigned long long plane = 0ull;
            for (int t = 0; t < n_sets_c; ++t) {
                const unsigned long long b = __ballot((int)((m >> t) & 1ull));
                if (lane == t) plane = b;
            }
            cplane[wave * kMaxSets + lane] = plane;   // zero for the lanes at or above n_sets_c
            __syncthreads();

            for (int w0 = 0; w0 < tile_n; w0 += kWave) {
                const double2 *cc = cand + w0;
                uint32_t close_lo = 0u, close_hi = 0u;
#pragma unroll
                for (int k = 0; k < 32; ++k)
                    close_lo |= (uint32_t)pair_is_close<SELF>(xi, yi, cc[k], s_lim, s_zero) << k;
#pragma unroll
                for (int k = 0; k < 32; ++k)
                    close_hi |= (uint32_t)pair_is_close<SELF>(xi, yi, cc[32 + k], s_lim, s_zero) << k;
                const unsigned long long *pl = cplane + (w0 / kWave) * kMaxSets;
#pragma unroll
                for (int g = 0; g < NCAP; g += 8) {
                    if (g < n_sets_c) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const unsigned long long p = pl[g + j];
                            count[g + j] += __popc(close_lo & (uint32_t)p) + __popc(close_hi & (uint32_t)(p >> 32));
                        }
                    }
                }
            }
        }

        // which lanes of this wave are cells of the FOV in row set s: lane s keeps the word
        uint32_t q_lo = 0u, q_hi = 0u;
        for (int s = 0; s < n_sets_q; ++s) {
            const unsigned long long b = __ballot((int)(mine && ((mq >> s) & 1ull)));
            if (lane == s) {
                q_lo = (uint32_t)b;
                q_hi = (uint32_t)(b >> 32);
            }
        }
        qplane[lane * 8 + wave * 2] = q_lo;
        qplane[lane * 8 + wave * 2 + 1] = q_hi;

        const int col0 = lane % CB;
        const int part = lane / CB;
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            if (pass * CB < n_sets_c) {
                if (pass > 0) __syncthreads();   // the pass before has been summed
#pragma unroll
                for (int j = 0; j < CB; ++j) sums[tid * STRIDE + j] = count[pass * CB + j];
                __syncthreads();
                const int col = pass * CB + col0;
                for (int s = wave; s < n_sets_q; s += kWaves) {
                    unsigned long long sum = 0ull;
                    for (int wi = part * WORDS; wi < (part + 1) * WORDS; ++wi) {
                        uint32_t bits = qplane[s * 8 + wi];
                        while (bits) {
                            const int a = __builtin_ctz(bits);
                            bits &= bits - 1u;
                            sum += sums[(wi * 32 + a) * STRIDE + col0];
                        }
                    }
                    if (col < n_sets_c && sum != 0ull)
                        atomicAdd(out + ((size_t)f * n_sets_q + s) * n_sets_c + col, sum);
                }
            }
        }
    });
}

template <bool SELF, int NCAP>
void launch(unsigned blocks, hipStream_t st, const double2 *xy, const unsigned long long *mq,
            const unsigned long long *mc, const int64_t *seg, int64_t n_fovs, int64_t n, int nq, int nc, double s_lim,
            double s_zero, unsigned long long *out)
{
    hipLaunchKernelGGL((close_pair_counts_kernel<SELF, NCAP>), dim3(blocks), dim3(kBlock), 0, st, xy, mq, mc, seg, n_fovs,
                       n, nq, nc, s_lim, s_zero, out);
}

}  // namespace

PXSOM_EXPORT int pxsom_close_pair_counts(const double *xy_dev, const uint64_t *member_q_dev,
                                         const uint64_t *member_c_dev, const int64_t *seg_dev, int64_t n_fovs, int64_t n,
                                         int n_sets_q, int n_sets_c, double s_lim, double s_zero, int self_neighbor,
                                         int64_t *out_dev, void *stream)
{
    const char *fn = "pxsom_close_pair_counts";
    if (n < 0 || n_fovs < 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld, n_fovs=%lld", fn, (long long)n, (long long)n_fovs);
    if (n_sets_q < 1 || n_sets_q > kMaxSets || n_sets_c < 1 || n_sets_c > kMaxSets)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_sets_q=%d, n_sets_c=%d outside 1 .. %d", fn, n_sets_q, n_sets_c, kMaxSets);
    if (const int rc = check_pair_test(fn, self_neighbor, s_lim, s_zero)) return rc;
    if (n > 0x7fffffffLL) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld too large", fn, (long long)n);
    if (n_fovs > (int64_t)1 << 40) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_fovs=%lld too large", fn, (long long)n_fovs);
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null seg", fn);
    if (n_fovs == 0) return PXSOM_OK;   // out is empty
    if (!out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
    if (n > 0) {
        if (!xy_dev || !member_q_dev || !member_c_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
        if (reinterpret_cast<uintptr_t>(xy_dev) % sizeof(double2) != 0)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: xy is not 16-byte aligned", fn);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PXSOM_HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)n_fovs * n_sets_q * n_sets_c * sizeof(int64_t), st));
    if (n == 0) return PXSOM_OK;
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
    const double2 *xy = reinterpret_cast<const double2 *>(xy_dev);
    const unsigned long long *mq = reinterpret_cast<const unsigned long long *>(member_q_dev);
    const unsigned long long *mc = reinterpret_cast<const unsigned long long *>(member_c_dev);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(out_dev);
#define PXSOM_CLOSE_PAIRS(SELF)                                                                                       \
    do {                                                                                                              \
        if (n_sets_c <= 8) launch<SELF, 8>(blocks, st, xy, mq, mc, seg_dev, n_fovs, n, n_sets_q, n_sets_c, s_lim, s_zero, out);       \
        else if (n_sets_c <= 32) launch<SELF, 32>(blocks, st, xy, mq, mc, seg_dev, n_fovs, n, n_sets_q, n_sets_c, s_lim, s_zero, out); \
        else launch<SELF, 64>(blocks, st, xy, mq, mc, seg_dev, n_fovs, n, n_sets_q, n_sets_c, s_lim, s_zero, out);                      \
    } while (0)
    if (self_neighbor) PXSOM_CLOSE_PAIRS(true); else PXSOM_CLOSE_PAIRS(false);
#undef PXSOM_CLOSE_PAIRS
    PXSOM_LAUNCH_CHECK("close_pair_counts_kernel");
    return PXSOM_OK;
}
