// pxsom_celldist.hip -- per cell, the mean float32 distance to its k nearest cells of every phenotype (K14).
//
// reference: ark/analysis/cell_neighborhood_stats.py calculate_mean_distance_to_cell_type over the float32 distance matrix
// that calc_dist_matrix writes: the columns of one phenotype, where(dist > 0), a sort of every row, the mean of its first
// k entries (NaN when fewer than k are left).  That matrix is never built here.  For a query cell i and a candidate j of
// the same FOV and of type t
//   s = fl(fl(dx * dx) + fl(dy * dy))            (binary64, one IEEE operation per statement, no contraction)
// as in pxsom_neighbors.hip; j counts when s > s_zero (float32(sqrt(s)) != 0, som_device.neighbor_thresholds).  sqrt and
// the cast are monotone, so the k smallest distances are those of the k smallest s: the selection runs on s, and only the
// k survivors of a (cell, type) pair see a square root.
//
// Shape.  pxsom_neighbors.hip's, with the run's counter joined by a sorted list: one thread owns one query cell, a
// workgroup of 256 owns 256 consecutive rows and walks every FOV they touch, 256 candidates at a time staged in LDS and
// read as broadcasts; the candidates of a FOV come sorted by type, so a type is one run whose wave-uniform boundaries come
// from one ballot per wave at staging time.  The list is L binary64 registers (L = 8, 16 or 32, the smallest that holds
// k), ascending, the k live entries at the TOP (a[L - k .. L - 1], +inf until filled) over L - k entries pinned at -inf:
// the k-th smallest so far is always a[L - 1], a static register, and one compare against it rejects the common
// candidate.  An insertion is a[j] = max(a[j - 1], min(a[j], s)) for every j (the pinned entries stay -inf by the same
// formula), all indices static: no scratch.  When the run ends the live entries are shifted to a[0 .. k - 1] by a
// log-step shifter under wave-uniform conditions, mapped to float32(sqrt(s)), summed in float32 in the order numpy's
// pairwise row reduction uses, and divided by float32(k).
//
// Memory safety does not depend on the device-side inputs: FOV offsets are clamped to [0, n], and a type outside
// [0, n_types) or out of order is never stored (its row is then wrong, not its neighbours' memory).
#include "pxsom_common.h"

namespace {

constexpr int kBlock = 256;   // threads per workgroup = query rows per workgroup = candidates per tile
constexpr int kWave = 64;
constexpr int kMaxK = 32;     // the largest list instantiated below

struct MeanRowWriter {
    float *row;     // out + i * n_types; touched only when `live`
    int n_types;
    int next;       // columns [0, next) are written
    bool live;

    // NaN for [next, t) (types the FOV lacks), then `v` at column t; t is the same for every lane
    __device__ __forceinline__ void put(int t, float v)
    {
        if (!live || t < next || t >= n_types) return;
        for (int u = next; u < t; ++u) row[u] = __builtin_nanf("");
        row[t] = v;
        next = t + 1;
    }
    __device__ __forceinline__ void finish()
    {
        if (!live) return;
        for (int u = next; u < n_types; ++u) row[u] = __builtin_nanf("");
        next = n_types;
    }
};

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ double squared_distance(double xi, double yi, double2 cj)
{
#pragma clang fp contract(off)
    const double dx = xi - cj.x;
    const double dy = yi - cj.y;
    const double px = dx * dx;
    const double py = dy * dy;
    return px + py;
}

// The k smallest s of a run, ascending in a[L - k .. L - 1]; a[0 .. L - k - 1] stay -inf.  Every index is static.
template <int L>
struct NearestList {
    double a[L];

    __device__ __forceinline__ void reset(int k)
    {
#pragma unroll
        for (int j = 0; j < L; ++j) a[j] = j < L - k ? -__builtin_inf() : __builtin_inf();
    }
    __device__ __forceinline__ double kth() const { return a[L - 1]; }
    // s < kth(): s enters, the largest leaves
    __device__ __forceinline__ void insert(double s)
    {
#pragma unroll
        for (int j = L - 1; j >= 1; --j)
            a[j] = __builtin_fmax(a[j - 1], __builtin_fmin(a[j], s));
        a[0] = __builtin_fmin(a[0], s);
    }
    // mean of float32(sqrt(.)) over the k entries, in numpy's order for a float32 row reduction (pairwise sum: a fold for
    // k < 8; else eight strided accumulators over the first k - k % 8 terms, combined as a tree, then the rest in order;
    // k <= 128, so its recursion never splits).  Destroys the list.
    __device__ __forceinline__ float mean(int k)
    {
        const int shift = L - k;
#pragma unroll
        for (int b = 1; b < L; b <<= 1) {
            if (shift & b) {
#pragma unroll
                for (int j = 0; j + b < L; ++j) a[j] = a[j + b];
            }
        }
        float d[L];
#pragma unroll
        for (int j = 0; j < L; ++j) {
            d[j] = 0.0f;
            if (j < k) d[j] = (float)__builtin_sqrt(a[j]);   // correctly rounded binary64, then round to nearest even
        }
        float res;
        if (k < 8) {
            res = 0.0f;
#pragma unroll
            for (int j = 0; j < (L < 8 ? L : 8); ++j)
                if (j < k) res += d[j];
        } else {
            const int n8 = k & ~7;
            float r[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = d[j];
#pragma unroll
            for (int j = 8; j < L; ++j)
                if (j < n8) r[j & 7] += d[j];
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
            for (int j = 8; j < L; ++j)
                if (j >= n8 && j < k) res += d[j];
        }
        return res / (float)k;
    }
};

template <int L>
__global__ __launch_bounds__(kBlock) void nearest_type_means_kernel(const double2 *__restrict__ xy,
                                                                    const int32_t *__restrict__ type,
                                                                    const int64_t *__restrict__ seg, int64_t n_fovs,
                                                                    int64_t n, int n_types, int k, double s_zero,
                                                                    float *__restrict__ means)
{
    __shared__ double2 cand[kBlock];
    __shared__ int32_t ctype[kBlock];
    __shared__ unsigned long long run_start[kBlock / kWave];

    const int tid = threadIdx.x;
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
    MeanRowWriter out{has_row ? means + i * n_types : nullptr, n_types, 0, has_row};
    NearestList<L> near;
    near.reset(k);

    // the first FOV that ends beyond r0
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
        int cur = -1, c = 0;   // the open run's type and its number of candidates at float32 distance > 0
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
                        if (mine && cur >= 0) out.put(cur, c >= k ? near.mean(k) : __builtin_nanf(""));
                        cur = __builtin_amdgcn_readfirstlane(ctype[w0 + p]);
                        c = 0;
                        near.reset(k);
                    }
                    const unsigned long long rest = p + 1 < kWave ? mask >> (p + 1) : 0ull;
                    int q = rest ? p + 1 + __builtin_ctzll(rest) : kWave;
                    q = q < cnt ? q : cnt;
#pragma unroll 4
                    for (int e = p; e < q; ++e) {
                        const double s = squared_distance(xi, yi, cand[w0 + e]);
                        const bool positive = s > s_zero;
                        c += positive ? 1 : 0;
                        if (positive && s < near.kth()) near.insert(s);
                    }
                    p = q;
                }
            }
        }
        if (mine && cur >= 0) out.put(cur, c >= k ? near.mean(k) : __builtin_nanf(""));
    }
    out.finish();
}

template <int L>
void launch(unsigned blocks, hipStream_t st, const double2 *xy, const int32_t *type, const int64_t *seg, int64_t n_fovs,
            int64_t n, int n_types, int k, double s_zero, float *means)
{
    hipLaunchKernelGGL(nearest_type_means_kernel<L>, dim3(blocks), dim3(kBlock), 0, st, xy, type, seg, n_fovs, n, n_types,
                       k, s_zero, means);
}

}  // namespace

PXSOM_EXPORT int pxsom_nearest_type_means(const double *xy_dev, const int32_t *type_dev, const int64_t *seg_dev,
                                          int64_t n_fovs, int64_t n, int n_types, int k, double s_zero,
                                          float *means_dev, void *stream)
{
    const char *fn = "pxsom_nearest_type_means";
    if (n < 0 || n_fovs < 0) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld, n_fovs=%lld", fn, (long long)n, (long long)n_fovs);
    if (n_types < 1) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n_types=%d < 1", fn, n_types);
    if (k < 1 || k > kMaxK)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: k=%d is outside 1 .. %d, the device route's limit", fn, k, kMaxK);
    if (s_zero != s_zero) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: s_zero is NaN", fn);
    if (!seg_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null seg", fn);
    if (n == 0) return PXSOM_OK;
    if (!xy_dev || !type_dev || !means_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null array", fn);
    if (reinterpret_cast<uintptr_t>(xy_dev) % sizeof(double2) != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: xy is not 16-byte aligned", fn);
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: n=%lld too large", fn, (long long)n);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double2 *xy = reinterpret_cast<const double2 *>(xy_dev);
    if (k <= 8)
        launch<8>((unsigned)blocks, st, xy, type_dev, seg_dev, n_fovs, n, n_types, k, s_zero, means_dev);
    else if (k <= 16)
        launch<16>((unsigned)blocks, st, xy, type_dev, seg_dev, n_fovs, n, n_types, k, s_zero, means_dev);
    else
        launch<32>((unsigned)blocks, st, xy, type_dev, seg_dev, n_fovs, n, n_types, k, s_zero, means_dev);
    PXSOM_LAUNCH_CHECK("nearest_type_means_kernel");
    return PXSOM_OK;
}
