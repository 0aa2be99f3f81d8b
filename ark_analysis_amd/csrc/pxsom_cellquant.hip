// pxsom_cellquant.hip -- the per-cell table of generate_cell_table on gfx950 (K12): a per-label reduction of an
// interleaved [H, W, C] image keyed by a finished segmentation.
//
//   count, exact row / column sums (centroid = sum / count), bounding box, and per channel one of
//     total_intensity   np.sum(img[rows, cols], axis=0) in the image's dtype       (ark/segmentation/signal_extraction.py)
//     positive_pixel    np.sum(img[rows, cols] > threshold, axis=0)
//     center_weighting  w.dot(img[rows, cols]), w = 1 - d / (max d + 1), d = Chebyshev distance to the centroid
//   and optionally the nuclear label with the most pixels inside the cell (segmentation_utils.find_nuclear_label_id).
//
// Three launches:
//   map_kernel    one wave per 64-column row segment: label -> dense cell index (the K10 key table: a dense LUT or a
//                 binary search), stored as an int32 index image; each run of equal labels in the segment adds its
//                 length, row sum and column sum with one set of atomics (integers: exact in any order) and widens the
//                 bounding box.  The nuclear image is mapped by the same kernel without statistics.
//   walk_kernel   one wave per cell.  The wave walks the cell's bounding box in raster order, 64 columns of a row at a
//                 time; a ballot of `index == cell` gives the member pixels, which are visited lowest bit first, so the
//                 pixels come in numpy's order (the coords of regionprops are raster order).  Lane = channel: every lane
//                 folds its channel over the pixels one after another, which is numpy's order for a float [n, C >= 2]
//                 sum over axis 0.  Integers are summed in int64 (exact, any order).
//   C == 1        numpy sums an [n, 1] float column with its pairwise scheme (blocks of 8192 from its reduction
//                 buffer, each pairwise with 8 accumulators below 128 elements).  The walk then copies the member values
//                 into a per-cell list in raster order and lane 0 evaluates that exact tree (pairwise_chunked).
//
// The nuclear overlap is counted during the walk in a register table of up to 128 (label, count) entries per wave
// (lane i holds entries i and i + 64).  A cell meeting more distinct nuclei than the table holds takes the overflow
// route: one more walk per distinct nucleus, in ascending label order, each finding the next smallest label and its count.
#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>

#include "pxsom_common.h"
#include "pxsom_keytable.h"

namespace {

constexpr int kWaves = 4;                      // waves per block, both kernels
constexpr int kNucMaxCapacity = 128;
constexpr int kBatch = 8;                      // member pixels whose loads are in flight together
constexpr int kAcc = 2;                        // channel accumulators per lane: 128 channels per walk
constexpr int64_t kNumpyBuffer = 8192;         // numpy's default ufunc buffer size (np.getbufsize())
constexpr int kPairwiseBlock = 128;            // numpy's PW_BLOCKSIZE

// dense cell index of a label: 0 is the background, -1
template <typename TI>
__device__ __forceinline__ int32_t dense_index(const KeyTable &t, TI label)
{
    if (label == (TI)0) return -1;
    return (int32_t)find_key(t, (int32_t)(int64_t)label);
}

__global__ __launch_bounds__(256) void init_kernel(int64_t n, unsigned long long *__restrict__ count,
                                                   unsigned long long *__restrict__ sums, int32_t *__restrict__ bbox)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        count[i] = 0;
        sums[2 * i] = 0;
        sums[2 * i + 1] = 0;
        bbox[4 * i + 0] = INT_MAX;   // row min, row max, column min, column max
        bbox[4 * i + 1] = -1;
        bbox[4 * i + 2] = INT_MAX;
        bbox[4 * i + 3] = -1;
    }
}

template <typename TI, bool kStats>
__global__ __launch_bounds__(256) void map_kernel(const TI *__restrict__ seg, int h, int w, int64_t ld, KeyTable t,
                                                  int32_t *__restrict__ idx, int segs_per_row,
                                                  unsigned long long *__restrict__ count,
                                                  unsigned long long *__restrict__ sums, int32_t *__restrict__ bbox)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (s >= (int64_t)h * segs_per_row) return;        // whole wave
    const int r = (int)(s / segs_per_row), cs = (int)(s % segs_per_row) * 64;
    const int col = cs + lane;
    const bool valid = col < w;
    const int32_t k = valid ? dense_index<TI>(t, seg[(int64_t)r * ld + col]) : -1;
    if (valid) idx[(int64_t)r * w + col] = k;
    if constexpr (kStats) {
        const int32_t left = __shfl_up(k, 1, 64), right = __shfl_down(k, 1, 64);
        const bool head = k >= 0 && (lane == 0 || left != k);
        const bool tail = k >= 0 && (lane == 63 || col + 1 >= w || right != k);
        const unsigned long long heads = __ballot(head);
        if (tail) {
            const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
            const int start = 63 - __builtin_clzll(heads & upto);
            const long long len = lane - start + 1, c0 = cs + start, c1 = col;
            atomicAdd(&count[k], (unsigned long long)len);
            atomicAdd(&sums[2 * (int64_t)k], (unsigned long long)((long long)r * len));
            atomicAdd(&sums[2 * (int64_t)k + 1], (unsigned long long)((c0 + c1) * len / 2));
            atomicMin(&bbox[4 * (int64_t)k + 0], r);
            atomicMax(&bbox[4 * (int64_t)k + 1], r);
            atomicMin(&bbox[4 * (int64_t)k + 2], (int)c0);
            atomicMax(&bbox[4 * (int64_t)k + 3], (int)c1);
        }
    }
}

// exclusive prefix of the counts (one block): where each cell's list starts in the C == 1 scratch
__global__ __launch_bounds__(1024) void offsets_kernel(const unsigned long long *__restrict__ count, int64_t n,
                                                       int64_t *__restrict__ off)
{
    __shared__ int64_t part[1024];
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < n ? (int64_t)count[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int64_t add = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n) off[i] = carry + part[threadIdx.x] - v;
        carry += part[1023];
        __syncthreads();
    }
}

template <typename T>
struct Acc {
    typedef typename std::conditional<std::is_floating_point<T>::value, T, int64_t>::type type;
};

// numpy's <TYPE>_pairwise_sum (loops_utils.h.src) over a contiguous list, recursion unrolled onto a stack
template <typename T>
__device__ T pairwise_leaf(const T *a, int64_t n)
{
    if (n < 8) {
        T res = (T)0;
        for (int64_t i = 0; i < n; i++) res += a[i];
        return res;
    }
    T r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = a[j];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] += a[i + j];
    }
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
}

template <typename T>
__device__ T pairwise(const T *a, int64_t n)
{
    struct Frame {
        int64_t off, n;
        int state;      // 0: descend left, 1: left done -> descend right, 2: both done
        T left;
    };
    Frame st[12];                  // depth <= 8 for a chunk of 8192 (blocks of 128 below it)
    int sp = 0;
    st[0].off = 0;
    st[0].n = n;
    st[0].state = 0;
    T ret = (T)0;
    for (;;) {
        Frame &f = st[sp];
        if (f.n <= kPairwiseBlock) {
            ret = pairwise_leaf(a + f.off, f.n);
        } else {
            int64_t n2 = f.n / 2;
            n2 -= n2 % 8;
            if (f.state == 0) {
                f.state = 1;
                st[sp + 1].off = f.off;
                st[sp + 1].n = n2;
                st[sp + 1].state = 0;
                ++sp;
                continue;
            }
            if (f.state == 1) {
                f.left = ret;
                f.state = 2;
                st[sp + 1].off = f.off + n2;
                st[sp + 1].n = f.n - n2;
                st[sp + 1].state = 0;
                ++sp;
                continue;
            }
            ret = f.left + ret;
        }
        if (sp == 0) break;
        --sp;
    }
    return ret;
}

// np.add.reduce of a contiguous column: out = 0, then out += pairwise(chunk) per buffer-sized chunk
template <typename T>
__device__ T pairwise_chunked(const T *a, int64_t n)
{
    T out = (T)0;
    for (int64_t s = 0; s < n; s += kNumpyBuffer) out += pairwise(a + s, min(kNumpyBuffer, n - s));
    return out;
}

// (count, label) order of find_nuclear_label_id: more pixels first, then the smaller label
__device__ __forceinline__ bool nuc_better(int c, int k, int bc, int bk)
{
    return c > bc || (c == bc && c > 0 && k < bk);
}

struct WalkArgs {
    const int32_t *idx;          // [h, w] dense cell index, -1 outside every cell
    const int32_t *nuc;          // [h, w] dense nucleus index or nullptr
    int h, w, c;
    int64_t n;
    const unsigned long long *count;
    const unsigned long long *sums;
    const int32_t *bbox;
    double threshold;
    int nuc_capacity;
    double *values;              // [n, c]
    int32_t *nuc_out;            // [n]
    const int64_t *off;          // C == 1 pairwise route: list offsets
    void *list;                  // C == 1 pairwise route: T [sum of counts]
};

template <typename T, int kMode, bool kPairwise>
__global__ __launch_bounds__(256) void walk_kernel(const T *__restrict__ img, WalkArgs a)
{
    typedef typename std::conditional<kMode == PXSOM_CELLQUANT_TOTAL, typename Acc<T>::type,
                                      typename std::conditional<kMode == PXSOM_CELLQUANT_POSITIVE, int64_t,
                                                                double>::type>::type A;
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (k >= a.n) return;                               // whole wave
    const int64_t n_px = (int64_t)a.count[k];
    const int r0 = a.bbox[4 * k], r1 = a.bbox[4 * k + 1], c0 = a.bbox[4 * k + 2], c1 = a.bbox[4 * k + 3];
    const int segs = n_px > 0 ? (c1 - c0) / 64 + 1 : 0;
    const int64_t n_segs = n_px > 0 ? (int64_t)(r1 - r0 + 1) * segs : 0;
    const int w = a.w, C = a.c;
    const unsigned long long below = (1ull << lane) - 1;

    // centroid and the largest Chebyshev distance (center_weighting): a first walk
    double cr = 0.0, cc = 0.0, denom = 1.0;
    if constexpr (kMode == PXSOM_CELLQUANT_CENTER) {
        if (n_px > 0) {
            cr = (double)(int64_t)a.sums[2 * k] / (double)n_px;
            cc = (double)(int64_t)a.sums[2 * k + 1] / (double)n_px;
        }
        double dmax = 0.0;
        for (int64_t s = 0; s < n_segs; s++) {
            const int r = r0 + (int)(s / segs), col = c0 + (int)(s % segs) * 64 + lane;
            if (col <= c1 && a.idx[(int64_t)r * w + col] == (int32_t)k)
                dmax = fmax(dmax, fmax(fabs((double)r - cr), fabs((double)col - cc)));
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, d, 64));
        denom = dmax + 1.0;
    }

    // nuclear overlap table: lane i holds entries i and i + 64
    int tk0 = -1, tc0 = 0, tk1 = -1, tc1 = 0, t_size = 0;
    bool overflow = false;
    const bool with_nuc = a.nuc != nullptr;

    T *list = kPairwise ? static_cast<T *>(a.list) + a.off[k] : nullptr;
    int64_t listed = 0;

    for (int cb = 0; cb < (kPairwise ? 1 : C); cb += 64 * kAcc) {
        A acc[kAcc];
#pragma unroll
        for (int j = 0; j < kAcc; j++) acc[j] = (A)0;
        int32_t next = -1;
        if (n_segs > 0) {
            const int col = c0 + lane;
            next = col <= c1 ? a.idx[(int64_t)r0 * w + col] : -1;
        }
        for (int64_t s = 0; s < n_segs; s++) {
            const int r = r0 + (int)(s / segs), cs = c0 + (int)(s % segs) * 64;
            const int32_t cur = next;
            if (s + 1 < n_segs) {                          // the next segment's indices, in flight during this one
                const int rn = r0 + (int)((s + 1) / segs), coln = c0 + (int)((s + 1) % segs) * 64 + lane;
                next = coln <= c1 ? a.idx[(int64_t)rn * w + coln] : -1;
            }
            const bool member = cur == (int32_t)k;
            unsigned long long mask = __ballot(member);
            if (mask == 0) continue;
            const int64_t pix_row = (int64_t)r * w + cs;

            if (with_nuc && cb == 0) {
                int32_t nid = member ? a.nuc[pix_row + lane] : -1;
                unsigned long long pend = __ballot(nid >= 0);
                while (pend) {
                    const int leader = __builtin_ctzll(pend);
                    const int key = __shfl(nid, leader, 64);
                    const unsigned long long same = __ballot(nid == key);
                    const int cnt = __popcll(same);
                    if (nid == key) nid = -1;
                    pend &= ~same;
                    const unsigned long long hit0 = __ballot(tk0 == key), hit1 = __ballot(tk1 == key);
                    if (hit0 || hit1) {
                        if (tk0 == key) tc0 += cnt;
                        if (tk1 == key) tc1 += cnt;
                    } else if (t_size < a.nuc_capacity) {
                        if (lane == (t_size & 63)) {
                            if (t_size < 64) { tk0 = key; tc0 = cnt; }
                            else { tk1 = key; tc1 = cnt; }
                        }
                        t_size++;
                    } else {
                        overflow = true;
                    }
                }
            }

            if constexpr (kPairwise) {
                if (member) list[listed + __popcll(mask & below)] = img[pix_row + lane];
                listed += __popcll(mask);
                continue;
            }

            while (mask) {
                int p[kBatch];
                int q = 0;
#pragma unroll
                for (int j = 0; j < kBatch; j++) {
                    p[j] = mask ? __builtin_ctzll(mask) : 0;
                    if (mask) { mask &= mask - 1; q++; }
                }
                T v[kBatch][kAcc];
#pragma unroll
                for (int j = 0; j < kBatch; j++) {
#pragma unroll
                    for (int i = 0; i < kAcc; i++) {
                        const int ch = cb + i * 64 + lane;
                        v[j][i] = (j < q && ch < C) ? img[(pix_row + p[j]) * C + ch] : (T)0;
                    }
                }
#pragma unroll
                for (int j = 0; j < kBatch; j++) {
                    if (j >= q) break;
                    if constexpr (kMode == PXSOM_CELLQUANT_TOTAL) {
#pragma unroll
                        for (int i = 0; i < kAcc; i++) acc[i] += (A)v[j][i];
                    } else if constexpr (kMode == PXSOM_CELLQUANT_POSITIVE) {
#pragma unroll
                        for (int i = 0; i < kAcc; i++) acc[i] += (double)v[j][i] > a.threshold ? 1 : 0;
                    } else {
                        const int col = cs + p[j];
                        const double d = fmax(fabs((double)r - cr), fabs((double)col - cc));
                        const double wgt = 1.0 - d / denom;
#pragma unroll
                        for (int i = 0; i < kAcc; i++) acc[i] += wgt * (double)v[j][i];
                    }
                }
            }
        }
        if constexpr (!kPairwise) {
#pragma unroll
            for (int i = 0; i < kAcc; i++) {
                const int ch = cb + i * 64 + lane;
                if (ch < C) a.values[k * C + ch] = (double)acc[i];
            }
        }
    }

    if constexpr (kPairwise) {
        if (lane == 0) a.values[k] = (double)pairwise_chunked(list, listed);
    }

    if (!with_nuc) return;
    int best_k = -1, best_c = 0;
    if (!overflow) {
        if (nuc_better(tc0, tk0, best_c, best_k)) { best_c = tc0; best_k = tk0; }
        if (nuc_better(tc1, tk1, best_c, best_k)) { best_c = tc1; best_k = tk1; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int oc = __shfl_xor(best_c, d, 64), ok = __shfl_xor(best_k, d, 64);
            if (nuc_better(oc, ok, best_c, best_k)) { best_c = oc; best_k = ok; }
        }
    } else {
        // overflow route: the distinct nuclei in ascending order, one walk each (next smallest index and its count)
        int prev = -1;
        for (;;) {
            int cur_min = INT_MAX, cur_cnt = 0;
            for (int64_t s = 0; s < n_segs; s++) {
                const int r = r0 + (int)(s / segs), col = c0 + (int)(s % segs) * 64 + lane;
                const int64_t px = (int64_t)r * w + col;
                const bool member = col <= c1 && a.idx[px] == (int32_t)k;
                const int nid = member ? a.nuc[px] : -1;
                int m = nid > prev ? nid : INT_MAX;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) m = min(m, __shfl_xor(m, d, 64));
                if (m == INT_MAX || m > cur_min) continue;
                const int cnt = __popcll(__ballot(nid == m));
                if (m < cur_min) { cur_min = m; cur_cnt = cnt; }
                else cur_cnt += cnt;
            }
            if (cur_min == INT_MAX) break;
            if (cur_cnt > best_c) { best_c = cur_cnt; best_k = cur_min; }   // ascending: a tie keeps the smaller
            prev = cur_min;
        }
    }
    if (lane == 0) a.nuc_out[k] = best_k;
}

bool is_float(int dt) { return dt == PXSOM_SEG_F32 || dt == PXSOM_SEG_F64; }

size_t lut_bytes(int64_t n_keys, int32_t key_min, int32_t key_max, int flags)
{
    return (flags & PXSOM_CELLQUANT_FORCE_SEARCH) ? 0 : pxsom::dense_lut_bytes(n_keys, key_min, key_max);
}

struct Layout {
    size_t idx, nuc_idx, lut, nuc_lut, off, list, total;
    size_t lut_b, nuc_lut_b;
};

Layout layout(int h, int w, int c, int img_dtype, int mode, int64_t n_keys, int32_t key_min, int32_t key_max,
              int64_t n_nuc_keys, int32_t nuc_key_min, int32_t nuc_key_max, int flags)
{
    Layout L;
    const size_t px = (size_t)h * (size_t)w;
    size_t at = 0;
    L.idx = at;
    at += pxsom::align_up(px * sizeof(int32_t), 256);
    L.nuc_idx = at;
    if (n_nuc_keys >= 0) at += pxsom::align_up(px * sizeof(int32_t), 256);
    L.lut_b = lut_bytes(n_keys, key_min, key_max, flags);
    L.lut = at;
    at += pxsom::align_up(L.lut_b, 256);
    L.nuc_lut_b = n_nuc_keys > 0 ? lut_bytes(n_nuc_keys, nuc_key_min, nuc_key_max, flags) : 0;
    L.nuc_lut = at;
    at += pxsom::align_up(L.nuc_lut_b, 256);
    L.off = L.list = at;
    if (mode == PXSOM_CELLQUANT_TOTAL && c == 1 && is_float(img_dtype)) {
        at += pxsom::align_up((size_t)(n_keys + 1) * sizeof(int64_t), 256);
        L.list = at;
        at += pxsom::align_up(px * (size_t)pxsom::plane_dtype_bytes(img_dtype), 256);
    }
    L.total = at;
    return L;
}

template <bool kStats>
int launch_map(const void *seg, int seg_dtype, int h, int w, int64_t ld, const KeyTable &t, int32_t *idx,
               unsigned long long *count, unsigned long long *sums, int32_t *bbox, hipStream_t st)
{
    const int segs = (w + 63) / 64;
    const int64_t blocks = ((int64_t)h * segs + kWaves - 1) / kWaves;
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_cellquant: image too large");
    pxsom::dispatch_label(seg_dtype, [&](auto ti) {
        typedef decltype(ti) TI;
        hipLaunchKernelGGL((map_kernel<TI, kStats>), dim3((unsigned)blocks), dim3(256), 0, st,
                           reinterpret_cast<const TI *>(seg), h, w, ld, t, idx, segs, count, sums, bbox);
    });
    PXSOM_LAUNCH_CHECK("map_kernel");
    return PXSOM_OK;
}

template <typename T>
int launch_walk_typed(const void *img, const WalkArgs &a, int mode, hipStream_t st)
{
    const int64_t blocks = (a.n + kWaves - 1) / kWaves;
    if (blocks > 0x7fffffff) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_cellquant: too many cells");
    const T *p = reinterpret_cast<const T *>(img);
    const dim3 grid((unsigned)blocks), block(256);
    if (mode == PXSOM_CELLQUANT_TOTAL) {
        if constexpr (std::is_floating_point<T>::value) {
            if (a.c == 1) {
                PXSOM_TIMED_LAUNCH((walk_kernel<T, PXSOM_CELLQUANT_TOTAL, true>), grid, block, 0, st, p, a);
                PXSOM_LAUNCH_CHECK("walk_kernel");
                return PXSOM_OK;
            }
        }
        PXSOM_TIMED_LAUNCH((walk_kernel<T, PXSOM_CELLQUANT_TOTAL, false>), grid, block, 0, st, p, a);
    } else if (mode == PXSOM_CELLQUANT_POSITIVE) {
        PXSOM_TIMED_LAUNCH((walk_kernel<T, PXSOM_CELLQUANT_POSITIVE, false>), grid, block, 0, st, p, a);
    } else {
        PXSOM_TIMED_LAUNCH((walk_kernel<T, PXSOM_CELLQUANT_CENTER, false>), grid, block, 0, st, p, a);
    }
    PXSOM_LAUNCH_CHECK("walk_kernel");
    return PXSOM_OK;
}

}  // namespace

PXSOM_EXPORT size_t pxsom_cellquant_workspace_bytes(int h, int w, int c, int img_dtype, int mode, int64_t n_keys,
                                                    int32_t key_min, int32_t key_max, int64_t n_nuc_keys,
                                                    int32_t nuc_key_min, int32_t nuc_key_max, int flags)
{
    if (h < 1 || w < 1 || c < 1 || n_keys < 0) return 0;
    return layout(h, w, c, img_dtype, mode, n_keys, key_min, key_max, n_nuc_keys, nuc_key_min, nuc_key_max, flags).total;
}

PXSOM_EXPORT int pxsom_cellquant(const void *seg_dev, int seg_dtype, int64_t ld, const void *nuc_dev, int nuc_dtype,
                                 int64_t ldn, int h, int w, const void *img_dev, int img_dtype, int c,
                                 const int32_t *keys_dev, int64_t n_keys, int32_t key_min, int32_t key_max,
                                 const int32_t *nuc_keys_dev, int64_t n_nuc_keys, int32_t nuc_key_min,
                                 int32_t nuc_key_max, int mode, double threshold, int nuc_capacity, int64_t *count_dev,
                                 int64_t *sums_dev, int32_t *bbox_dev, double *values_dev, int32_t *nuc_out_dev,
                                 void *workspace_dev, size_t workspace_bytes, int flags, void *stream)
{
    const char *fn = "pxsom_cellquant";
    if (!pxsom::is_label_dtype(seg_dtype)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad seg_dtype %d", fn, seg_dtype);
    if (!pxsom::is_image_dtype(img_dtype, true)) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad img_dtype %d", fn, img_dtype);
    if (mode < PXSOM_CELLQUANT_TOTAL || mode > PXSOM_CELLQUANT_CENTER)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad mode %d", fn, mode);
    if (h < 1 || w < 1 || c < 1 || ld < w)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad sizes (%d x %d x %d, ld %lld)", fn, h, w, c, (long long)ld);
    if (flags & ~PXSOM_CELLQUANT_FORCE_SEARCH) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: unknown flags %d", fn, flags);
    if (!seg_dev || !img_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null image", fn);
    if (n_keys < 0 || (n_keys > 0 && (!keys_dev || key_min > key_max || !count_dev || !sums_dev || !bbox_dev ||
                                       !values_dev)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad cell table or outputs", fn);
    const bool with_nuc = nuc_dev != nullptr;
    if (with_nuc) {
        if (!pxsom::is_label_dtype(nuc_dtype) || ldn < w || n_nuc_keys < 0 || (n_keys > 0 && !nuc_out_dev) ||
            (n_nuc_keys > 0 && (!nuc_keys_dev || nuc_key_min > nuc_key_max)))
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: bad nuclear image, table or output", fn);
        if (nuc_capacity == 0) nuc_capacity = kNucMaxCapacity;
        if (nuc_capacity < 1 || nuc_capacity > kNucMaxCapacity)
            return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: nuc_capacity %d outside 1 .. %d", fn, nuc_capacity,
                               kNucMaxCapacity);
    }
    const Layout L = layout(h, w, c, img_dtype, mode, n_keys, key_min, key_max, with_nuc ? n_nuc_keys : -1,
                            nuc_key_min, nuc_key_max, flags);
    if (!workspace_dev || workspace_bytes < L.total)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, L.total);
    if (n_keys == 0) return PXSOM_OK;

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_dev);
    unsigned long long *count = reinterpret_cast<unsigned long long *>(count_dev);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(sums_dev);
    hipLaunchKernelGGL(init_kernel, dim3(pxsom::flat_grid(n_keys, 4)), dim3(256), 0, st, n_keys, count, sums, bbox_dev);
    PXSOM_LAUNCH_CHECK("init_kernel");
    KeyTable t{keys_dev, nullptr, n_keys, key_min, 0};
    if (L.lut_b) {
        const int rc = build_lut(t, reinterpret_cast<int32_t *>(ws + L.lut), L.lut_b, st);
        if (rc != PXSOM_OK) return rc;
    }
    int32_t *idx = reinterpret_cast<int32_t *>(ws + L.idx);
    int rc = launch_map<true>(seg_dev, seg_dtype, h, w, ld, t, idx, count, sums, bbox_dev, st);
    if (rc != PXSOM_OK) return rc;

    int32_t *nuc_idx = nullptr;
    if (with_nuc) {
        nuc_idx = reinterpret_cast<int32_t *>(ws + L.nuc_idx);
        KeyTable tn{nuc_keys_dev, nullptr, n_nuc_keys, nuc_key_min, 0};
        if (n_nuc_keys == 0) {
            PXSOM_HIP_TRY(hipMemsetAsync(nuc_idx, 0xFF, (size_t)h * w * sizeof(int32_t), st));
        } else {
            if (L.nuc_lut_b) {
                rc = build_lut(tn, reinterpret_cast<int32_t *>(ws + L.nuc_lut), L.nuc_lut_b, st);
                if (rc != PXSOM_OK) return rc;
            }
            rc = launch_map<false>(nuc_dev, nuc_dtype, h, w, ldn, tn, nuc_idx, nullptr, nullptr, nullptr, st);
            if (rc != PXSOM_OK) return rc;
        }
    }

    WalkArgs a;
    a.idx = idx;
    a.nuc = nuc_idx;
    a.h = h;
    a.w = w;
    a.c = c;
    a.n = n_keys;
    a.count = count;
    a.sums = sums;
    a.bbox = bbox_dev;
    a.threshold = threshold;
    a.nuc_capacity = nuc_capacity;
    a.values = values_dev;
    a.nuc_out = nuc_out_dev;
    a.off = nullptr;
    a.list = nullptr;
    if (mode == PXSOM_CELLQUANT_TOTAL && c == 1 && is_float(img_dtype)) {
        int64_t *off = reinterpret_cast<int64_t *>(ws + L.off);
        hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(1024), 0, st, count, n_keys, off);
        PXSOM_LAUNCH_CHECK("offsets_kernel");
        a.off = off;
        a.list = ws + L.list;
    }
    return pxsom::dispatch_image<true>(img_dtype, [&](auto ti) { return launch_walk_typed<decltype(ti)>(img_dev, a, mode, st); });
}
