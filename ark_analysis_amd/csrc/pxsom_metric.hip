// pxsom_metric.hip -- BMU assignment for FlowSOM's other distances (distf 1 Manhattan, 3 Chebyshev, 4 cosine):
// pxsom_assign_metric (include/pxsom.h; DESIGN.md "K7m").
//
// Every (row, node) pair is evaluated in binary64 in the oracle's order (pxsom_metric.h); there is no screen, so the
// result is the table of pxsom.h bit for bit by construction, ties and NaN included.  One lane per row; the codebook,
// transposed to [c][kp] (kp = k rounded up to kNodeTile, padded with zero nodes) by a prep launch, is read with scalar
// loads -- at a fixed channel the kNodeTile nodes of a tile are kNodeTile consecutive, wave-uniform doubles -- so the
// inner loop is two binary64 VALU instructions per (row, node, channel) term (three for Chebyshev, whose accumulator the
// compiler re-canonicalises before each maxNum).  Rows of up to kRegChannels channels are converted once into registers.
// Wider rows are staged per wave, kStageCh channels of its 64 rows at a time: coalesced loads (kStageCh consecutive lanes
// read one row's segment), converted once to binary64 and written channel-major to the wave's own LDS slice, from which
// each lane reads its row conflict-free for the 16 nodes of the tile.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "pxsom_common.h"
#include "pxsom_metric.h"

namespace {

using pxsom_metric::finish;
using pxsom_metric::square_add;
using pxsom_metric::term;

constexpr int kNodeTile = 16;     // accumulators per lane (32 VGPRs)
constexpr int kRegChannels = 32;  // rows held in registers (64 VGPRs) up to this width
constexpr size_t kHdrBytes = 256; // [0]: unsigned, rows evaluated in binary64 (pxsom_assign_last_exact_rows)
constexpr int kStageCh = 16;      // wider rows: channels per staged chunk
constexpr int kStageLd = 65;      // doubles between two channels of a chunk (odd: the staging writes spread over the banks)
constexpr size_t kStageBytes = (size_t)4 * kStageCh * kStageLd * sizeof(double);   // 4 waves per workgroup (33 KB)

int padded_nodes(int k) { return (k + kNodeTile - 1) / kNodeTile * kNodeTile; }

size_t metric_workspace_bytes(int c, int k)
{
    const size_t kp = (size_t)padded_nodes(k);
    return kHdrBytes + (size_t)c * kp * sizeof(double) + kp * sizeof(double);
}

// wt[j][kk] = w[kk][j] (zero for the padding nodes); wn[kk] = sqrt(sum_j w_kj * w_kj), j ascending (cosine only)
__global__ __launch_bounds__(256) void metric_prep_kernel(const double *__restrict__ w, int k, int c, int kp,
                                                          double *__restrict__ wt, double *__restrict__ wn,
                                                          unsigned *hdr, unsigned rows, int norms)
{
    const int64_t total = (int64_t)c * kp;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e / kp), kk = (int)(e - (int64_t)j * kp);
        wt[e] = kk < k ? w[(size_t)kk * c + j] : 0.0;
    }
    if (norms) {
        for (int kk = blockIdx.x * 256 + threadIdx.x; kk < kp; kk += gridDim.x * 256) {
            double d2 = 0.0;
            if (kk < k)
                for (int j = 0; j < c; j++) d2 = square_add(d2, w[(size_t)kk * c + j]);
            wn[kk] = sqrt(d2);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr[0] = rows;
}

// CX > 0: rows of c <= CX channels, converted once into registers; CX == 0: any width, staged in LDS per chunk
template <int M, typename T, int CX>
__global__ __launch_bounds__(256) void bmu_metric_kernel(const T *__restrict__ x, int64_t n, int c, int64_t ldx,
                                                         const double *__restrict__ wt, const double *__restrict__ wn,
                                                         int k, int kp, int32_t *__restrict__ labels,
                                                         double *__restrict__ dist)
{
#pragma clang fp contract(off)
    constexpr bool COS = M == PXSOM_METRIC_COSINE;
    extern __shared__ double stage_raw[];
    const int lane = threadIdx.x & 63;
    double *xs = stage_raw + (threadIdx.x >> 6) * (kStageCh * kStageLd);   // this wave's [kStageCh][kStageLd] chunk
    const int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63);
    // wave-uniform loop: the last wave's idle lanes work on row n - 1 and store nothing
    for (int64_t base = wave0; base < n; base += (int64_t)gridDim.x * 256) {
        const int64_t row = base + lane;
        const T *xp = x + (row < n ? row : n - 1) * ldx;
        double xr[CX > 0 ? CX : 1];
        if constexpr (CX > 0) {
#pragma unroll
            for (int j = 0; j < CX; j++) xr[j] = (double)xp[j < c ? j : c - 1];  // (slots j >= c are never used)
        }
        double sx = 0.0;  // cosine: sqrt(sum_j x_j * x_j), j ascending (staged rows: during the first node tile)
        double d1 = 0.0;
        if constexpr (COS && CX > 0) {
#pragma unroll
            for (int j = 0; j < CX; j++)
                if (j < c) d1 = square_add(d1, xr[j]);
            sx = sqrt(d1);
        }
        (void)xp;
        (void)xs;
        double best = DBL_MAX;
        int bk = -1;
        for (int k0 = 0; k0 < kp; k0 += kNodeTile) {
            double acc[kNodeTile];
#pragma unroll
            for (int t = 0; t < kNodeTile; t++) acc[t] = 0.0;
            if constexpr (CX > 0) {
#pragma unroll
                for (int j = 0; j < CX; j++) {
                    if (j < c) {  // uniform: a fully unrolled loop keeps the row in registers
                        const double *wj = wt + (size_t)j * kp + k0;
#pragma unroll
                        for (int t = 0; t < kNodeTile; t++) acc[t] = term<M>(acc[t], xr[j], wj[t]);
                    }
                }
            } else {
                for (int j0 = 0; j0 < c; j0 += kStageCh) {
                    const int cw = min(kStageCh, c - j0);
                    // LDS runs a wave's accesses in order: the previous chunk's reads precede these writes, the writes
                    // precede the reads below (the wave barriers only keep the compiler from moving code across)
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int u = 0; u < kStageCh; u++) {
                        const int e = lane + 64 * u, r = e / kStageCh, ch = e % kStageCh;
                        if (ch < cw) {
                            const int64_t sr = base + r < n ? base + r : n - 1;
                            xs[ch * kStageLd + r] = (double)x[sr * ldx + j0 + ch];
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
#pragma unroll 4
                    for (int jj = 0; jj < cw; jj++) {
                        const double xj = xs[jj * kStageLd + lane];
                        if (COS && k0 == 0) d1 = square_add(d1, xj);
                        const double *wj = wt + (size_t)(j0 + jj) * kp + k0;
#pragma unroll
                        for (int t = 0; t < kNodeTile; t++) acc[t] = term<M>(acc[t], xj, wj[t]);
                    }
                }
                if (COS && k0 == 0) sx = sqrt(d1);
            }
            // FlowSOM's selection, nodes ascending: first strict minimum below DBL_MAX (NaN never compares smaller)
#pragma unroll
            for (int t = 0; t < kNodeTile; t++) {
                if (k0 + t < k) {
                    const double d = finish<M>(acc[t], sx, COS ? wn[k0 + t] : 0.0);
                    if (d < best) {
                        best = d;
                        bk = k0 + t;
                    }
                }
            }
        }
        if (row < n) {
            labels[row] = bk + 1;
            if (dist) dist[row] = best;
        }
    }
}

template <int M, typename T>
int assign_metric_typed(const T *x, int64_t n, int c, int64_t ldx, const double *w, int k, int32_t *labels,
                        double *dist, char *ws, hipStream_t st)
{
    const int kp = padded_nodes(k);
    double *wt = reinterpret_cast<double *>(ws + kHdrBytes);
    double *wn = wt + (size_t)c * kp;
    const int pgrid = (int)std::min<int64_t>(((int64_t)c * kp + 255) / 256, 1024);
    hipLaunchKernelGGL(metric_prep_kernel, dim3(pgrid), dim3(256), 0, st, w, k, c, kp, wt, wn,
                       reinterpret_cast<unsigned *>(ws), (unsigned)n, M == PXSOM_METRIC_COSINE ? 1 : 0);
    PXSOM_LAUNCH_CHECK("metric_prep_kernel");
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)pxsom::device_cu_count() * 8));
    const bool reg = c <= kRegChannels;
    auto kern = reg ? bmu_metric_kernel<M, T, kRegChannels> : bmu_metric_kernel<M, T, 0>;
    const size_t lds = reg ? 0 : kStageBytes;
    pxsom::Prof *prof = pxsom::current_prof();
    pxsom::prof_mark(prof, st, true, n);
    PXSOM_TIMED_LAUNCH(kern, dim3((unsigned)grid), dim3(256), lds, st, x, n, c, ldx, wt, wn, k, kp, labels, dist);
    pxsom::prof_mark(prof, st, false, n);
    PXSOM_LAUNCH_CHECK("bmu_metric_kernel");
    return PXSOM_OK;
}

template <int M>
int assign_metric(const void *x, int64_t n, int c, int64_t ldx, int dtype, const double *w, int k, int32_t *labels,
                  double *dist, char *ws, hipStream_t st)
{
    PXSOM_DISPATCH_DTYPE(dtype, x, xp, (assign_metric_typed<M, T>(xp, n, c, ldx, w, k, labels, dist, ws, st)));
}

bool metric_known(int metric) { return metric >= PXSOM_METRIC_MANHATTAN && metric <= PXSOM_METRIC_COSINE; }

}  // namespace

PXSOM_EXPORT size_t pxsom_assign_metric_workspace_bytes(int64_t n, int c, int k, int metric)
{
    if (metric == PXSOM_METRIC_EUCLIDEAN) return pxsom_assign_workspace_bytes(n, c, k);
    if (!metric_known(metric) || n < 0 || c < 1 || c > PXSOM_MAX_CHANNELS || k < 1 || k > PXSOM_MAX_NODES) return 0;
    return metric_workspace_bytes(c, k);
}

PXSOM_EXPORT int pxsom_assign_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev,
                                     int k, int32_t *labels_dev, double *dist_dev, void *workspace_dev,
                                     size_t workspace_bytes, int metric, void *stream)
{
    if (!metric_known(metric))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG,
                           "pxsom_assign_metric: unknown metric %d (FlowSOM distf: 1 Manhattan, 2 Euclidean, 3 Chebyshev, "
                           "4 cosine)", metric);
    if (metric == PXSOM_METRIC_EUCLIDEAN)
        return pxsom_assign(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, dist_dev, workspace_dev, workspace_bytes, stream);
    if (n < 0 || n > 0x7fffffffLL)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_metric: n=%lld outside [0, 2^31)", (long long)n);
    if (c < 1 || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_metric: c=%d outside [1, %d]", c, PXSOM_MAX_CHANNELS);
    if (k < 1 || k > PXSOM_MAX_NODES)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_metric: k=%d outside [1, %d]", k, PXSOM_MAX_NODES);
    if (ldx < c) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_metric: ldx=%lld < c=%d", (long long)ldx, c);
    if (!pxsom::dtype_ok(dtype)) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_metric: dtype %d", dtype);
    if (!w_dev || (n > 0 && (!x_dev || !labels_dev)))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "pxsom_assign_metric: null pointer");
    const size_t need = metric_workspace_bytes(c, k);
    if (!workspace_dev || workspace_bytes < need)
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "pxsom_assign_metric: workspace %zu < %zu bytes", workspace_bytes, need);
    if (pxsom::row_view_active())
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_assign_metric: the metric kernels do not take row views");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = reinterpret_cast<char *>(workspace_dev);
    if (n == 0) {
        PXSOM_HIP_TRY(hipMemsetAsync(ws, 0, kHdrBytes, st));
        return PXSOM_OK;
    }
    switch (metric) {
    case PXSOM_METRIC_MANHATTAN: return assign_metric<PXSOM_METRIC_MANHATTAN>(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, dist_dev, ws, st);
    case PXSOM_METRIC_CHEBYSHEV: return assign_metric<PXSOM_METRIC_CHEBYSHEV>(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, dist_dev, ws, st);
    default: return assign_metric<PXSOM_METRIC_COSINE>(x_dev, n, c, ldx, dtype, w_dev, k, labels_dev, dist_dev, ws, st);
    }
}
