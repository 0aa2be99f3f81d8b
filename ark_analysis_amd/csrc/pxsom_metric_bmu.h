// pxsom_metric_bmu.h -- what the kernels of FlowSOM's other distances (distf 1, 3, 4) share: the prepared codebook and the
// search of one wave's 64 rows.  Used by pxsom_metric.hip (labels: pxsom_assign_metric) and pxsom_metric_step.hip (labels and
// batch statistics in one pass: pxsom_assign_sums_metric); each rule below is stated here once.
//
// Prepared codebook (workspace of metric_workspace_bytes(c, k)): a kHdrBytes header ([0]: unsigned, rows evaluated in binary64,
// what pxsom_assign_last_exact_rows reads), then wt[c][kp] -- the codebook transposed, kp = k rounded up to kNodeTile, zero
// nodes as padding --, then wn[kp], the nodes' norms sqrt(sum_j w_kj * w_kj), j ascending (cosine only).
//
// Search: one lane per row; at a fixed channel the kNodeTile nodes of a tile are kNodeTile consecutive, wave-uniform doubles
// (scalar loads), so the inner loop is two binary64 VALU instructions per (row, node, channel) term (three for Chebyshev).  Rows
// of up to kRegChannels channels are converted once into registers.  Wider rows are staged per wave, SCH channels of its 64 rows
// at a time: coalesced loads (SCH consecutive lanes read one row's segment), converted once to binary64 and written
// channel-major to the wave's own LDS slice, from which each lane reads its row conflict-free for the nodes of the tile.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "pxsom_common.h"
#include "pxsom_metric.h"
#include "pxsom_metric_step.h"

namespace pxsom_metric {

constexpr int kNodeTile = 16;     // accumulators per lane (32 VGPRs)
constexpr int kRegChannels = 32;  // rows held in registers (64 VGPRs) up to this width
constexpr size_t kHdrBytes = 256; // [0]: unsigned, rows evaluated in binary64 (pxsom_assign_last_exact_rows)
constexpr int kStageCh = 16;      // wider rows: channels per staged chunk
constexpr int kStagedWavesPerSimd = 4;   // occupancy the staged-row kernels are compiled for (128 VGPRs)
constexpr int kStageLd = 65;      // doubles between two channels of a chunk (odd: the staging writes spread over the banks)
// the staging slices of a 4-wave workgroup (33 KB at kStageCh channels per chunk)
constexpr size_t stage_bytes(int sch) { return (size_t)4 * sch * kStageLd * sizeof(double); }

inline int padded_nodes(int k) { return (k + kNodeTile - 1) / kNodeTile * kNodeTile; }

inline size_t metric_workspace_bytes(int c, int k)
{
    const size_t kp = (size_t)padded_nodes(k);
    return kHdrBytes + (size_t)c * kp * sizeof(double) + kp * sizeof(double);
}

// wt[j][kk] = w[kk][j] (zero for the padding nodes); wn[kk] = sqrt(sum_j w_kj * w_kj), j ascending (cosine only)
static __global__ __launch_bounds__(256) void metric_prep_kernel(const double *__restrict__ w, int k, int c, int kp,
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

struct Prepared {
    const double *wt, *wn;
    int kp;
};

// prepares the workspace `ws` (metric_workspace_bytes(c, k)) for the codebook w [k, c]; hdr[0] = rows
inline int launch_metric_prep(const double *w, int k, int c, int metric, char *ws, unsigned rows, hipStream_t st, Prepared *out)
{
    const int kp = padded_nodes(k);
    double *wt = reinterpret_cast<double *>(ws + kHdrBytes);
    double *wn = wt + (size_t)c * kp;
    const int pgrid = (int)std::min<int64_t>(((int64_t)c * kp + 255) / 256, 1024);
    hipLaunchKernelGGL(metric_prep_kernel, dim3(pgrid), dim3(256), 0, st, w, k, c, kp, wt, wn, reinterpret_cast<unsigned *>(ws),
                       rows, metric == PXSOM_METRIC_COSINE ? 1 : 0);
    PXSOM_LAUNCH_CHECK("metric_prep_kernel");
    out->wt = wt;
    out->wn = wn;
    out->kp = kp;
    return PXSOM_OK;
}

// The BMU of this lane's row among the nodes 0..k-1: FlowSOM's selection, nodes ascending -- first strict minimum below DBL_MAX
// (NaN never compares smaller); returns the node (-1: nothing compared smaller), *best its distance (DBL_MAX then).
// row_of(r), r in [0, 64): the row of the matrix that lane r of this wave works on (a valid row for every r: idle lanes repeat one).
// CX > 0: rows of c <= CX channels, converted once into xr (left there for the caller); CX == 0: any width, staged through
// xs, this wave's [SCH][kStageLd] slice of LDS.
template <int M, typename T, int CX, int SCH, typename RowOf>
__device__ __forceinline__ int bmu_search(const T *__restrict__ x, int64_t ldx, int c, RowOf row_of, int lane, double *xs,
                                          const double *__restrict__ wt, const double *__restrict__ wn, int k, int kp,
                                          double (&xr)[CX > 0 ? CX : 1], double *best_out)
{
#pragma clang fp contract(off)
    constexpr bool COS = M == PXSOM_METRIC_COSINE;
    const T *xp = x + row_of(lane) * ldx;
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
            for (int j0 = 0; j0 < c; j0 += SCH) {
                const int cw = min(SCH, c - j0);
                // LDS runs a wave's accesses in order: the previous chunk's reads precede these writes, the writes
                // precede the reads below (the wave barriers only keep the compiler from moving code across)
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int u = 0; u < SCH; u++) {
                    const int e = lane + 64 * u, r = e / SCH, ch = e % SCH;
                    if (ch < cw) xs[ch * kStageLd + r] = (double)x[row_of(r) * ldx + j0 + ch];
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
    *best_out = best;
    return bk;
}

}  // namespace pxsom_metric
