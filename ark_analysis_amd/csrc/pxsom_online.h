// pxsom_online.h -- K6a, the exact online SOM (pxsom_train_online[_ex|_metric]) on gfx950: kernels, launchers, shape dispatch.
//
//   Replaces pyFlowSOM.som: FlowSOM's C_SOM loop, n*rlen strictly sequential steps.  One persistent workgroup;
//   thread <-> SOM node; the binary64 codebook lives in LDS ([channel][node], so a wave's reads are conflict-free);
//   the presented rows are gathered 64 steps ahead into an LDS ring, so no step waits on HBM; one s_barrier per step.
//   Latency-bound by construction (neither roofline applies): DESIGN.md "K6a".
//
// Everything here is a template over the row type, and the instantiations (three row types x shape table x three extra
// metrics x in-place variant) are nearly all of the library's compile time.  So each row type is instantiated by a unit
// of its own -- pxsom_online_f32.hip, _f64.hip, _f16.hip, a third of the kernels each -- and the units compile side by
// side; pxsom_online.hip holds the entry points and instantiates nothing.
#pragma once
#include <cmath>

#include "pxsom_common.h"
#include "pxsom_metric.h"
#include "pxsom_wave.h"

// ------------------------------------------------------------------------------------------------
// The route of a shape: which kernel, how many threads, which chunk, how much LDS, codebook in place or not.  Decided
// here and only here -- the launchers below take the plan as it is, and pxsom_train_online_route reports it.
// Each table row is (node bound, channel bound, kernel form); the first row whose two bounds hold wins.
// ------------------------------------------------------------------------------------------------
// Euclidean, several lanes per node -- (K <=, c <=, CH channels per lane, L lanes per node): fewer binary64 instructions
// per wave per step on small maps; the 16 / 20 / 26 x 4 rows are the cell SOM's wide rows (~100 cluster-count features)
// on maps up to 128 nodes, 4 lanes per node in a 512-thread workgroup (two waves per SIMD)
#define PXSOM_ONLINE_SPLIT_ROUTES(X)                                             \
    X(64, 16, 4, 4) X(64, 24, 6, 4) X(64, 40, 10, 4)                             \
    X(128, 8, 4, 2) X(128, 16, 8, 2) X(128, 24, 12, 2) X(128, 40, 20, 2)         \
    X(128, 64, 16, 4) X(128, 80, 20, 4) X(128, 104, 26, 4)
// Euclidean, thread per node -- (K <=, c <=, CMAX, MAXT).  <= 256 nodes: 4 waves at most, the whole register file is
// available per thread (104: one wave per SIMD, 512 registers); <= 512 nodes (config 5's 20 x 20 map): two waves per
// SIMD, 256 registers per thread; more nodes or wider rows: 128 VGPRs per thread, the codebook stays out of registers
#define PXSOM_ONLINE_NODE_ROUTES(X)                                                                   \
    X(256, 8, 8, 256) X(256, 16, 16, 256) X(256, 24, 24, 256) X(256, 40, 40, 256) X(256, 64, 64, 256) \
    X(256, 104, 104, 256) X(256, PXSOM_MAX_CHANNELS, 0, 256)                                          \
    X(512, 8, 8, 512) X(512, 16, 16, 512) X(512, 24, 24, 512) X(512, 40, 40, 512)                     \
    X(PXSOM_MAX_NODES, PXSOM_MAX_CHANNELS, 0, 1024)
// Manhattan, Chebyshev, cosine: thread per node for every shape (the split kernel's several lanes per node would sum a
// node's channels out of the oracle's order); fewer register widths than the Euclidean route -- pad slots add exact zeros
#define PXSOM_ONLINE_METRIC_ROUTES(X)                                                                  \
    X(256, 8, 8, 256) X(256, 24, 24, 256) X(256, 40, 40, 256) X(256, 64, 64, 256)                      \
    X(256, PXSOM_MAX_CHANNELS, 0, 256) X(512, 16, 16, 512) X(512, 40, 40, 512)                         \
    X(PXSOM_MAX_NODES, PXSOM_MAX_CHANNELS, 0, 1024)

namespace pxsom {

// the record of pxsom_train_online_route, field for field (include/pxsom.h)
struct OnlinePlan {
    int family;     // PXSOM_ONLINE_LANES_PER_NODE / PXSOM_ONLINE_THREAD_PER_NODE
    int width;      // CH (channels per lane) / CMAX (register width; 0: the codebook is not in registers)
    int span;       // L (lanes per node) / MAXT (the kernel's thread bound)
    int in_place;   // CMAX 0 only: the codebook does not fit the LDS beside the row ring and is trained where it lies
    int threads;
    int chunk;      // steps whose rows are gathered ahead together
    int lds_bytes;
};

// K nodes x c channels (both validated by the caller) under `metric`.  Host arithmetic only.
inline int plan_online(int K, int c, int metric, OnlinePlan *p)
{
    *p = OnlinePlan{-1, 0, 0, 0, 0, 0, 0};
#define PXSOM_ROUTE(KB, CB, W, S)                           \
    if (p->family < 0 && K <= (KB) && c <= (CB)) {          \
        p->family = family;                                 \
        p->width = (W);                                     \
        p->span = (S);                                      \
    }
    int family = PXSOM_ONLINE_LANES_PER_NODE;
    if (metric == PXSOM_METRIC_EUCLIDEAN) {
        PXSOM_ONLINE_SPLIT_ROUTES(PXSOM_ROUTE)
    }
    family = PXSOM_ONLINE_THREAD_PER_NODE;
    if (metric == PXSOM_METRIC_EUCLIDEAN) {
        PXSOM_ONLINE_NODE_ROUTES(PXSOM_ROUTE)
    } else {
        PXSOM_ONLINE_METRIC_ROUTES(PXSOM_ROUTE)
    }
#undef PXSOM_ROUTE
    if (p->family < 0)
        return fail(PXSOM_ERR_UNSUPPORTED, "pxsom_train_online: %d nodes x %d channels: no kernel", K, c);
    if (p->family == PXSOM_ONLINE_LANES_PER_NODE) {
        const int CH = p->width, L = p->span;
        const int bd = ((K * L + 63) / 64) * 64;
        int chunk = 64;
        while ((chunk * c + bd - 1) / bd > 16) chunk >>= 1;  // gather registers per thread
        p->threads = bd;
        p->chunk = chunk;
        p->lds_bytes = (int)((size_t)2 * chunk * CH * L * 8 + (3 * 128 + 8) * 8 + (size_t)chunk * 8 +
                             (size_t)2 * chunk * 8 + (size_t)(CH * L + 2) * 8);
        return PXSOM_OK;
    }
    const int CMAX = p->width;
    const int bd = ((K + 63) / 64) * 64;
    const int nwv = bd / 64;
    const int cs = CMAX > 0 ? CMAX : c;
    // LDS besides the row ring: the codebook (CMAX == 0, when it fits) + per-wave exchange + learning rates
    auto plan = [&](bool codebook_in_lds, int *chunk_out) -> size_t {
        const size_t fixed = (codebook_in_lds ? (size_t)c * K * 8 : 0) + (size_t)2 * nwv * 8 + (size_t)2 * nwv * 4 +
                             (size_t)nwv * 8 + 2 * 64 * 8 + 64;
        int chunk = 64;
        while (chunk > 8 && fixed + (size_t)2 * chunk * cs * 8 > 150 * 1024) chunk >>= 1;
        while ((chunk * c + bd - 1) / bd > 16) chunk >>= 1;  // gather registers per thread
        *chunk_out = chunk;
        return fixed + (size_t)2 * chunk * cs * 8;
    };
    int chunk = 0;
    size_t lds = plan(CMAX == 0, &chunk);
    if (CMAX == 0 && (chunk < 1 || lds > 160 * 1024)) {  // the codebook does not fit beside the ring: train it where it lies
        p->in_place = 1;
        lds = plan(false, &chunk);
    }
    if (chunk < 1 || lds > 160 * 1024)
        return fail(PXSOM_ERR_UNSUPPORTED, "pxsom_train_online: %d nodes x %d channels: no LDS for the row ring", K, c);
    p->threads = bd;
    p->chunk = chunk;
    p->lds_bytes = (int)lds;
    return PXSOM_OK;
}

}  // namespace pxsom

namespace {

using pxsom::dpp_f64;
using pxsom::shr1_f64;
using pxsom::wave_min_f64;
using pxsom::wave_min_u32;

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// exact online SOM.  CMAX > 0: this thread's node (CMAX doubles) and the presented row live in
// registers -- per step one burst of LDS reads for the row, then pure register arithmetic in the
// oracle's order.  CMAX == 0: any channel count, codebook in LDS ([channel][node]) -- or, GLB, where it is:
// codebooks past the LDS (K * C * 8 > ~150 KB, e.g. 264 nodes x 128 channels) are trained in place in w
// (every thread touches only its own node's row; L2-resident, a few microseconds per step).
// ------------------------------------------------------------------------------------------------
// One term of FlowSOM's `change` accumulator (only ever consulted at the start of a pass, when rlen > 1).  The build reads the
// published loop as `change += fabs(tmp)`; PXSOM_ONLINE_INT_ABS is the other recollection -- C's integer abs(), i.e. the
// double truncated towards zero first, which makes every |tmp| < 1 count as 0 (oracle: ORC_V_INT_ABS).
__device__ __forceinline__ double change_term(double tmp, int flags)
{
    return ((flags & PXSOM_ONLINE_INT_ABS) && fabs(tmp) < 2147483648.0) ? (double)abs((int)tmp) : fabs(tmp);
}

// M: the BMU distance (PXSOM_METRIC_*); every other part of the loop is the same for all of them.
template <typename T, int CMAX, int MAXT, bool GLB = false, int M = PXSOM_METRIC_EUCLIDEAN>
__global__ __launch_bounds__(MAXT) void som_online_kernel(const T *__restrict__ x, int64_t n, int c,
                                                          int64_t ldx, double *w, int xdim, int ydim,
                                                          int rlen, double a0, double a1, double r0,
                                                          double r1, const int64_t *__restrict__ order,
                                                          int chunk, int flags)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int K = xdim * ydim;
    const int tid = threadIdx.x, bd = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6, nwv = bd >> 6;
    constexpr bool REG = CMAX > 0;
    static_assert(!(REG && GLB), "register-resident nodes need no codebook storage");
    double *wt = reinterpret_cast<double *>(smem_raw);            // [c][K] (LDS codebook; unused if REG / GLB)
    const int cs = REG ? CMAX : c;                                // row stride of the LDS ring
    double *xs = wt + ((REG || GLB) ? 0 : (size_t)c * K);         // [2][chunk][cs] (pad slots stay 0)
    double *exd = xs + (size_t)2 * chunk * cs;                    // [2][nwv] best distance per wave
    int *exk = reinterpret_cast<int *>(exd + 2 * nwv);            // [2][nwv] best node per wave
    double *red = reinterpret_cast<double *>(exk + 2 * nwv);      // [nwv] change partials
    double *alpha_ring = red + nwv;                               // [2][chunk] learning rate per step

    const bool has_node = tid < K;
    const int node = tid;
    const int nx = node / ydim, ny = node % ydim;
    // channel j of this thread's node, wherever the codebook lives
    auto wref = [&](int j) -> double & { return GLB ? w[(size_t)node * c + j] : wt[(size_t)j * K + node]; };
    double wr[REG ? CMAX : 1];
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < CMAX; j++) wr[j] = (has_node && j < c) ? w[(size_t)node * c + j] : 0.0;
    } else if constexpr (!GLB) {
        if (has_node)
            for (int j = 0; j < c; j++) wt[(size_t)j * K + node] = w[(size_t)node * c + j];
    }

    const int64_t niter = (int64_t)rlen * n;
    double threshold = r0;
    const double thresholdStep = (r0 - r1) / (double)niter;
    double change = 1.0;   // uniform: the epoch's total, known after the epoch-boundary reduction
    double mychange = 0.0; // this thread's share of the running epoch
    const bool track = rlen > 1;
    const int per_thread = (chunk * c + bd - 1) / bd;  // gathered elements per thread per chunk
    constexpr int kMaxPer = 16;
    T pre[kMaxPer];  // converted at commit: no use of a loaded value before its chunk is over

    // branch-free per lane (clamped element and step index): a load guarded by a divergent branch
    // gets its s_waitcnt right behind it, which serialises the HBM round trips
    auto gather = [&](int64_t step0) {
#pragma unroll
        for (int u = 0; u < kMaxPer; u++) {
            if (u < per_thread) {  // uniform
                const int e = min(tid + u * bd, chunk * c - 1);
                const int s = e / c, j = e - s * c;
                const int64_t st = step0 + s < niter ? step0 + s : niter - 1;
                pre[u] = x[order[st] * ldx + j];
            }
        }
    };
    // the oracle's alpha = a0 - (a0 - a1) * k / niter (same operation order), one lane per step,
    // so the binary64 division is off the per-step critical path
    auto alphas = [&](int buf, int64_t step0) {
        if (tid < chunk) {
            const int64_t kk = step0 + tid;
            alpha_ring[buf * chunk + tid] = a0 - (a0 - a1) * (double)kk / (double)niter;
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int u = 0; u < kMaxPer; u++) {
            const int e = tid + u * bd;
            if (u < per_thread && e < chunk * c) {
                const int srow = e / c, j = e - srow * c;
                xs[((size_t)buf * chunk + srow) * cs + j] = (double)pre[u];
            }
        }
    };

    // zero the ring once: slots j >= c of every row are never written again, so the unguarded
    // CMAX-long register loops below add exact zeros (x + 0 == x: bit-exactness is preserved)
    for (int e = tid; e < 2 * chunk * cs; e += bd) xs[e] = 0.0;
    __syncthreads();
    gather(0);
    commit(0);
    alphas(0, 0);
    __syncthreads();

    bool done = false;
    int par = 0;
    int64_t in_epoch = 0;  // step % n without a 64-bit division per step
    int cur_buf = 0;
    for (int64_t step0 = 0; step0 < niter && !done; step0 += chunk) {
        const int buf = cur_buf;
        gather(step0 + chunk);  // in flight while this chunk computes
        const double *xc = xs + (size_t)buf * chunk * cs;
        for (int s = 0; s < chunk; s++) {
            const int64_t step = step0 + s;
            if (step >= niter) break;
            int64_t k = step;
            const bool epoch_start = in_epoch == 0;
            if (++in_epoch == n) in_epoch = 0;
            if (epoch_start) {
                if (step > 0) {
                    // epoch boundary: total |delta| of the finished epoch (summation order differs
                    // from the oracle's sequential one; only `change < 1` is ever looked at)
                    double v = mychange;
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                    if (lane == 0) red[wv] = v;
                    __syncthreads();
                    change = 0.0;
                    for (int i = 0; i < nwv; i++) change += red[i];
                    __syncthreads();
                }
                if (change < 1.0) {
                    k = niter;  // FlowSOM: body runs once more with k == niter, then the loop ends
                    done = true;
                }
                change = 0.0;
                mychange = 0.0;
            }
            const double *xr = xc + (size_t)s * cs;
            double xreg[REG ? CMAX : 1];
            int nearest;
            if constexpr (M == PXSOM_METRIC_EUCLIDEAN) {
                // squared distance of this thread's node (binary64, j ascending) -- FlowSOM eucl() before
                // its sqrt.  The oracle compares sqrt(d2) values with a strict '<' (first minimum wins).
                // sqrt is monotone, so whenever the smallest d2 is isolated by more than a few ulps its
                // node is the answer and no sqrt is evaluated; only near-coincident candidates (d2 within
                // 2^-50 relative of the minimum) take the sqrt path, which reproduces the oracle's ties.
                double d2 = INFINITY;
                if constexpr (REG) {
#pragma unroll
                    for (int j = 0; j < CMAX; j++) xreg[j] = xr[j];  // one burst of broadcast LDS reads
                    double xdist = 0.0;
#pragma unroll
                    for (int j = 0; j < CMAX; j++) {
                        const double tmp = xreg[j] - wr[j];  // pad slots: 0 - 0
                        xdist += tmp * tmp;
                    }
                    if (has_node && xdist == xdist) d2 = xdist;
                } else if (has_node) {
                    double xdist = 0.0;
                    for (int j = 0; j < c; j++) {
                        const double tmp = xr[j] - wref(j);
                        xdist += tmp * tmp;
                    }
                    if (xdist == xdist) d2 = xdist;
                }
                const double near_eps = 8.881784197001252e-16;  // 2^-50
                double wmin = wave_min_f64(d2);
                unsigned long long cand = __ballot(d2 <= wmin + wmin * near_eps);
                int bk;
                double bd2;
                if (__popcll(cand) == 1) {
                    bk = (wv << 6) + (int)__ffsll((long long)cand) - 1;
                    bd2 = wmin;
                } else {
                    const double sd = sqrt(d2);
                    const double smin = wave_min_f64(sd);
                    cand = __ballot(sd == smin);
                    const int first = cand ? (int)__ffsll((long long)cand) - 1 : 0;
                    bk = (wv << 6) + first;
                    bd2 = __shfl(d2, first);
                }
                if (bk >= K) bk = 0x7fffffff;  // only padding lanes (all-infinite wave)
                nearest = bk;
                if (nwv > 1) {
                    if (lane == 0) {
                        exd[par * nwv + wv] = bd2;
                        exk[par * nwv + wv] = bk;
                    }
                    __syncthreads();
                    double gmin = exd[par * nwv];
                    for (int i = 1; i < nwv; i++) gmin = fmin(gmin, exd[par * nwv + i]);
                    const double lim = gmin + gmin * near_eps;
                    int ncand = 0;
                    for (int i = 0; i < nwv; i++) {
                        if (exd[par * nwv + i] <= lim) {
                            if (ncand == 0) nearest = exk[par * nwv + i];
                            ncand++;
                        }
                    }
                    if (ncand > 1) {  // near-coincident minima in different waves: compare like the oracle
                        double best = INFINITY;
                        nearest = 0x7fffffff;
                        for (int i = 0; i < nwv; i++) {
                            const double sdi = sqrt(exd[par * nwv + i]);
                            const int ki = exk[par * nwv + i];
                            if (sdi < best || (sdi == best && ki < nearest)) {
                                best = sdi;
                                nearest = ki;
                            }
                        }
                    }
                    par ^= 1;
                }
            } else {
                // FlowSOM's selection: nearest starts at node 0 and moves on `d[k] < d[nearest]` -- the first minimum over
                // the non-NaN distances, or node 0 when its own distance is NaN.  Keys: NaN -> +inf, node 0's NaN -> -inf
                // (exact comparisons from here on: the first lane / wave holding the minimum key is the oracle's node)
                double d = INFINITY;
                if constexpr (REG) {
#pragma unroll
                    for (int j = 0; j < CMAX; j++) xreg[j] = xr[j];
                    double acc = 0.0, d1 = 0.0, d2w = 0.0;
#pragma unroll
                    for (int j = 0; j < CMAX; j++) {  // pad slots: x = w = 0 leaves every accumulator unchanged
                        acc = pxsom_metric::term<M>(acc, xreg[j], wr[j]);
                        if constexpr (M == PXSOM_METRIC_COSINE) {
                            d1 = pxsom_metric::square_add(d1, xreg[j]);
                            d2w = pxsom_metric::square_add(d2w, wr[j]);
                        }
                    }
                    d = pxsom_metric::finish<M>(acc, sqrt(d1), sqrt(d2w));
                } else {
                    double acc = 0.0, d1 = 0.0, d2w = 0.0;
                    if (has_node) {
                        for (int j = 0; j < c; j++) {
                            const double wj = wref(j);
                            acc = pxsom_metric::term<M>(acc, xr[j], wj);
                            if constexpr (M == PXSOM_METRIC_COSINE) {
                                d1 = pxsom_metric::square_add(d1, xr[j]);
                                d2w = pxsom_metric::square_add(d2w, wj);
                            }
                        }
                    }
                    d = pxsom_metric::finish<M>(acc, sqrt(d1), sqrt(d2w));
                }
                const double key = !has_node ? INFINITY : d == d ? d : node == 0 ? -INFINITY : INFINITY;
                const double wmin = wave_min_f64(key);
                const unsigned long long cand = __ballot(key == wmin);
                nearest = (wv << 6) + (int)__ffsll((long long)cand) - 1;
                if (nwv > 1) {
                    if (lane == 0) {
                        exd[par * nwv + wv] = wmin;
                        exk[par * nwv + wv] = nearest;
                    }
                    __syncthreads();
                    double gmin = exd[par * nwv];
                    for (int i = 1; i < nwv; i++) gmin = fmin(gmin, exd[par * nwv + i]);
                    for (int i = nwv - 1; i >= 0; i--)
                        if (exd[par * nwv + i] == gmin) nearest = exk[par * nwv + i];
                    par ^= 1;
                }
            }
            if (nearest >= K) nearest = 0;
            if (threshold < 1.0) threshold = 0.5;
            const double alpha = k == step ? alpha_ring[buf * chunk + s]
                                           : a0 - (a0 - a1) * (double)k / (double)niter;  // early-stop step
            if (has_node) {
                const int bx = nearest / ydim, by = nearest % ydim;
                const int dx = nx > bx ? nx - bx : bx - nx, dy = ny > by ? ny - by : by - ny;
                const double nh = (double)(dx > dy ? dx : dy);
                if (!(nh > threshold)) {
                    if constexpr (REG) {
#pragma unroll
                        for (int j = 0; j < CMAX; j++) {
                            const double tmp = xreg[j] - wr[j];
                            if (track) mychange += change_term(tmp, flags);  // only ever consulted when rlen > 1
                            wr[j] = wr[j] + tmp * alpha;
                        }
                    } else {
                        for (int j = 0; j < c; j++) {
                            const double wv_ = wref(j);
                            const double tmp = xr[j] - wv_;
                            mychange += change_term(tmp, flags);
                            wref(j) = wv_ + tmp * alpha;
                        }
                    }
                }
            }
            threshold -= thresholdStep;
            if (done) break;
        }
        // publish the next chunk's rows (other buffer: nobody reads it during this chunk)
        commit(buf ^ 1);
        alphas(buf ^ 1, step0 + chunk);
        cur_buf ^= 1;
        __syncthreads();
    }
    if (has_node) {
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < CMAX; j++)
                if (j < c) w[(size_t)node * c + j] = wr[j];
        } else if constexpr (!GLB) {
            for (int j = 0; j < c; j++) w[(size_t)node * c + j] = wt[(size_t)j * K + node];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// exact online SOM, split form: L adjacent lanes share one node, each owning CH consecutive channels
// (K * L <= 256 threads: the Pixie default 10x10 x <= 24 markers runs as 4 waves, one per SIMD, 12
// channels per lane).  binary64 issue (~6.75 cycles per wave instruction) bounds the thread<->node
// form; splitting the channels cuts the per-wave instruction count.  The codebook update is
// element-wise and splits trivially.  The winner search runs in two tiers, both bit-faithful:
//  * every step: squared distances by a pairwise tree + butterfly (short dependency chain), wave minimum
//    on their upper 32 bits (one v_min_u32 DPP per stage).  The tree sum is within a few ulp of the
//    oracle's left-to-right sum, so it decides the step only when no other node's key is within one key
//    step (2^-21 relative) of the leader's -- then the oracle's winner is necessarily the same node;
//  * otherwise (near ties, duplicates, non-finite rows; block-uniform branch): the oracle's own
//    arithmetic -- lane q continues the strictly left-to-right partial sum of lane q-1 (row_shr:1 DPP),
//    so after L phases lane L-1 holds the oracle's value bit for bit -- a second exchange, and the
//    key / sqrt comparison of the thread<->node form.
// ------------------------------------------------------------------------------------------------
// scripts/ubench/online_step_timing.hip includes this header with PXSOM_STEP_TIMING defined: s_memtime
// deltas per step segment, accumulated by wave 0 (changes the schedule slightly; diagnosis only)
#ifdef PXSOM_STEP_TIMING
__device__ long long g_step_ticks[8];
#define PXSOM_TICK(i)                                 \
    do {                                              \
        const long long t_now = clock64();            \
        tick_acc[i] += t_now - tick_prev;             \
        tick_prev = t_now;                            \
    } while (0)
#else
#define PXSOM_TICK(i) \
    do {              \
    } while (0)
#endif

template <typename T, int CH, int L>
__global__ __launch_bounds__(CH * L > 40 ? 512 : 256) void som_online_split_kernel(const T *__restrict__ x, int64_t n, int c,
                                                               int64_t ldx, double *w, int xdim, int ydim,
                                                               int rlen, double a0, double a1, double r0,
                                                               double r1, const int64_t *__restrict__ order,
                                                               int chunk, int flags)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int CMAX = CH * L;
    constexpr int LOG_L = L == 4 ? 2 : 1;
    constexpr int NS = 128;  // distance slots per parity (K <= 128); slots >= K stay +inf
    const int K = xdim * ydim;
    const int tid = threadIdx.x, bd = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6, nwv = bd >> 6;
    double *xs = reinterpret_cast<double *>(smem_raw);        // [2][chunk][CMAX] (pad slots stay 0)
    double *dall = xs + (size_t)2 * chunk * CMAX;             // [2][NS] squared distance of every node
    double *dexact = dall + 2 * NS;                           // [NS] FlowSOM-order distances of a close call
    double *red = dexact + NS;                                // [8] change partials (one per wave)
    int64_t *ordl = reinterpret_cast<int64_t *>(red + 8);     // [chunk] rows presented in the next chunk
    double *alpha_ring = reinterpret_cast<double *>(ordl + chunk);  // [2][chunk] (+ CMAX doubles of slack:
                                                                    //  the one-step-ahead reads may overrun)

    const int node = tid >> LOG_L, q = tid & (L - 1);
    const bool has_node = node < K;
    const bool owner = has_node && q == L - 1;                // this lane ends up with the node's d2
    const int nx = node / ydim, ny = node % ydim;
    // every wave searches all K distances after the exchange: lane l looks at nodes 2l and 2l + 1
    const int pk0 = (2 * lane) | (((2 * lane) / ydim) << 8) | (((2 * lane) % ydim) << 16);
    const int pk1 = (2 * lane + 1) | (((2 * lane + 1) / ydim) << 8) | (((2 * lane + 1) % ydim) << 16);
    const int ch0 = q * CH;
    double wr[CH];
#pragma unroll
    for (int j = 0; j < CH; j++) wr[j] = (has_node && ch0 + j < c) ? w[(size_t)node * c + ch0 + j] : 0.0;

    const int64_t niter = (int64_t)rlen * n;
    double threshold = r0;
    const double thresholdStep = (r0 - r1) / (double)niter;
    double change = 1.0, mychange = 0.0;
    const bool track = rlen > 1;
    const int per_thread = (chunk * c + bd - 1) / bd;
    constexpr int kMaxPer = 16;
    T pre[kMaxPer];
    int64_t ord_pre = 0;

    // presented rows travel HBM -> registers -> LDS one chunk ahead of their use; their row numbers
    // (order[]) two chunks ahead, so neither dependent HBM round trip is ever waited on mid-chunk
    auto fetch_order = [&](int64_t step0) {  // branch-free as well (steps past the end re-read the last)
        const int64_t st = step0 + min(tid, chunk - 1);
        ord_pre = order[st < niter ? st : niter - 1];
    };
    auto publish_order = [&]() {
        if (tid < chunk) ordl[tid] = ord_pre;
    };
    // branch-free per lane (clamped element index, row 0 past the end): a load guarded by a divergent
    // branch gets its s_waitcnt right behind it, which serialises the HBM round trips
    auto gather = [&](int64_t) {
#pragma unroll
        for (int u = 0; u < kMaxPer; u++) {
            if (u < per_thread) {  // uniform
                const int e = min(tid + u * bd, chunk * c - 1);
                const int s = e / c, j = e - s * c;
                pre[u] = x[ordl[s] * ldx + j];
            }
        }
    };
    auto commit = [&](int buf, int64_t step0) {
#pragma unroll
        for (int u = 0; u < kMaxPer; u++) {
            const int e = tid + u * bd;
            if (u < per_thread && e < chunk * c) {
                const int srow = e / c, j = e - srow * c;
                xs[((size_t)buf * chunk + srow) * CMAX + j] = (double)pre[u];
            }
        }
        if (tid < chunk) {
            const int64_t kk = step0 + tid;
            alpha_ring[buf * chunk + tid] = a0 - (a0 - a1) * (double)kk / (double)niter;
        }
    };

    for (int e = tid; e < 2 * chunk * CMAX; e += bd) xs[e] = 0.0;
    for (int e = tid; e < 3 * NS; e += bd) dall[e] = INFINITY;  // dall and dexact
    fetch_order(0);
    publish_order();
    __syncthreads();
    gather(0);
    fetch_order(chunk);
    commit(0, 0);
    __syncthreads();  // everyone has consumed ordl (the loads above have returned)
    publish_order();
    __syncthreads();
    // nothing issued so far is still in flight: without this the s_waitcnt pass keeps a vmcnt(0) at
    // the top of the step loop, which would wait for every chunk's prefetch
    __builtin_amdgcn_s_waitcnt(0x0F70);

    bool done = false;
    int par = 0, buf = 0;
    int64_t in_epoch = 0;
    typedef double d2_t __attribute__((ext_vector_type(2)));
#ifdef PXSOM_STEP_TIMING
    long long tick_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tick_prev = clock64();
#endif
    for (int64_t step0 = 0; step0 < niter && !done; step0 += chunk) {
        fetch_order(step0 + 2 * chunk);  // row numbers of the chunk after the next
        gather(step0 + chunk);           // rows of the next chunk (their numbers are in ordl)
        const double *xc = xs + (size_t)buf * chunk * CMAX + ch0;
        PXSOM_TICK(7);
        // the row and learning rate of step s + 1 are read from LDS while step s computes
        double xcur[CH], alpha_cur = alpha_ring[buf * chunk];
#pragma unroll
        for (int j = 0; j < CH; j++) xcur[j] = xc[j];
        for (int s = 0; s < chunk; s++) {
            const int64_t step = step0 + s;
            if (step >= niter) break;
            int64_t k = step;
            const bool epoch_start = in_epoch == 0;
            if (++in_epoch == n) in_epoch = 0;
            if (epoch_start) {
                if (step > 0) {
                    double v = mychange;
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                    if (lane == 0) red[wv] = v;
                    __syncthreads();
                    change = 0.0;
                    for (int i = 0; i < nwv; i++) change += red[i];
                    __syncthreads();
                }
                if (change < 1.0) {
                    k = niter;
                    done = true;
                }
                change = 0.0;
                mychange = 0.0;
            }
            PXSOM_TICK(0);
            double tmp[CH], sq[CH];
#pragma unroll
            for (int j = 0; j < CH; j++) {
                tmp[j] = xcur[j] - wr[j];  // pad slots: 0 - 0
                sq[j] = tmp[j] * tmp[j];
            }
            const double alpha_ring_s = alpha_cur;
            {
                const double *xr = xc + (size_t)(s + 1) * CMAX;  // s + 1 == chunk: in-bounds, unused
#pragma unroll
                for (int j = 0; j < CH; j++) xcur[j] = xr[j];
                alpha_cur = alpha_ring[buf * chunk + s + 1];
            }
            // Squared distance, fast form: pairwise tree over the lane's channels, butterfly over the node's
            // L lanes.  It differs from FlowSOM's left-to-right sum by a few ulp at most (< 2^-47 relative),
            // so it may only decide a step whose runner-up is far away; see the key test below.
            double tsum[CH];
#pragma unroll
            for (int j = 0; j < CH; j++) tsum[j] = sq[j];
#pragma unroll
            for (int stride = 1; stride < CH; stride *= 2)
#pragma unroll
                for (int j = 0; j + stride < CH; j += 2 * stride) tsum[j] += tsum[j + stride];
            double dfast = tsum[0];
            dfast += dpp_f64(dfast, 0);
            if (L == 4) dfast += dpp_f64(dfast, 1);
            PXSOM_TICK(1);
            // all-to-all through LDS: one write, one barrier, one 16-byte read per lane; every wave then
            // finds the minimum of all K distances itself (no second exchange of per-wave winners)
            if (owner) dall[par * NS + node] = dfast == dfast ? dfast : INFINITY;
            __syncthreads();
            PXSOM_TICK(2);
            const d2_t df = *reinterpret_cast<const d2_t *>(dall + par * NS + 2 * lane);
            par ^= 1;
            // keys = upper 32 bits of d2 (sign, exponent, 20 mantissa bits).  Exactly one key within
            // {kmin, kmin + 1}: every other node is at least one whole key step (>= 2^-21 relative) above the
            // leader -- far more than the fast sum can be off -- so the leader is FlowSOM's winner as well.
            const unsigned fk0 = (unsigned)(__double_as_longlong(df[0]) >> 32);
            const unsigned fk1 = (unsigned)(__double_as_longlong(df[1]) >> 32);
            const unsigned fkmin = wave_min_u32(min(fk0, fk1));
            const unsigned long long near0 = __ballot(fk0 <= fkmin + 1u), near1 = __ballot(fk1 <= fkmin + 1u);
            int nearest;
            if (__popcll(near0) + __popcll(near1) == 1 && fkmin < 0x7ff00000u) {
                nearest = near0 ? __builtin_amdgcn_readlane(pk0, (int)__ffsll((long long)near0) - 1)
                                : __builtin_amdgcn_readlane(pk1, (int)__ffsll((long long)near1) - 1);
            } else {
                // close call (or no finite distance): redo the step with FlowSOM's own arithmetic.
                // eucl() before its sqrt: xdist = 0; xdist += tmp_j^2, j ascending over the node's channels
                // (0 + sq_0 == sq_0 exactly); lane q continues the partial sum of lane q - 1.
                double acc = sq[0];
#pragma unroll
                for (int j = 1; j < CH; j++) acc += sq[j];
#pragma unroll
                for (int p = 1; p < L; p++) {
                    double t = shr1_f64(acc);
#pragma unroll
                    for (int j = 0; j < CH; j++) t += sq[j];
                    acc = q == 0 ? acc : t;
                }
                if (owner) dexact[node] = acc == acc ? acc : INFINITY;
                __syncthreads();  // block-uniform branch: every wave read the same distances
                const d2_t dd = *reinterpret_cast<const d2_t *>(dexact + 2 * lane);
                // the oracle compares sqrt(d2) with a strict '<' in node order.  sqrt is monotone: a node
                // whose d2 is the only one with the smallest key wins outright; keys shared by several nodes
                // are settled on the sqrt values themselves.
                const unsigned key0 = (unsigned)(__double_as_longlong(dd[0]) >> 32);
                const unsigned key1 = (unsigned)(__double_as_longlong(dd[1]) >> 32);
                const unsigned kmin = wave_min_u32(min(key0, key1));
                unsigned long long cand0 = __ballot(key0 == kmin), cand1 = __ballot(key1 == kmin);
                if (__popcll(cand0) + __popcll(cand1) == 1) {
                    nearest = cand0 ? __builtin_amdgcn_readlane(pk0, (int)__ffsll((long long)cand0) - 1)
                                    : __builtin_amdgcn_readlane(pk1, (int)__ffsll((long long)cand1) - 1);
                } else {
                    const double s0 = key0 == kmin ? sqrt(dd[0]) : INFINITY;
                    const double s1 = key1 == kmin ? sqrt(dd[1]) : INFINITY;
                    const double sl = fmin(s0, s1);
                    const double smin = wave_min_f64(sl);
                    const unsigned long long cl = __ballot(sl == smin);
                    const int first = (int)__ffsll((long long)cl) - 1;  // lanes ascend in node order
                    const int p0 = __builtin_amdgcn_readlane(pk0, first), p1 = __builtin_amdgcn_readlane(pk1, first);
                    const bool zero_first = (__ballot(s0 == smin) >> first) & 1ull;
                    nearest = zero_first ? p0 : p1;
                    // no finite distance anywhere (NaN row, overflow): FlowSOM's loop never replaces node 0
                    if (!(smin < INFINITY)) nearest = 0;
                }
            }
            PXSOM_TICK(4);
            if (threshold < 1.0) threshold = 0.5;
            const double alpha = k == step ? alpha_ring_s : a0 - (a0 - a1) * (double)k / (double)niter;
            const int bx = (nearest >> 8) & 0xff, by = (nearest >> 16) & 0xff;
            const int dx = nx > bx ? nx - bx : bx - nx, dy = ny > by ? ny - by : by - ny;
            const double nh = (double)(dx > dy ? dx : dy);
            if (has_node && !(nh > threshold)) {
#pragma unroll
                for (int j = 0; j < CH; j++) wr[j] = wr[j] + tmp[j] * alpha;
                if (track) {  // only ever consulted when rlen > 1
#pragma unroll
                    for (int j = 0; j < CH; j++) mychange += change_term(tmp[j], flags);
                }
            }
            threshold -= thresholdStep;
            PXSOM_TICK(5);
            if (done) break;
        }
        commit(buf ^ 1, step0 + chunk);
        publish_order();
        buf ^= 1;
        __syncthreads();
        PXSOM_TICK(6);
    }
#ifdef PXSOM_STEP_TIMING
    if (tid == 0)
        for (int i = 0; i < 8; i++) g_step_ticks[i] = tick_acc[i];
#endif
    if (has_node) {
#pragma unroll
        for (int j = 0; j < CH; j++)
            if (ch0 + j < c) w[(size_t)node * c + ch0 + j] = wr[j];
    }
}

#pragma clang fp contract(fast)

// the arguments of one training run, as the kernels take them
template <typename T>
struct OnlineArgs {
    const T *x;
    int64_t n;
    int c;
    int64_t ldx;
    double *w;
    int xdim, ydim, rlen;
    double a0, a1, r0, r1;
    const int64_t *order;
    int flags;
    hipStream_t st;
};

// Both launchers take the plan as it is (pxsom::plan_online): threads, chunk, LDS bytes and the in-place decision are
// computed there and nowhere else.
template <typename T, typename Kernel>
int launch_planned(Kernel kern, const char *name, const pxsom::OnlinePlan &p, const OnlineArgs<T> &a, bool raise_lds)
{
    if (raise_lds)
        PXSOM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, p.lds_bytes));
    hipLaunchKernelGGL(kern, dim3(1), dim3(p.threads), (size_t)p.lds_bytes, a.st, a.x, a.n, a.c, a.ldx, a.w, a.xdim, a.ydim,
                       a.rlen, a.a0, a.a1, a.r0, a.r1, a.order, p.chunk, a.flags);
    PXSOM_LAUNCH_CHECK(name);
    return PXSOM_OK;
}

template <typename T, int CMAX, int MAXT, int M>
int launch_online(const pxsom::OnlinePlan &p, const OnlineArgs<T> &a)
{
    if constexpr (CMAX == 0) {
        if (p.in_place) return launch_planned(som_online_kernel<T, CMAX, MAXT, true, M>, "som_online_kernel", p, a, true);
    }
    return launch_planned(som_online_kernel<T, CMAX, MAXT, false, M>, "som_online_kernel", p, a, true);
}

template <typename T, int CH, int L>
int launch_online_split(const pxsom::OnlinePlan &p, const OnlineArgs<T> &a)
{
    return launch_planned(som_online_split_kernel<T, CH, L>, "som_online_split_kernel", p, a, p.lds_bytes > 48 * 1024);
}

// The kernel of a plan: one instantiation per row of the route tables (the rows name CH x L or CMAX x MAXT once each).
template <typename T, int M>
int launch_online_plan(const pxsom::OnlinePlan &p, const OnlineArgs<T> &a)
{
    if constexpr (M == PXSOM_METRIC_EUCLIDEAN) {
#define PXSOM_ROUTE(KB, CB, CH, L) \
    if (p.family == PXSOM_ONLINE_LANES_PER_NODE && p.width == CH && p.span == L) return launch_online_split<T, CH, L>(p, a);
        PXSOM_ONLINE_SPLIT_ROUTES(PXSOM_ROUTE)
#undef PXSOM_ROUTE
    }
#define PXSOM_ROUTE(KB, CB, CM, MT) \
    if (p.family == PXSOM_ONLINE_THREAD_PER_NODE && p.width == CM && p.span == MT) return launch_online<T, CM, MT, M>(p, a);
    if constexpr (M == PXSOM_METRIC_EUCLIDEAN) {
        PXSOM_ONLINE_NODE_ROUTES(PXSOM_ROUTE)
    } else {
        PXSOM_ONLINE_METRIC_ROUTES(PXSOM_ROUTE)
    }
#undef PXSOM_ROUTE
    return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "pxsom_train_online: no kernel for plan %d / %d / %d", p.family, p.width, p.span);
}

}  // namespace

namespace pxsom {

// One online training run on rows of type T (arguments validated by the caller, n > 0 and rlen > 0).
// metric: PXSOM_METRIC_*.
template <typename T>
int train_online(const T *x, int64_t n, int c, int64_t ldx, double *w, int xdim, int ydim, int rlen, double a0, double a1,
                 double r0, double r1, const int64_t *order, int metric, int flags, hipStream_t st)
{
    OnlinePlan p;
    const int rc = plan_online(xdim * ydim, c, metric, &p);
    if (rc) return rc;
    const OnlineArgs<T> a{x, n, c, ldx, w, xdim, ydim, rlen, a0, a1, r0, r1, order, flags, st};
    switch (metric) {
    case PXSOM_METRIC_MANHATTAN: return launch_online_plan<T, PXSOM_METRIC_MANHATTAN>(p, a);
    case PXSOM_METRIC_CHEBYSHEV: return launch_online_plan<T, PXSOM_METRIC_CHEBYSHEV>(p, a);
    case PXSOM_METRIC_COSINE: return launch_online_plan<T, PXSOM_METRIC_COSINE>(p, a);
    default: return launch_online_plan<T, PXSOM_METRIC_EUCLIDEAN>(p, a);
    }
}

// `template int pxsom::train_online<T>(PXSOM_ONLINE_ARGS(T));` in the unit of row type T and nowhere else
#define PXSOM_ONLINE_ARGS(T) \
    const T *, int64_t, int, int64_t, double *, int, int, int, double, double, double, double, const int64_t *, int, int, hipStream_t
extern template int train_online<float>(PXSOM_ONLINE_ARGS(float));
extern template int train_online<double>(PXSOM_ONLINE_ARGS(double));
extern template int train_online<_Float16>(PXSOM_ONLINE_ARGS(_Float16));

}  // namespace pxsom
