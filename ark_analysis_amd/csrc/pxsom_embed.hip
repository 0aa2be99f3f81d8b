// pxsom_embed.hip -- PCA scores and exact t-SNE of a cell table (K30; include/pxsom.h states the contract, DESIGN.md "K30").
//
// Everything is binary64.  No floating-point atomic, no waiting between workgroups: Z -> gradient -> next iteration is
// stream order.  Every sum runs over a fixed partition in a fixed order:
//   * a row of n pair terms: element j belongs to thread (j >> 1) & 255 of the row's workgroup; a thread adds its elements
//     in ascending j; the 64 lanes of a wave are folded by the xor pattern 32, 16, 8, 4, 2, 1 (both partners form the same
//     sum, so every lane holds the same bits); the four wave sums are added in wave order.  A workgroup of the step
//     kernels owns kStepRows rows and keeps one such sum per row, so the order per row does not depend on kStepRows;
//   * a vector of n per-row values (the row sums of Z, of the KL terms, of the squared gradient): element k belongs to
//     thread k & 255 of ONE workgroup, folded as above.  Z is therefore one number every workgroup reads;
//   * the column moments: rows in blocks of kMomentRows, a block's terms added in row order, the blocks in block order
//     (the blocks are summed side by side; the order of the additions does not depend on that).
#include "pxsom_common.h"

#include <cmath>
#include <limits>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStepRows = 4;        // rows of P one workgroup of the step kernels owns
constexpr int kMomentRows = 256;    // row block of pxsom_column_moments
constexpr int kDistTile = 16;       // pxsom_pair_sqdist_f32: a workgroup forms a 16 x 16 tile of d2
constexpr int kDistChunk = 32;      // ... from 32 channels at a time
constexpr int kJointTile = 32;      // the in-place symmetrisation swaps 32 x 32 tiles through LDS
constexpr double kEps = 2.220446049250313e-16;   // 2^-52, numpy's finfo(double).eps (sklearn's MACHINE_EPSILON)

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the sum of v over the workgroup, the same bits in every thread; lds holds kWaves doubles
__device__ __forceinline__ double block_sum(double v, double *lds)
{
    v = wave_sum(v);
    __syncthreads();   // (the previous sum's readers are done with lds)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// ---- column moments and projection -------------------------------------------------------------------------------------
// One workgroup per column (mean) or per entry of the covariance: thread t sums the row blocks t, t + 256, ..., each in row
// order, into LDS (parts: one double per row block, at most 4096 of them); thread 0 folds them in block order.
template <typename T>
__global__ __launch_bounds__(kThreads) void column_mean_kernel(const T *__restrict__ x, int64_t n, int c, double *__restrict__ mean)
{
    extern __shared__ double parts[];
    const int col = blockIdx.x, blocks = (int)((n + kMomentRows - 1) / kMomentRows);
    for (int b = threadIdx.x; b < blocks; b += kThreads) {
        const int64_t r0 = (int64_t)b * kMomentRows, r1 = r0 + kMomentRows < n ? r0 + kMomentRows : n;
        double part = 0.0;
        for (int64_t r = r0; r < r1; ++r) part += (double)x[r * c + col];
        parts[b] = part;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int b = 0; b < blocks; ++b) total += parts[b];
        mean[col] = total / (double)n;
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void column_cov_kernel(const T *__restrict__ x, int64_t n, int c,
                                                              const double *__restrict__ mean, double *__restrict__ cov)
{
    extern __shared__ double parts[];
    const int a = blockIdx.x / c, b2 = blockIdx.x % c, blocks = (int)((n + kMomentRows - 1) / kMomentRows);
    const double ma = mean[a], mb = mean[b2];
    for (int b = threadIdx.x; b < blocks; b += kThreads) {
        const int64_t r0 = (int64_t)b * kMomentRows, r1 = r0 + kMomentRows < n ? r0 + kMomentRows : n;
        double part = 0.0;
        for (int64_t r = r0; r < r1; ++r) part += ((double)x[r * c + a] - ma) * ((double)x[r * c + b2] - mb);
        parts[b] = part;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int b = 0; b < blocks; ++b) total += parts[b];
        cov[blockIdx.x] = total / (double)(n - 1);
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void project_rows_kernel(const T *__restrict__ x, int64_t n, int c,
                                                                const double *__restrict__ mean,
                                                                const double *__restrict__ axes, double *__restrict__ scores)
{
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    double s0 = 0.0, s1 = 0.0;
    for (int t = 0; t < c; ++t) {
        const double d = (double)x[r * c + t] - mean[t];
        s0 += d * axes[t];
        s1 += d * axes[c + t];
    }
    scores[2 * r] = s0;
    scores[2 * r + 1] = s1;
}

// ---- squared distances and affinities: one rounding per operation --------------------------------------------------------
#pragma clang fp contract(off)

template <typename T>
__global__ __launch_bounds__(kThreads) void pair_sqdist_kernel(const T *__restrict__ x, int n, int c, float *__restrict__ d2)
{
    __shared__ double xi[kDistTile][kDistChunk + 1], xj[kDistTile][kDistChunk + 1];
    const int tx = threadIdx.x & (kDistTile - 1), ty = threadIdx.x / kDistTile;
    const int i0 = blockIdx.y * kDistTile, j0 = blockIdx.x * kDistTile;
    double s = 0.0;
    for (int t0 = 0; t0 < c; t0 += kDistChunk) {
        for (int e = threadIdx.x; e < kDistTile * kDistChunk; e += kThreads) {
            const int r = e / kDistChunk, t = e % kDistChunk;
            const bool live = t0 + t < c;
            xi[r][t] = live && i0 + r < n ? (double)x[(int64_t)(i0 + r) * c + t0 + t] : 0.0;
            xj[r][t] = live && j0 + r < n ? (double)x[(int64_t)(j0 + r) * c + t0 + t] : 0.0;
        }
        __syncthreads();
        const int tmax = c - t0 < kDistChunk ? c - t0 : kDistChunk;
        for (int t = 0; t < tmax; ++t) {
            const double d = xi[ty][t] - xj[tx][t];
            s = s + d * d;
        }
        __syncthreads();
    }
    const int i = i0 + ty, j = j0 + tx;
    if (i < n && j < n) d2[(int64_t)i * n + j] = i == j ? 0.0f : (float)s;
}

// One workgroup per row: sklearn's _binary_search_perplexity.  The row of P is the scratch for exp(-d beta), as in sklearn;
// a thread reads back only what it wrote.  Leaves the conditional row (p / sum) in P and its sum in rowsum.
__global__ __launch_bounds__(kThreads) void tsne_conditional_kernel(const float *__restrict__ d2, int n, double target,
                                                                    double tol, double tiny, double *__restrict__ beta_out,
                                                                    int32_t *__restrict__ steps_out, double *__restrict__ P,
                                                                    double *__restrict__ rowsum)
{
    __shared__ double lds[kWaves];
    const int i = blockIdx.x;
    const float *drow = d2 + (int64_t)i * n;
    double *prow = P + (int64_t)i * n;
    double beta = 1.0, lo = -INFINITY, hi = INFINITY;
    int l = 0;
    for (;; ++l) {
        double part = 0.0;
        for (int j0 = 2 * threadIdx.x; j0 < n; j0 += 2 * kThreads)
            for (int j = j0; j < j0 + 2 && j < n; ++j) {
                if (j == i) continue;
                const double p = exp(-(double)drow[j] * beta);
                prow[j] = p;
                part += p;
            }
        double s = block_sum(part, lds);
        if (s == 0.0) s = tiny;
        part = 0.0;
        for (int j0 = 2 * threadIdx.x; j0 < n; j0 += 2 * kThreads)
            for (int j = j0; j < j0 + 2 && j < n; ++j) {
                if (j == i) continue;
                const double q = prow[j] / s;
                prow[j] = q;
                part += (double)drow[j] * q;
            }
        const double sd = block_sum(part, lds);
        const double diff = (log(s) + beta * sd) - target;
        if (fabs(diff) <= tol) break;
        if (diff > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
        }
        if (l == 99) break;     // (the row keeps the 100th evaluation; beta has moved on, as sklearn's has)
    }
    double part = 0.0;
    for (int j0 = 2 * threadIdx.x; j0 < n; j0 += 2 * kThreads)
        for (int j = j0; j < j0 + 2 && j < n; ++j)
            if (j != i) part += prow[j];
    const double total = block_sum(part, lds);
    if (threadIdx.x == 0) {
        prow[i] = 0.0;
        beta_out[i] = beta;
        steps_out[i] = l;
        rowsum[i] = total;
    }
}

// P = max((Pc + Pc^T) / max(sum, eps), eps) in place: a workgroup takes the tile (bi, bj), bi <= bj, and its mirror.
__global__ __launch_bounds__(kThreads) void tsne_joint_kernel(double *__restrict__ P, int n, const double *__restrict__ total)
{
    __shared__ double a[kJointTile][kJointTile + 1], b[kJointTile][kJointTile + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    const double sum_p = 2.0 * total[0] > kEps ? 2.0 * total[0] : kEps;
    const int i0 = bi * kJointTile, j0 = bj * kJointTile;
    for (int e = threadIdx.x; e < kJointTile * kJointTile; e += kThreads) {
        const int r = e / kJointTile, cc = e % kJointTile;
        a[r][cc] = i0 + r < n && j0 + cc < n ? P[(int64_t)(i0 + r) * n + j0 + cc] : 0.0;
        b[r][cc] = j0 + r < n && i0 + cc < n ? P[(int64_t)(j0 + r) * n + i0 + cc] : 0.0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kJointTile * kJointTile; e += kThreads) {
        const int r = e / kJointTile, cc = e % kJointTile;
        if (i0 + r < n && j0 + cc < n) {
            const double v = (a[r][cc] + b[cc][r]) / sum_p;
            P[(int64_t)(i0 + r) * n + j0 + cc] = v > kEps ? v : kEps;
        }
        if (bi != bj && j0 + r < n && i0 + cc < n) {
            const double v = (a[cc][r] + b[r][cc]) / sum_p;    // the same two addends as its mirror: P stays symmetric
            P[(int64_t)(j0 + r) * n + i0 + cc] = v > kEps ? v : kEps;
        }
    }
}

// sklearn's _gradient_descent on one parameter: gains, clip, grad *= gains, update, p += update.  Returns grad * gains.
__device__ __forceinline__ double descent_update(double g, double y, double momentum, double learning_rate, double min_gain,
                                                 double *__restrict__ update, double *__restrict__ gains,
                                                 double *__restrict__ y_out)
{
    const double u = *update;
    double gn = *gains;
    gn = u * g < 0.0 ? gn + 0.2 : gn * 0.8;
    gn = gn < min_gain ? min_gain : gn;
    g = g * gn;
    const double mu = momentum * u, lg = learning_rate * g;
    const double un = mu - lg;
    *gains = gn;
    *update = un;
    *y_out = y + un;
    return g;
}

// ---- one descent iteration ------------------------------------------------------------------------------------------------
// Still without contraction, with the fused steps written out: the gradient launch with and without the KL terms, and with
// and without 16-byte loads, forms the same operations and so the same bits.

// n_ij = 1 / (1 + |y_i - y_j|^2) and the two differences
__device__ __forceinline__ double student_weight(const double2 yi, const double2 yj, double &dx, double &dy)
{
    dx = yi.x - yj.x;
    dy = yi.y - yj.y;
    return 1.0 / (1.0 + fma(dx, dx, dy * dy));
}

// out0 = sum(v0), out1 = sqrt(sum(v1)): workgroup b folds vector b
__global__ __launch_bounds__(kThreads) void fold_kernel(const double *__restrict__ v0, const double *__restrict__ v1, int n,
                                                        double *__restrict__ out0, double *__restrict__ out1)
{
    __shared__ double lds[kWaves];
    const double *v = blockIdx.x == 0 ? v0 : v1;
    double part = 0.0;
    for (int k = threadIdx.x; k < n; k += kThreads) part += v[k];
    const double s = block_sum(part, lds);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0)
            *out0 = s;
        else
            *out1 = sqrt(s);
    }
}

// zrow[i] = sum over j != i of 1 / (1 + |y_i - y_j|^2)
__global__ __launch_bounds__(kThreads) void tsne_z_rows_kernel(const double2 *__restrict__ y, int n, double *__restrict__ zrow)
{
    __shared__ double lds[kWaves][kStepRows];
    const int i0 = blockIdx.x * kStepRows;
    double2 yi[kStepRows];
    double acc[kStepRows];
#pragma unroll
    for (int r = 0; r < kStepRows; ++r) {
        yi[r] = y[i0 + r < n ? i0 + r : n - 1];
        acc[r] = 0.0;
    }
    for (int j0 = 2 * threadIdx.x; j0 < n; j0 += 2 * kThreads) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = j0 + e;
            if (j >= n) break;
            const double2 yj = y[j];
#pragma unroll
            for (int r = 0; r < kStepRows; ++r) {
                double dx, dy;
                const double nn = student_weight(yi[r], yj, dx, dy);
                acc[r] += j == i0 + r ? 0.0 : nn;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kStepRows; ++r) {
        const double s = wave_sum(acc[r]);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][r] = s;
    }
    __syncthreads();
    if (threadIdx.x < kStepRows && i0 + (int)threadIdx.x < n) {
        const int r = threadIdx.x;
        zrow[i0 + r] = ((lds[0][r] + lds[1][r]) + lds[2][r]) + lds[3][r];
    }
}

struct StepArgs {
    const double *P;
    const double2 *y_in;
    double *y_out, *update, *gains, *grad;
    const double *z;
    double *klrow, *gnrow;
    int n;
    double exaggeration, momentum, learning_rate, min_gain;
};

// A stream over kStepRows rows of P: the gradient of those rows, their KL terms on demand, then the update of those rows.
// VEC: n is even and P is 16-byte aligned, so every pair (j, j + 1) of a row is one 16-byte load.
template <bool KL, bool VEC>
__global__ __launch_bounds__(kThreads) void tsne_gradient_kernel(StepArgs a)
{
    __shared__ double lds[kWaves][kStepRows][3];
    const int n = a.n, i0 = blockIdx.x * kStepRows;
    const double inv_z = 1.0 / a.z[0], ex = a.exaggeration;
    double2 yi[kStepRows];
    const double *prow[kStepRows];
    double g0[kStepRows], g1[kStepRows], kl[kStepRows];
#pragma unroll
    for (int r = 0; r < kStepRows; ++r) {
        const int i = i0 + r < n ? i0 + r : n - 1;      // a row past the end repeats the last one and is dropped below
        yi[r] = a.y_in[i];
        prow[r] = a.P + (int64_t)i * n;
        g0[r] = g1[r] = kl[r] = 0.0;
    }
    for (int j0 = 2 * threadIdx.x; j0 < n; j0 += 2 * kThreads) {
        double p[kStepRows][2];
        const bool two = j0 + 1 < n;
#pragma unroll
        for (int r = 0; r < kStepRows; ++r) {
            if (VEC) {
                const double2 v = *reinterpret_cast<const double2 *>(prow[r] + j0);
                p[r][0] = v.x;
                p[r][1] = v.y;
            } else {
                p[r][0] = prow[r][j0];
                p[r][1] = two ? prow[r][j0 + 1] : 0.0;
            }
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = j0 + e;
            if (e == 1 && !two) break;
            const double2 yj = a.y_in[j];
#pragma unroll
            for (int r = 0; r < kStepRows; ++r) {
                double dx, dy;
                const double nn = student_weight(yi[r], yj, dx, dy);
                double q = nn * inv_z;
                q = q > kEps ? q : kEps;
                const double pe = ex * p[r][e];
                const double w = (pe - q) * nn;     // at j == i: dx = dy = 0, the term is a zero
                g0[r] = fma(w, dx, g0[r]);
                g1[r] = fma(w, dy, g1[r]);
                if (KL) kl[r] += j == i0 + r ? 0.0 : pe * log((pe > kEps ? pe : kEps) / q);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kStepRows; ++r) {
        const double s0 = wave_sum(g0[r]), s1 = wave_sum(g1[r]), s2 = KL ? wave_sum(kl[r]) : 0.0;
        if ((threadIdx.x & 63) == 0) {
            lds[threadIdx.x >> 6][r][0] = s0;
            lds[threadIdx.x >> 6][r][1] = s1;
            lds[threadIdx.x >> 6][r][2] = s2;
        }
    }
    __syncthreads();
    if (threadIdx.x < kStepRows && i0 + (int)threadIdx.x < n) {
        const int r = threadIdx.x, i = i0 + r;
        double g[2], gn2 = 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            g[k] = 4.0 * (((lds[0][r][k] + lds[1][r][k]) + lds[2][r][k]) + lds[3][r][k]);
            if (a.grad) a.grad[2 * i + k] = g[k];
            const double y = k == 0 ? a.y_in[i].x : a.y_in[i].y;
            const double gg = descent_update(g[k], y, a.momentum, a.learning_rate, a.min_gain, a.update + 2 * i + k,
                                             a.gains + 2 * i + k, a.y_out + 2 * i + k);
            gn2 += gg * gg;
        }
        if (KL) {
            a.klrow[i] = ((lds[0][r][2] + lds[1][r][2]) + lds[2][r][2]) + lds[3][r][2];
            a.gnrow[i] = gn2;
        }
    }
}

#pragma clang fp contract(fast)

int check_rows(const char *fn, const void *x, int64_t n, int c, int dtype, int c_min)
{
    if (n < 1 || n > PXSOM_TSNE_MAX_ROWS) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: n=%lld outside [1, %d]", fn, (long long)n, PXSOM_TSNE_MAX_ROWS);
    if (c < c_min || c > PXSOM_MAX_CHANNELS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: c=%d outside [%d, %d]", fn, c, c_min, PXSOM_MAX_CHANNELS);
    if (dtype != PXSOM_F32 && dtype != PXSOM_F64) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: dtype %d", fn, dtype);
    if (!x) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null matrix", fn);
    return PXSOM_OK;
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// the doubles of the workspace: zrow [n], klrow [n], gnrow [n], z [2]; the affinities use zrow as their row sums
size_t workspace_doubles(int64_t n) { return 3 * (size_t)n + 2; }

}  // namespace

PXSOM_EXPORT size_t pxsom_tsne_workspace_bytes(int64_t n)
{
    if (n < 1 || n > PXSOM_TSNE_MAX_ROWS) return 0;
    return pxsom::align_up(workspace_doubles(n) * sizeof(double), 256);
}

PXSOM_EXPORT int pxsom_column_moments(const void *x_dev, int64_t n, int c, int dtype, double *mean_dev, double *cov_dev,
                                      void *stream)
{
    const char *fn = "pxsom_column_moments";
    if (int rc = check_rows(fn, x_dev, n, c, dtype, 2)) return rc;
    if (n < 2) return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: n=%lld < 2", fn, (long long)n);
    if (!mean_dev || !cov_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null output", fn);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned cov_grid = (unsigned)c * (unsigned)c;     // <= 2^20 workgroups
    const size_t lds = (size_t)((n + kMomentRows - 1) / kMomentRows) * sizeof(double);     // <= 32 KiB at PXSOM_TSNE_MAX_ROWS
    if (dtype == PXSOM_F32) {
        const float *x = static_cast<const float *>(x_dev);
        hipLaunchKernelGGL(column_mean_kernel<float>, dim3((unsigned)c), dim3(kThreads), lds, st, x, n, c, mean_dev);
        hipLaunchKernelGGL(column_cov_kernel<float>, dim3(cov_grid), dim3(kThreads), lds, st, x, n, c, mean_dev, cov_dev);
    } else {
        const double *x = static_cast<const double *>(x_dev);
        hipLaunchKernelGGL(column_mean_kernel<double>, dim3((unsigned)c), dim3(kThreads), lds, st, x, n, c, mean_dev);
        hipLaunchKernelGGL(column_cov_kernel<double>, dim3(cov_grid), dim3(kThreads), lds, st, x, n, c, mean_dev, cov_dev);
    }
    PXSOM_LAUNCH_CHECK("column_moments kernels");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_project_rows(const void *x_dev, int64_t n, int c, int dtype, const double *mean_dev,
                                    const double *axes_dev, double *scores_dev, void *stream)
{
    const char *fn = "pxsom_project_rows";
    if (int rc = check_rows(fn, x_dev, n, c, dtype, 1)) return rc;
    if (!mean_dev || !axes_dev || !scores_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)((n + kThreads - 1) / kThreads);
    if (dtype == PXSOM_F32)
        hipLaunchKernelGGL(project_rows_kernel<float>, dim3(grid), dim3(kThreads), 0, st, static_cast<const float *>(x_dev), n,
                           c, mean_dev, axes_dev, scores_dev);
    else
        hipLaunchKernelGGL(project_rows_kernel<double>, dim3(grid), dim3(kThreads), 0, st, static_cast<const double *>(x_dev),
                           n, c, mean_dev, axes_dev, scores_dev);
    PXSOM_LAUNCH_CHECK("project_rows_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_pair_sqdist_f32(const void *x_dev, int64_t n, int c, int dtype, float *d2_dev, void *stream)
{
    const char *fn = "pxsom_pair_sqdist_f32";
    if (int rc = check_rows(fn, x_dev, n, c, dtype, 1)) return rc;
    if (!d2_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null output", fn);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned tiles = (unsigned)((n + kDistTile - 1) / kDistTile);    // <= 65536 for n <= PXSOM_TSNE_MAX_ROWS
    if (dtype == PXSOM_F32)
        hipLaunchKernelGGL(pair_sqdist_kernel<float>, dim3(tiles, tiles), dim3(kThreads), 0, st,
                           static_cast<const float *>(x_dev), (int)n, c, d2_dev);
    else
        hipLaunchKernelGGL(pair_sqdist_kernel<double>, dim3(tiles, tiles), dim3(kThreads), 0, st,
                           static_cast<const double *>(x_dev), (int)n, c, d2_dev);
    PXSOM_LAUNCH_CHECK("pair_sqdist_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_tsne_affinities(const float *d2_dev, int64_t n, double perplexity, int joint, double *beta_dev,
                                       int32_t *steps_dev, double *p_dev, void *workspace_dev, size_t workspace_bytes,
                                       void *stream)
{
    const char *fn = "pxsom_tsne_affinities";
    if (n < 2 || n > PXSOM_TSNE_MAX_ROWS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: n=%lld outside [2, %d]", fn, (long long)n, PXSOM_TSNE_MAX_ROWS);
    if (!(perplexity > 0.0) || !std::isfinite(perplexity))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: perplexity %g", fn, perplexity);
    if (!d2_dev || !beta_dev || !steps_dev || !p_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (!workspace_dev || workspace_bytes < pxsom_tsne_workspace_bytes(n) || !aligned16(workspace_dev))
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", fn, workspace_bytes,
                           pxsom_tsne_workspace_bytes(n));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *rowsum = static_cast<double *>(workspace_dev), *total = rowsum + 3 * n;
    // sklearn's cdef floats: the perplexity, its tolerance 1e-5 and the replacement 1e-8 of a zero sum are binary32 values
    const double target = std::log((double)(float)perplexity), tol = (double)1e-5f, tiny = (double)1e-8f;
    hipLaunchKernelGGL(tsne_conditional_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, d2_dev, (int)n, target, tol, tiny,
                       beta_dev, steps_dev, p_dev, rowsum);
    PXSOM_LAUNCH_CHECK("tsne_conditional_kernel");
    if (!joint) return PXSOM_OK;
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(kThreads), 0, st, rowsum, rowsum, (int)n, total, total + 1);
    const unsigned tiles = (unsigned)((n + kJointTile - 1) / kJointTile);
    hipLaunchKernelGGL(tsne_joint_kernel, dim3(tiles, tiles), dim3(kThreads), 0, st, p_dev, (int)n, total);
    PXSOM_LAUNCH_CHECK("tsne_joint_kernel");
    return PXSOM_OK;
}

PXSOM_EXPORT int pxsom_tsne_step(const double *p_dev, int64_t n, const double *y_in_dev, double *y_out_dev, double *update_dev,
                                 double *gains_dev, double exaggeration, double momentum, double learning_rate,
                                 double min_gain, int want_error, double *error_and_gradnorm_dev, double *grad_dev,
                                 void *workspace_dev, size_t workspace_bytes, void *stream)
{
    const char *fn = "pxsom_tsne_step";
    if (n < 2 || n > PXSOM_TSNE_MAX_ROWS)
        return pxsom::fail(PXSOM_ERR_UNSUPPORTED, "%s: n=%lld outside [2, %d]", fn, (long long)n, PXSOM_TSNE_MAX_ROWS);
    if (!p_dev || !y_in_dev || !y_out_dev || !update_dev || !gains_dev || (want_error && !error_and_gradnorm_dev))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (y_in_dev == y_out_dev) return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: y_in and y_out are one buffer", fn);
    if (!aligned16(y_in_dev) || reinterpret_cast<uintptr_t>(p_dev) % 8 != 0)
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: y_in must be 16-byte and P 8-byte aligned", fn);
    if (!std::isfinite(exaggeration) || !std::isfinite(momentum) || !std::isfinite(learning_rate) || !std::isfinite(min_gain))
        return pxsom::fail(PXSOM_ERR_INVALID_ARG, "%s: a non-finite parameter", fn);
    if (!workspace_dev || workspace_bytes < pxsom_tsne_workspace_bytes(n) || !aligned16(workspace_dev))
        return pxsom::fail(PXSOM_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", fn, workspace_bytes,
                           pxsom_tsne_workspace_bytes(n));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *zrow = static_cast<double *>(workspace_dev), *klrow = zrow + n, *gnrow = klrow + n, *z = gnrow + n;
    const double2 *y_in = reinterpret_cast<const double2 *>(y_in_dev);
    const unsigned grid = (unsigned)((n + kStepRows - 1) / kStepRows);
    hipLaunchKernelGGL(tsne_z_rows_kernel, dim3(grid), dim3(kThreads), 0, st, y_in, (int)n, zrow);
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(kThreads), 0, st, zrow, zrow, (int)n, z, z + 1);
    StepArgs a;
    a.P = p_dev;
    a.y_in = y_in;
    a.y_out = y_out_dev;
    a.update = update_dev;
    a.gains = gains_dev;
    a.grad = grad_dev;
    a.z = z;
    a.klrow = klrow;
    a.gnrow = gnrow;
    a.n = (int)n;
    a.exaggeration = exaggeration;
    a.momentum = momentum;
    a.learning_rate = learning_rate;
    a.min_gain = min_gain;
    const bool vec = n % 2 == 0 && aligned16(p_dev);
    if (want_error) {
        if (vec)
            hipLaunchKernelGGL((tsne_gradient_kernel<true, true>), dim3(grid), dim3(kThreads), 0, st, a);
        else
            hipLaunchKernelGGL((tsne_gradient_kernel<true, false>), dim3(grid), dim3(kThreads), 0, st, a);
        hipLaunchKernelGGL(fold_kernel, dim3(2), dim3(kThreads), 0, st, klrow, gnrow, (int)n, error_and_gradnorm_dev,
                           error_and_gradnorm_dev + 1);
    } else {
        if (vec)
            hipLaunchKernelGGL((tsne_gradient_kernel<false, true>), dim3(grid), dim3(kThreads), 0, st, a);
        else
            hipLaunchKernelGGL((tsne_gradient_kernel<false, false>), dim3(grid), dim3(kThreads), 0, st, a);
    }
    PXSOM_LAUNCH_CHECK("tsne step kernels");
    return PXSOM_OK;
}
