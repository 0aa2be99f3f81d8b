// pxsom_codebook_rules.h -- the small arithmetic rules by which a codebook is updated and prepared for the BMU filter, each stated
// once.  The batch rule and the filter agree with the oracle bit for bit only because every kernel that updates or prepares a
// codebook applies the same rules: prep_body (pxsom_prep.h), batch_step_kernel and batch_update_prep_kernel (pxsom_batch_step.hip),
// batch_step_wide_kernel (pxsom_batch_step_wide.hip), batch_update_kernel (pxsom_batch_train.hip).  The tolerance derivation
// (DESIGN.md "K7 error bound") rests on all of them choosing the same scale, the same unfit test and the same hi/lo split.
// A site whose kernel came out with other instructions when it called a rule keeps the rule written out under a comment that
// names it (profiles/codebook_rules/README.md has the table, site by site); the arithmetic of such a site is the rule's, to the letter.
#pragma once
#include <cfloat>
#include <cmath>

#include "pxsom_assign.h"

namespace pxsom_bmu {
namespace {

// R1 window radius: nodes b with max(|dx|, |dy|) <= thr  <=>  |dx|, |dy| <= floor(thr)   (integer distances)
__device__ __forceinline__ int window_radius(double thr) { return thr < 0.0 ? -1 : (thr > 1.0e6 ? 1000000 : (int)floor(thr)); }

// R2 gain and reciprocal of a node from the count of its window.  gain = 1 - (1-alpha)^den (batch_gain); == 1 exactly for wide
// windows: the node is then the window mean itself (orc_batch_update).  gain -1, inv 0: no rows, the node stays.
__device__ __forceinline__ void node_gain_inv(double den, double q, double sat, double &gain, double &inv)
{
    gain = den > 0.0 ? batch_gain(den, q, sat) : -1.0;
    inv = den > 0.0 ? 1.0 / den : 0.0;
}

// R3 node update.  gain == 1 exactly (wide windows): the node is the window mean itself, so nodes sharing a window are
// bit-identical (and masked as duplicates by the preparation) instead of one ulp apart (orc_batch_update)
__device__ __forceinline__ double node_update(double v, double gain, double mean)
{
#pragma clang fp contract(off)
    return gain == 1.0 ? mean : v + gain * (mean - v);
}

// R4 duplicate-key term of the step kernels: the bit pattern rotated by a channel-dependent amount, xor-ed up by the caller (no
// multiplies: integer multiplies run at quarter rate; a key match is verified channel by channel anyway).
// (prep_body hashes with two multiplications instead, on purpose: keys never leave a unit, so the two need not agree.)
__device__ __forceinline__ unsigned long long dup_key_term(double v, int ch)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    const int rot = (7 * ch + 1) & 63;
    return (bits << rot) | (bits >> ((64 - rot) & 63));
}

// R5 scale exponent: scale = 2^e with maxabs * scale in [128, 256) -- fp16 keeps 11 significant bits there and the low halves of the
// split stay normal down to |x| ~ 1e-4 * maxabs.  A codebook that has (nearly) collapsed onto the centring vector must not blow the
// scale up: rows lie as far from it as they did before, and x' * scale has to stay inside binary16 -- at most 2^6 over what the
// magnitude cap_norm alone would choose (0: no cap): the norm of the centring vector (step kernels: binary32, no reduction of
// their own for it) or the largest uncentred node norm (prep_body: binary64).
template <typename F>
__device__ __forceinline__ int scale_exponent(double maxabs, F cap_norm)
{
    int e = 0;
    if (maxabs > 0.0 && maxabs <= DBL_MAX) {
        int ex;
        frexp(maxabs, &ex);  // maxabs = m * 2^ex, m in [0.5, 1)
        e = 8 - ex;
        if (cap_norm > (F)0) {
            int exn;
            frexp(cap_norm, &exn);
            if (e > 8 - exn + 6) e = 8 - exn + 6;
        }
        if (e > 100) e = 100;
        if (e < -100) e = -100;
    }
    return e;
}

// R6 unfit codebook (NaN / Inf / huge): every row takes the exact path.  (maxabs * scale < 256 is what filter_cut_abs counts on: it
// fails only where the exponent clamp of R5 bit)
__device__ __forceinline__ bool codebook_unfit(bool bad, double wn2max, double maxabs, double scale)
{
    return bad || !(wn2max * scale * scale <= 1.0e30) || !(maxabs * scale < 256.0);
}

// R7 norm bounds wn_max (scaled, centred) and wn_raw (scale 1: the screened exact kernel's rounding bound is on the raw vectors):
// rounded up by a hair, 0 when unfit
__device__ __forceinline__ float norm_bound(double n2max, double scale, bool unfit)
{
    return unfit ? 0.f : (float)(sqrt(n2max) * scale * (1.0 + 1e-6));
}

// R8 fix_exp: a row the filter vouches for has |x' * scale|_2 < x_limit, hence |x_j * scale| < x_limit + max_j |mu_s_j|: below
// 2^(16 + t) for the smallest such t >= 0; fix_exp = e - t
template <typename MU>
__device__ __forceinline__ int fix_exp_shift(const MU *mu, int c, double scale)
{
    double mumax = 0.0;
    for (int j = 0; j < (c < kFilterMaxChannels ? c : kFilterMaxChannels); j++) mumax = fmax(mumax, fabs((double)mu[j]) * scale);
    int t = 0;
    while (t < 60 && !(60000.0 + mumax <= ldexp(65536.0, t))) t++;
    return t;
}

// R9 hi/lo split of a scaled weight into two binary16 values: hi = fl16(W), lo = fl16(W - hi) (the subtraction is exact in binary32)
__device__ __forceinline__ _Float16 split_hi(float W) { return (_Float16)W; }
__device__ __forceinline__ _Float16 split_lo(float W, _Float16 hi) { return (_Float16)(W - (float)hi); }

// R10 this workgroup's slice of the NEXT step's statistics buffer is cleared by the launch that applies the pending update (three
// buffers rotate): no clearing launch
template <int NT>
__device__ __forceinline__ void clear_stats_slice(double *stats_zero, int zero_count)
{
    if (stats_zero) {
        const int per = (zero_count + (int)gridDim.x - 1) / (int)gridDim.x;
        const int z1 = min(((int)blockIdx.x + 1) * per, zero_count);
        for (int e = (int)blockIdx.x * per + (int)threadIdx.x; e < z1; e += NT) stats_zero[e] = 0.0;
    }
}

// R11 (the housekeeping block and the load loop that three branches of batch_step_kernel repeat) and R12 (the output loops that
// batch_update_prep_kernel and prep_body share: fragments, bias, binary32 copy) have no definition here: as lambdas resp. function
// templates they changed the kernels of every caller (profiles/codebook_rules/README.md).  Those loops stay written out, and an
// edit to one of them is an edit to its twins.

}  // namespace
}  // namespace pxsom_bmu
