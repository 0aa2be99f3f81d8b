// pxsom_sums.h -- per-cluster sums (pxsom_sums.hip): what the batch rule's driver takes from that unit
#ifndef PXSOM_SUMS_H
#define PXSOM_SUMS_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pxsom {

// sums[label - 1, :] += x[i, :], counts[label - 1] += 1 for rows with an even channel count, an even leading
// dimension and a pair-aligned base (channel PAIRS are loaded: 4 / 8 / 16 bytes for fp16 / fp32 / fp64).  counts_f64: the counts
// buffer holds binary64 (the batch rule's statistics) instead of int64.  nwv tables per workgroup.
// Returns false without launching when the shape is outside this kernel.
template <typename T>
bool launch_sums_pairs(const T *x, int64_t n, int c, int64_t ldx, const int32_t *labels, int k, double *sums,
                       void *counts, bool counts_f64, hipStream_t st, int nwv, int blocks_per_cu);

// sums[label - 1, :] += x[i, :], counts[label - 1] += 1 by the fastest kernel the shape has.  COUNT_F64: the counts buffer
// holds binary64 (the batch rule's statistics) instead of int64.  qmagic != 0 (binary64 rows of a reproducible training run,
// include/pxsom.h): values are rounded to the run's quantum as they are added.
template <typename T, bool COUNT_F64 = false>
int cluster_sums_typed(const T *x, int64_t n, int c, int64_t ldx, const int32_t *labels, int k, double *sums,
                       int64_t *counts, hipStream_t st, double qmagic = 0.0);

// whether cluster_sums_typed reads a scheduled step's rows where they lie (pxsom::RowView) on this shape
template <typename T>
bool sums_take_views(const T *x, int c, int64_t ldx, int k);

}  // namespace pxsom
#endif
