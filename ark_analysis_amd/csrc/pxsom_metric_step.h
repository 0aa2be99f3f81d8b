// pxsom_metric_step.h -- what the batch driver (pxsom_batch_train.hip) takes from the kernels of FlowSOM's other distances
// (distf 1, 3, 4): host declarations only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pxsom.h"

namespace pxsom_metric {

inline bool metric_known(int metric) { return metric >= PXSOM_METRIC_MANHATTAN && metric <= PXSOM_METRIC_COSINE; }

// pxsom_metric_step.hip: labels (labels == NULL: none) and batch statistics of the rows i of x with e0 <= i % phases < e1, ADDED
// into stats [k*c sums | k counts], on the workspace ws (pxsom_metric_step_workspace_bytes(c, k, metric)).  scratch: room for the
// labels of the window's rows, or NULL -- with it (or with labels, for a window of every row) the shapes measured slower in one
// pass take two launches (DESIGN.md "K6m").  Arguments validated by the caller (pxsom_assign_sums_metric states the contract:
// include/pxsom.h).
int assign_sums_step(const void *x, int64_t n, int c, int64_t ldx, int dtype, const double *w, int k, int phases, int e0, int e1,
                     int32_t *labels, int32_t *scratch, double *stats, double qmagic, char *ws, int metric, hipStream_t st);

}  // namespace pxsom_metric
