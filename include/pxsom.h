/*
 * pxsom.h -- C ABI of libpxsom.so: the MI355X (gfx950) implementation of ark-analysis' Pixie
 * pixel/cell SOM hot path.
 *
 * The reference (pure Python) reaches its native arithmetic through exactly two foreign calls
 * into the Cython package pyFlowSOM (/root/reference/src/ark/phenotyping/cluster_helpers.py:14):
 *     som(data, xdim, ydim, rlen, alpha_range, seed)            cluster_helpers.py:106-109
 *     map_data_to_nodes(weights, data)[0]                       cluster_helpers.py:152-157
 * plus numpy/scipy/pandas loops for normalisation, blur, quantiles and per-cluster means
 * (pixie_preprocessing.py:47-75, pixel_cluster_utils.py:16-142, 369-404).  Every entry point
 * below names the reference interface it replaces.  INTEGRATION.md shows the ctypes binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - plain C, no exceptions cross the ABI; every function returns PXSOM_OK (0) or a negative
 *     pxsom_status; pxsom_last_error() returns a thread-local message for the last failure.
 *   - "dev" pointers are device (HBM) pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()); the library allocates nothing persistent.  Scratch comes from a caller
 *     workspace sized by the matching *_workspace_bytes() query.
 *   - every launch is ordered on the caller's stream (void* = hipStream_t; NULL = default
 *     stream); calls are asynchronous unless documented otherwise; re-entrant per stream.
 *   - matrices are row-major [rows, c] with a row stride ldx given in ELEMENTS.
 *   - SOM nodes: node k = x*ydim + y on the xdim*ydim grid; labels are 1-based (k+1), as
 *     pyFlowSOM returns them (tests/phenotyping/cluster_helpers_test.py:388-391 of the reference).
 */
#ifndef PXSOM_H
#define PXSOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PXSOM_ABI_VERSION 9

typedef enum pxsom_status {
    PXSOM_OK = 0,
    PXSOM_ERR_INVALID_ARG = -1,
    PXSOM_ERR_UNSUPPORTED = -2, /* shape / dtype outside what the kernels are built for */
    PXSOM_ERR_WORKSPACE = -3,   /* workspace NULL or too small */
    PXSOM_ERR_HIP = -4          /* a HIP runtime call failed; see pxsom_last_error() */
} pxsom_status;

typedef enum pxsom_dtype {
    PXSOM_F32 = 0, /* IEEE binary32 pixel matrix (BASELINE.json configs 2-4) */
    PXSOM_F64 = 1, /* IEEE binary64 pixel matrix (what the reference's feather tables hold) */
    PXSOM_F16 = 2  /* IEEE binary16 pixel matrix (BASELINE.json config 5); every value is used as the exact
                      real number it encodes -- results equal those for the same values held in binary64 */
} pxsom_dtype;

/* Limits of the gfx950 kernels in this build.  Rows of up to 128 channels take the MFMA filter + exact recheck; wider
 * rows (the cell SOM over the 400 cluster counts of a 20 x 20 pixel SOM: cell_cluster_utils.py:63-192) are evaluated
 * directly in the oracle's arithmetic -- same labels, a lower rate, sized for cell tables (10^5 .. 10^6 rows). */
#define PXSOM_MAX_CHANNELS 1024
#define PXSOM_MAX_NODES 1024

int pxsom_abi_version(void);
const char *pxsom_last_error(void);

/* ---- in-library kernel timer --------------------------------------------------------------
 * HIP event pairs recorded on the launch stream immediately around the dominant kernel of each
 * pxsom_assign call (the BMU filter kernel) whose row count is >= min_rows, while a profiler is
 * attached to the calling thread.  pxsom_prof_collect synchronises on the recorded events and
 * returns the summed kernel time and the number of launches, then resets.  bench.py uses it for
 * the roofline figure (the same duration rocprofv3 --kernel-trace reports for that kernel). */
int pxsom_prof_create(void **out_handle);
int pxsom_prof_destroy(void *handle);
int pxsom_prof_attach(void *handle_or_null, int64_t min_rows);
int pxsom_prof_collect(void *handle, double *total_ms, int64_t *launches);

/* ---- host helper (no GPU) ------------------------------------------------------------------
 * glibc rand() stream (TYPE_3 additive feedback), the presentation-order generator of the
 * pyFlowSOM-compatible som() front end (replaces the libc srand/rand pair inside pyFlowSOM's
 * Cython loop, cluster_helpers.py:106-109 passes `seed`). out[i] in [0, 2^31). */
int pxsom_host_glibc_rand_fill(uint32_t seed, int64_t count, int32_t *out);

/* ---- BMU assignment: replaces pyFlowSOM.map_data_to_nodes -----------------------------------
 * reference: cluster_helpers.py:150-157 (PixieSOMCluster.generate_som_clusters).
 * labels_dev[i] = 1 + argmin_k sqrt(sum_j (x_ij - w_kj)^2), evaluated as the reference does in
 * binary64 with first-minimum tie-break; rows containing NaN get label 0 (FlowSOM's minid=-1).
 *   x_dev      [n, c] row-major, dtype, row stride ldx elements
 *   w_dev      [k, c] row-major binary64 codebook
 *   labels_dev [n] int32 out
 *   dist_dev   [n] binary64 out, or NULL (the reference discards it: `[0]` at :157)
 * Mechanism: fp16-split MFMA filter + exact binary64 re-evaluation of every row whose two best
 * scores are closer than a rigorous error bound (DESIGN.md "K7").  Result is independent of
 * the filter: bit-identical to the oracle. */
size_t pxsom_assign_workspace_bytes(int64_t n, int c, int k);
int pxsom_assign(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev,
                 int k, int32_t *labels_dev, double *dist_dev, void *workspace_dev,
                 size_t workspace_bytes, void *stream);
/* pxsom_assign with flags (ABI 9).  PXSOM_ASSIGN_SCREEN_ALL_LISTS: every list of rows for the exact path goes through the
 * long-list kernel (binary32 screening, binary64 for the surviving nodes), whatever its length -- by default lists shorter than
 * ~2.25e6 / c rows take the wave-per-row kernel.  Same labels either way; the flag exists so that the long-list kernel can be
 * exercised on small inputs (a per-call argument: the library reads no environment variables). */
#define PXSOM_ASSIGN_SCREEN_ALL_LISTS 1
int pxsom_assign_ex(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev,
                    int k, int32_t *labels_dev, double *dist_dev, void *workspace_dev,
                    size_t workspace_bytes, int flags, void *stream);

/* Number of rows the last pxsom_assign on this workspace sent to the exact binary64 path
 * (diagnostic; synchronises the stream). */
int pxsom_assign_last_exact_rows(const void *workspace_dev, void *stream, int64_t *out_rows);

/* ---- per-cluster sums / counts: replaces the pandas groupby in compute_pixel_cluster_channel_avg
 * reference: pixel_cluster_utils.py:369-404.  ADDS into sums_dev [k, c] binary64 and
 * counts_dev [k] int64 (caller zeroes them; lets several FOVs / ranks accumulate):
 *   sums[labels[i]-1, :] += x[i, :];  counts[labels[i]-1] += 1     (labels outside 1..k skipped)
 * Also the accumulation half of the batch SOM rule (step 2 of DESIGN.md "K6b"). */
int pxsom_cluster_sums(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype,
                       const int32_t *labels_dev, int k, double *sums_dev, int64_t *counts_dev,
                       void *stream);

/* ---- labels and per-cluster sums / counts in one pass over x ------------------------------------------
 * pxsom_assign followed by pxsom_cluster_sums, reading the pixel matrix ONCE: what cluster_pixels + generate_som_avg_files
 * compute together when the labelled rows are still in HBM (reference: cluster_helpers.py:150-157 +
 * pixel_cluster_utils.py:369-404).  labels_dev as pxsom_assign; sums_dev / counts_dev are ADDED into, as pxsom_cluster_sums.
 * Register-resident shapes (K = 97..100, even c <= 32, pair-aligned rows) take the fused launch; other shapes run the two
 * kernels one after the other.  Workspace: pxsom_assign_sums_workspace_bytes(n, c, k).
 * ACCURACY CONTRACT (since ABI 7): labels and counts are exact; on the fused launch the SUMS are accumulated in 64-bit
 * fixed point inside a workgroup -- every value enters rounded to a multiple of 2^-s, s = 46 + e - max(11, ceil(log2(rows a
 * workgroup meets))), 2^e the filter's power-of-two scale (|W|max * 2^e in [128, 256)) -- i.e. an absolute error per value of at
 * most 2^-28 * rows-per-workgroup / 2^11 relative to the codebook's largest magnitude (1.8e-12 for 41 K rows per workgroup),
 * then flushed as binary64.  They are therefore NOT the bit-exact binary64 sums of pxsom_assign + pxsom_cluster_sums, but
 * within 1e-6 relative of them per mean (tests: test_assign_sums_one_pass_equals_two_passes).  Values outside the format
 * (>= 2^(16 - e), non-finite) and listed rows bypass the table in binary64.  (ABI 9: the environment switch PXSOM_SUMS_F64 is
 * gone -- the library reads no environment variable; exact binary64 tables: pxsom_assign + pxsom_cluster_sums.) */
size_t pxsom_assign_sums_workspace_bytes(int64_t n, int c, int k);
/* ABI 9.  The workspace of pxsom_assign_sums / pxsom_assign_means begins with a statistics region of
 * pxsom_assign_sums_scratch_bytes(c, k) bytes (it does not move with n); the assign workspace follows it (pass
 * `workspace + scratch bytes` to pxsom_assign_last_exact_rows).  Every successful call LEAVES THAT REGION ZERO.  The _ex forms take
 * flags: PXSOM_TABLES_SCRATCH_CLEAN -- the caller vouches that the region is zero on entry (it cleared the workspace once when it
 * allocated it, and every call since returned PXSOM_OK): the call skips its clearing launch (~6 us in front of a 0.22 ms kernel).
 * After a failed call, clear the region (or drop the flag once). */
#define PXSOM_TABLES_SCRATCH_CLEAN 1
size_t pxsom_assign_sums_scratch_bytes(int c, int k);
int pxsom_assign_sums_ex(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                         int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, void *workspace_dev,
                         size_t workspace_bytes, int flags, void *stream);
int pxsom_assign_means_ex(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                          int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, double *means_dev, void *workspace_dev,
                          size_t workspace_bytes, int flags, void *stream);
int pxsom_assign_sums(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                      int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, void *workspace_dev,
                      size_t workspace_bytes, void *stream);

/* The same pass with the tables OVERWRITTEN (no clearing by the caller) and the per-cluster means formed in the same
 * final launch: means_dev [k, c] = sums / max(count, 1), or NULL.  What generate_som_avg_files needs from one process
 * (pixel_cluster_utils.py:369-404); a multi-rank job all-reduces sums / counts and divides itself. */
int pxsom_assign_means(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                       int32_t *labels_dev, double *sums_dev, int64_t *counts_dev, double *means_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);

/* ---- cell x pixel-cluster counts: the counting step of create_c2pc_data --------------------------
 * reference: cell_cluster_utils.py:128-141 (groupby(['label', pixel_cluster_col]).size() + pivot per
 * FOV).  hist[a_i * nb + b_i] += 1 for every i with 0 <= a_i < na and 0 <= b_i < nb (other pairs are
 * ignored); hist_dev [na, nb] int64 is accumulated into, the caller clears it.  Exact integer counts. */
int pxsom_pair_histogram(const int32_t *a_dev, const int32_t *b_dev, int64_t n, int64_t na, int nb,
                         int64_t *hist_dev, void *stream);

/* ---- exact online SOM training: replaces pyFlowSOM.som -------------------------------------
 * reference: cluster_helpers.py:106-109 (PixieSOMCluster.train_som), FlowSOM C_SOM semantics:
 * n*rlen strictly sequential steps; step t presents row order_dev[t]; Euclidean BMU (first
 * minimum); every node within Chebyshev grid distance <= threshold of the BMU moves by
 * alpha*(x - w); alpha and threshold decay linearly (a0->a1, r0->r1; threshold pinned to 0.5
 * once below 1).  All arithmetic binary64, one rounding per operation, in the oracle's order.
 *   w_dev [k=xdim*ydim, c] binary64, in: initial nodes, out: trained nodes
 *   order_dev [n*rlen] int64 presentation order (explicit input, never generated here) */
int pxsom_train_online(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *w_dev,
                       int xdim, int ydim, int rlen, double a0, double a1, double r0, double r1,
                       const int64_t *order_dev, void *stream);
/* The same with `flags` for the RECALLED details of the loop (pyFlowSOM 0.1.16 is absent from the build image: each
 * recollection is a named switch, oracle/pxsom_oracle.c ORC_V_*).  PXSOM_ONLINE_INT_ABS: the accumulator behind the
 * "stop at the start of a pass when change < 1" test adds C's integer abs() of each difference -- truncated towards zero
 * first, so every |x - w| < 1 counts as 0 -- instead of fabs() (oracle: ORC_V_INT_ABS).  Only observable with rlen >= 2. */
#define PXSOM_ONLINE_INT_ABS 1
int pxsom_train_online_ex(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *w_dev,
                          int xdim, int ydim, int rlen, double a0, double a1, double r0, double r1,
                          const int64_t *order_dev, int flags, void *stream);

/* ---- batch SOM training (throughput mode; no pyFlowSOM analogue) -----------------------------
 * One mini-batch step = pxsom_batch_accumulate [+ all-reduce of stats across ranks] + pxsom_batch_update.
 * stats_dev is [k*c sums | k counts], all binary64 (counts are exact integers), so the collective is a
 * single sum over one buffer.
 *   accumulate: zero stats; labels = BMU(x rows, w) (pxsom_assign; labels_dev [n] int32 scratch that also
 *               returns them); stats[b, :] += x_i, stats_count[b] += 1 for b = label_i - 1.
 *   update:     num[k] = sum_{b: cheb(k,b) <= thr} sums[b], den[k] = sum_{b: ...} counts[b]
 *               (summed in orc_batch_update's separable order: along y inside a grid row, then over the rows)
 *               den[k] > 0:  w[k] += (1 - (1-alpha)^den[k]) * (num[k] * (1/den[k]) - w[k])
 *               (the gain is formed as -expm1(den * log1p(-alpha)))
 *   update_prepare: the same update with sums/counts = the two halves of stats_dev; the same launch clears
 *               stats_next_dev, the buffer the next accumulate will fill (alternate two buffers; NULL or
 *               == stats_dev: cleared by a separate fill), so the next
 *               pxsom_batch_accumulate(..., PXSOM_ACC_PREPARED, ...) is a single launch for the
 *               register-resident shapes (the accumulating filter prepares the codebook itself); other
 *               shapes get workspace_dev prepared for the new codebook here (may be NULL otherwise).
 * Oracle of record: oracle/pxsom_oracle.c orc_cluster_sums / orc_batch_update. */
#define PXSOM_ACC_PREPARED 1 /* flags: stats_dev was cleared (and the workspace prepared) by update_prepare */
int pxsom_batch_accumulate(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype,
                           const double *w_dev, int k, int32_t *labels_dev, double *stats_dev,
                           void *workspace_dev, size_t workspace_bytes, int flags, void *stream);
int pxsom_batch_update(double *w_dev, int xdim, int ydim, int c, const double *sums_dev,
                       const double *counts_dev, double thr, double alpha, void *stream);
int pxsom_batch_update_prepare(double *w_dev, int xdim, int ydim, int c, double *stats_dev,
                               double *stats_next_dev, double thr, double alpha, void *workspace_dev,
                               size_t workspace_bytes, void *stream);

/* ---- batch SOM training, one call per run of steps ------------------------------------------------
 * The host loop over the mini-batch steps of a pass, inside the library (no per-step Python / ctypes work).
 * Step g of total_steps (= num_passes * batch_steps) uses the rows i = (g % batch_steps) + r * batch_steps of
 * x_dev and the schedule thr/alpha(g) of orc_som_batch.  State, all caller-owned:
 *   wbuf_dev        [2][k*c] binary64: W_g, the codebook step g searches with, lives in wbuf[g % 2].
 *                   Before the first call the caller stores W_0 in wbuf[0].
 *   stats_ring_dev  [3][k*(c+1)] binary64: step g leaves its [k*c sums | k counts] in ring[g % 3] and clears
 *                   ring[(g+1) % 3]; the call with g_begin == 0 clears ring[0] first.
 * A single process runs [0, total_steps) in one call.  A multi-rank job runs ONE step per call and sum-all-reduces
 * ring[g % 3] across ranks before the next call (the only exchange of the rule).  After the last step (and its
 * all-reduce) pxsom_batch_train_finish applies the last pending update: w_out_dev [k, c] receives W_total.
 * Register-resident shapes (10 x 10 grid, even c <= 32, rows 2-element aligned) take ONE launch per step: the
 * pending update of step g-1 and the codebook preparation run at the head of step g's BMU search in every
 * workgroup; other shapes run update / prepare / search / exact / sums launches per step -- except steps of up to
 * 16 384 binary32 / binary64 rows on codebooks of up to 256 nodes x 128 channels that fit a CU's LDS, which take ONE
 * launch as well (csrc/pxsom_batch_step_wide.hip): the steps whose pending update has its threshold pinned at 0.5 on any
 * grid (a node's window is the node), the others -- up to 4 096 rows -- on grids up to 16 x 16.  Same results either way (PXSOM_TRAIN_UNFUSED forces
 * the launch-per-phase route for every step).  Oracle of record: oracle/pxsom_oracle.c orc_som_batch. */
#define PXSOM_TRAIN_UNFUSED 1
/* (flag value 2 was PXSOM_TRAIN_PERSISTENT_TAIL in ABI 6 - 8: an opt-in persistent launch for the BMU-only tail, measured slower
 * than the launches it replaced and removed in ABI 9; the bit is ignored.) */
/* A test switch of the fused 10 x 10 step (csrc/pxsom_batch_step.hip): the two bucket tables of its duplicate-node test
 * shrink to 4 buckets each, so that every node collides and the linear scan behind the tables runs.  Same results. */
#define PXSOM_TRAIN_SMALL_DUP_TABLES 4
size_t pxsom_batch_train_workspace_bytes(int64_t n, int batch_steps, int c, int k);
int pxsom_batch_train_steps(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *wbuf_dev,
                            double *stats_ring_dev, int xdim, int ydim, int batch_steps, int g_begin, int g_end,
                            int total_steps, double a0, double a1, double r0, double r1, void *workspace_dev,
                            size_t workspace_bytes, int flags, void *stream);
int pxsom_batch_train_finish(const double *wbuf_dev, const double *stats_ring_dev, int xdim, int ydim, int c,
                             int steps_done, int total_steps, double a0, double a1, double r0, double r1,
                             double *w_out_dev, void *stream);

/* ---- batch SOM training on a SCHEDULE (round 3): unequal mini-batch steps ----------------------------------
 * The rows are dealt into `phases` phases (row i: phase i % phases); step g of a pass takes the phases
 * [edges[g], edges[g+1]) (edges_host [steps_per_pass + 1], edges[0] == 0, edges[steps_per_pass] == phases,
 * non-decreasing; steps_per_pass <= PXSOM_MAX_SCHED_STEPS).  Its update is taken at the point of the online schedule
 * (threshold, alpha) where the rows presented before it end: (pass * phases + edges[g]) / (num_passes * phases).
 * Equal steps (edges = 0..phases) are pxsom_batch_train_steps, bit for bit.  A step is one latency-bound launch
 * whatever its size, so a pass is priced in steps: few large steps while the neighbourhood is wide, many small ones
 * in the BMU-only tail reach the quality of 64 equal steps in under half the launches (DESIGN.md "K6b").
 * State (wbuf_dev, stats_ring_dev), routes, flags and comm as pxsom_batch_train_steps[_sharded]; steps are numbered
 * over the whole run, g in [0, num_passes * steps_per_pass); the call with g_begin == 0 must come first on a workspace
 * (it clears ring[0] and, for shapes outside the fused kernel with steps wider than one phase whose kernels do not all read a
 * step's rows where they lie -- 32 channels or fewer, binary64 rows, rows not contiguous in x, a per-cluster table small enough
 * for the wave-private sums kernels --, gathers the rows into step order inside the workspace: one extra read + write of the
 * matrix per run; round 6: other shapes are read in place).  Every rank runs the same steps.
 * The WORKSPACE IS RUN STATE, like wbuf and the ring: the g_begin == 0 call also leaves the run's centring vector (the
 * mean of W_0 per channel and its norm, read by every later step's filter) in it, so the calls of one run must be given
 * the same, untouched workspace; a later call on a fresh or foreign workspace would centre on whatever bytes it finds
 * (results stay exact -- every label is settled against the binary64 codebook -- but most rows would be listed).
 * Oracle of record: oracle/pxsom_oracle.c orc_som_batch_sched.  Reference call replaced: cluster_helpers.py:98-116. */
/* Reproducible statistics for binary64 rows (sum_quantum > 0; ignored for binary32 / binary16 rows).  The per-BMU sums
 * of a step are floating-point additions in whatever order the workgroups and ranks deliver them.  binary32 / binary16 rows
 * whose partial sums all fit binary64's 53 bits (counts-like data, binary16 values) give exact, order-free sums; wider
 * ranges (values far below the sums they join) can round a sum in its last bit.  For binary64 rows that
 * order leaves 1e-16 noise which the degenerate first steps of a pass (near-identical nodes) can amplify into different
 * BMUs -- two runs on the same data then end in different codebooks, where the reference pins same-seed retraining
 * (tests/phenotyping/cluster_helpers_test.py:323-332 of the reference).  With sum_quantum = q (a power of two) every
 * value enters the statistics rounded to a multiple of q (round-half-even; the BMU search still sees the value itself);
 * q = pxsom_exact_sum_quantum(max |x| over the job's rows, most rows any step holds over all ranks) makes every partial
 * sum exactly representable, hence every addition exact, hence the statistics -- and the whole run -- independent of
 * order, workgroup count and rank count.  The rounding is part of the rule: orc_som_batch_sched takes the same q.
 * pxsom_absmax: max |x| over the finite entries of a matrix into out_dev[0] (0 when there is none: a matrix of
 * NaN / +-inf only, or n = 0; a negative entry counts by its magnitude). */
double pxsom_exact_sum_quantum(double value_bound, int64_t rows_bound);
int pxsom_absmax(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *out_dev, void *stream);

#define PXSOM_MAX_SCHED_STEPS 256
typedef struct pxsom_comm pxsom_comm; /* the library-owned RCCL communicator, below */
size_t pxsom_batch_train_sched_workspace_bytes(int64_t n, int c, int k, int dtype, int phases, const int32_t *edges_host,
                                               int steps_per_pass);
int pxsom_batch_train_sched(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *wbuf_dev,
                            double *stats_ring_dev, int xdim, int ydim, int phases, const int32_t *edges_host,
                            int steps_per_pass, int g_begin, int g_end, int num_passes, double a0, double a1, double r0,
                            double r1, double sum_quantum, void *workspace_dev, size_t workspace_bytes, int flags,
                            pxsom_comm *comm, void *stream);
/* The same with the run's first codebook W_0 handed over where the caller holds it (ABI 9): w0_dev [k, c] or NULL.  With g_begin
 * == 0 the launch that prepares the run copies it into wbuf_dev[0] itself -- no copy launch in front of a pass of 22 short steps;
 * w0_dev may be the buffer pxsom_batch_train_sched_finish later writes into.  Ignored when g_begin > 0. */
int pxsom_batch_train_sched_from(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w0_dev, double *wbuf_dev,
                                 double *stats_ring_dev, int xdim, int ydim, int phases, const int32_t *edges_host,
                                 int steps_per_pass, int g_begin, int g_end, int num_passes, double a0, double a1, double r0,
                                 double r1, double sum_quantum, void *workspace_dev, size_t workspace_bytes, int flags,
                                 pxsom_comm *comm, void *stream);
int pxsom_batch_train_sched_finish(const double *wbuf_dev, const double *stats_ring_dev, int xdim, int ydim, int c,
                                   int phases, const int32_t *edges_host, int steps_per_pass, int steps_done,
                                   int num_passes, double a0, double a1, double r0, double r1, double *w_out_dev,
                                   void *stream);
/* 1 when the steps of this matrix / shape take the one-launch fused kernel, 0 for the launch-per-phase route.  The
 * ranks of a job agree on the route before the run (MIN over ranks, PXSOM_TRAIN_UNFUSED for all otherwise): the two
 * routes round the codebook's last bits differently, and every rank must hold the same codebook. */
int pxsom_batch_train_fused_route(const void *x_dev, int c, int64_t ldx, int dtype, int xdim, int ydim, int phases);

/* ---- the exchange of a multi-rank batch run, inside the library ---------------------------------------
 * One process per GPU, rows sharded by rank: the rule's only exchange is the sum of ring[g % 3] over the ranks
 * after every step.  pxsom_batch_train_steps_sharded is pxsom_batch_train_steps with that all-reduce (RCCL,
 * in place, binary64) enqueued on `stream` right behind each step's launch, so a whole run of steps is one call
 * here as well -- no host work between a step and its exchange.  comm == NULL: no exchange (single rank).
 * RCCL is bound at run time: pxsom_comm_bind(path of the librccl.so this process uses; NULL = "librccl.so.1")
 * once per process; rank 0 draws the id with pxsom_comm_unique_id and hands it to the other ranks by whatever
 * channel launched them (the Python host uses the torch.distributed store); every rank then calls
 * pxsom_comm_create -- collective -- with its HIP device current.  Every rank must run the same steps.
 * The reference has no analogue (single-core training, cluster_helpers.py:106-109). */
#define PXSOM_COMM_ID_BYTES 128
int pxsom_comm_bind(const char *librccl_path);
int pxsom_comm_unique_id(void *id_out, size_t id_bytes);
int pxsom_comm_create(const void *id, size_t id_bytes, int nranks, int rank, pxsom_comm **out);
int pxsom_comm_destroy(pxsom_comm *comm);
int pxsom_comm_allreduce_sum_f64(pxsom_comm *comm, double *buf_dev, size_t count, void *stream);
/* One-shot peer-to-peer exchange (round 4; csrc/pxsom_comm.hip): every rank owns an exchange block in its device memory,
 * mapped by the others through HIP IPC; an exchange is ONE launch per rank (write the own contribution into every block,
 * flag, wait for the others' flags, add the slots in rank order: bit-identical sums on all ranks).  Ranks may share a
 * device (two processes on one GPU: how a one-GPU box validates the protocol) or sit on the devices of one node.
 *   create(nranks <= 16, rank, max_count binary64 values per exchange) -> handle(64 bytes; gather them from all ranks,
 *   rank order) -> connect(all handles).  The communicator then serves pxsom_comm_allreduce_sum_f64 and
 *   pxsom_batch_train_sched like an RCCL one.  pxsom_comm_p2p_error: 0, or the epoch at which a peer failed to arrive
 *   within 4 s (that exchange's buffer was set to NaN; the GPU is not left hanging; the FIRST such epoch stays on record).
 * pxsom_comm_p2p_set_fused(comm, 1) (ABI 9; EVERY rank, same value): pxsom_batch_train_sched on such a communicator runs the
 * exchange INSIDE the launches of the fused 10 x 10 step (the last workgroup of a step writes this rank's statistics into every
 * block, the next step adds the slots in rank order while it applies the update: the same bits as the one-launch exchange, one
 * launch per step); a peer that is late there turns the codebook to NaN, sets the same error word, and this rank still raises
 * its flags (over NaN slots) so that nobody waits for it.  The last step of a call and every other shape keep the one-launch
 * exchange.  The switch is a property of the communicator (no process-wide state). */
#define PXSOM_P2P_HANDLE_BYTES 64
int pxsom_comm_p2p_create(int nranks, int rank, size_t max_count, pxsom_comm **out);
int pxsom_comm_p2p_handle(pxsom_comm *comm, void *handle_out, size_t handle_bytes);
int pxsom_comm_p2p_connect(pxsom_comm *comm, const void *handles, size_t handles_bytes);
int pxsom_comm_p2p_error(pxsom_comm *comm, unsigned long long *epoch_out);
int pxsom_comm_p2p_set_fused(pxsom_comm *comm, int on);
/* pxsom_batch_train_steps with the exchange enqueued behind every step (comm: RCCL or peer-to-peer; NULL = none).  Equal
 * steps only: 1 <= batch_steps <= PXSOM_MAX_SCHED_STEPS (256) and total_steps a whole number of passes (total_steps %
 * batch_steps == 0) -- other values are PXSOM_ERR_INVALID_ARG since ABI 7; schedules: pxsom_batch_train_sched. */
int pxsom_batch_train_steps_sharded(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *wbuf_dev,
                                    double *stats_ring_dev, int xdim, int ydim, int batch_steps, int g_begin,
                                    int g_end, int total_steps, double a0, double a1, double r0, double r1,
                                    void *workspace_dev, size_t workspace_bytes, int flags, pxsom_comm *comm,
                                    void *stream);

/* ---- pre-processing (create_fov_pixel_data and the 99.9 % values) -----------------------------
 * reference: pixie_preprocessing.py:47-49 -> scipy.ndimage.gaussian_filter(plane, sigma) per channel:
 * separable, 'reflect' boundary, axis 0 then axis 1, binary64, scipy's symmetric-kernel summation
 * order.  weights_host [2*radius+1] is the normalised kernel exactly as scipy builds it
 * (numpy exp / sum on the host: part of the reference numerics), radius = int(4*sigma + 0.5).
 * img_dev [h, w, c] binary64 interleaved, blurred in place; tmp_dev: same-size scratch. */
#define PXSOM_BLUR_GENERIC_FORM 2 /* OR-ed into f32_semantics: the thread-per-output kernel for every shape (the pipeline's
                                    radius-8 blur otherwise runs a register-window pass down the rows and an LDS-tiled pass
                                    along the columns; same results bit for bit -- the tests compare the two) */
int pxsom_gaussian_blur_hwc(double *img_dev, double *tmp_dev, int h, int w, int c,
                            const double *weights_host, int radius, int f32_semantics, void *stream);
/* f32_semantics (here and below): the matrix holds float32 values widened to binary64 -- what the
 * pipeline feeds create_fov_pixel_data for float32 TIFFs (pixie_preprocessing.py:152-159).  scipy then
 * stores every blur pass as float32 and pandas sums / divides the float32 frame in binary32; with the flag
 * the kernels round in exactly those places, so the results are the reference's float32 values (widened). */

/* reference: pixie_preprocessing.py:67-75 + pixel_cluster_utils.normalize_rows (:126-130):
 * keep pixel i iff rowsum_i > thresh and any(x_ij != 0); out row = x_i / rowsum_i (left-to-right
 * binary64 row sum, as pandas computes it).  Kept rows are compacted in pixel order.
 * As in pandas, the row sum skips NaN (DataFrame.sum, skipna) and NaN != 0 holds: a row with a NaN is judged by the
 * sum of its other values, and its NaN entries stay NaN.  The comparison with thresh is strict; a kept row whose
 * sum is 0 or infinite comes out as the division gives it (inf, NaN, 0).
 *   out_rows_dev [<= n, c] binary64, out_index_dev [<= n] int64 flat pixel index of each kept row,
 *   out_count_dev [1] int64.  workspace from pxsom_rownorm_workspace_bytes(n). */
size_t pxsom_rownorm_workspace_bytes(int64_t n);
int pxsom_rowsum_filter_normalize(const double *x_dev, int64_t n, int c, double thresh,
                                  double *out_rows_dev, int64_t *out_index_dev,
                                  int64_t *out_count_dev, void *workspace_dev,
                                  size_t workspace_bytes, int f32_semantics, void *stream);

/* reference: PixelSOMCluster.normalize_data (cluster_helpers.py:242-246): x[:, j] / norm[j] in
 * binary64 (in place allowed: out_dev may equal x_dev). */
int pxsom_normalize_columns(const double *x_dev, int64_t n, int c, int64_t ldx,
                            const double *norm_dev, double *out_dev, int64_t ldo, void *stream);

/* reference: df.replace(0, nan).quantile(q) per column (pixie_preprocessing.py:406-408,
 * cluster_helpers.py:366) / np.quantile(img[img > 0], q) (pixel_cluster_utils.py:47-51):
 * type-7 (linear) quantile of the kept values (keep_mode 0: != 0 and not NaN, 1: > 0, 2: not NaN) of each
 * column.
 * out_dev [c] binary64 (NaN for a column with no kept value).  Exact: MSB-first radix select on the
 * binary64 bit patterns, then numpy's interpolation formula.  Note pandas' effective q is (q*100)/100.
 * Infinite values are kept and ordered like numbers; where numpy's interpolation then meets inf - inf the result is
 * NaN, as numpy's is.  The select orders -0.0 below +0.0, numpy's sort leaves their order open: the SIGN of a zero
 * result may differ from numpy's (keep_mode 2 only; the other modes drop zeros), its value does not. */
size_t pxsom_quantile_workspace_bytes(int64_t n, int c);
int pxsom_quantile_nonzero(const double *x_dev, int64_t n, int c, int64_t ldx, double q,
                           int keep_mode, double *out_dev, void *workspace_dev,
                           size_t workspace_bytes, void *stream);

/* reference: np.quantile(img[img > 0], percentile) on a float32 image (calculate_channel_percentiles,
 * pixel_cluster_utils.py:41-51) and np.quantile(summed_data, 0.05) (calculate_pixel_intensity_percentile,
 * :96-103).  Same radix select on float32 columns; index, fraction and interpolation in binary32 exactly as
 * numpy forms them for a float32 array.  keep_mode 2 keeps every non-NaN value.  out_dev [c] binary64
 * holding the float32 results. */
int pxsom_quantile_f32(const float *x_dev, int64_t n, int c, int64_t ldx, double q, int keep_mode,
                       double *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* reference: np.sum(img_data / norm_vect, axis=-1) of calculate_pixel_intensity_percentile
 * (pixel_cluster_utils.py:96-101): per pixel the float32 sum over channels of img/norm, added in numpy's
 * order for a contiguous float32 axis (c <= 128).  img_dev [n, c] float32, out_dev [n] float32. */
int pxsom_scaled_rowsum_f32(const float *img_dev, int64_t n, int c, int64_t ldx, const float *norm_dev,
                            float *out_dev, void *stream);
/* The same sum in binary64: what numpy computes when the image is not float32 (uint16 / int16 exports: the
 * division by the binary64 channel percentiles promotes to float64) -- same summation order. */
int pxsom_scaled_rowsum_f64(const double *img_dev, int64_t n, int c, int64_t ldx, const double *norm_dev,
                            double *out_dev, void *stream);

/* ---- pixel cluster mask: the relabel + scatter of generate_pixel_cluster_mask ------------------------
 * reference: utils/data_utils.py:532-553 -- coordinates = row_index * W + column_index;
 * cluster_labels = [id_mapping[label] for label in ...]; img.ravel()[coordinates] = cluster_labels on an
 * int16 image of zeros.  lut_dev [lut_size] int32 holds id_mapping densely (PXSOM_LUT_UNMAPPED where the
 * mapping has no entry).  mask_dev [h, w] int16 is overwritten (0 where the table has no pixel; ids are
 * narrowed to int16 the way numpy's assignment does).  A pixel listed more than once keeps the id of its
 * LAST row, like the sequential numpy assignment.  status_dev [1] int32 comes back 0, or with
 * PXSOM_MASK_BAD_LABEL (a label outside the LUT or unmapped: the reference raises KeyError) and / or
 * PXSOM_MASK_BAD_PIXEL (a coordinate outside the image: IndexError) set; the mask is then unspecified.
 * A NEGATIVE flat position row_index * W + column_index is PXSOM_MASK_BAD_PIXEL here, where numpy's fancy assignment
 * would wrap it to the end of the image: the reference's tables never hold one, and the kernel does not imitate the wrap.
 * workspace: pxsom_cluster_mask_workspace_bytes(h, w) (one int64 per pixel: index of the winning row). */
#define PXSOM_LUT_UNMAPPED (-2147483647 - 1)
#define PXSOM_MASK_BAD_LABEL 1
#define PXSOM_MASK_BAD_PIXEL 2
size_t pxsom_cluster_mask_workspace_bytes(int h, int w);
int pxsom_cluster_mask(const int64_t *row_index_dev, const int64_t *column_index_dev, const int64_t *labels_dev,
                       int64_t n, const int32_t *lut_dev, int64_t lut_size, int h, int w, int16_t *mask_dev,
                       int32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- SOM cluster -> meta cluster: the per-pixel half of pixel_consensus_cluster -----------------------------
 * reference: cluster_helpers.py:669-682 (PixieConsensusCluster.assign_consensus_labels: Series.map through the
 * K-row mapping), applied per FOV table at pixel_meta_clustering.py:17-50.  out_dev[i] = lut_dev[labels_dev[i]] for
 * labels inside [0, lut_size), `fill` otherwise (what the map turns into NaN); in place allowed. */
int pxsom_relabel(const int32_t *labels_dev, int64_t n, const int32_t *lut_dev, int lut_size, int32_t fill,
                  int32_t *out_dev, void *stream);

/* ---- other distances: FlowSOM's `distf` codes ------------------------------------------------------------
 * pyFlowSOM's som / map_data_to_nodes take distf = 1 (Manhattan), 2 (Euclidean), 3 (Chebyshev), 4 (cosine).  The
 * formulas are RECALLED from FlowSOM's som.c (parity with pyFlowSOM unpinned, as for Euclidean).  All arithmetic binary64,
 * channels j = 0..c-1 ascending, one rounding per operation:
 *   1  d = 0; d += fabs(x_j - w_j)
 *   3  d = 0; t = fabs(x_j - w_j); if (t > d) d = t          (a NaN channel never replaces d: an all-NaN row has d = 0)
 *   4  nom += x_j*w_j; d1 += x_j*x_j; d2 += w_j*w_j; d = (-nom / (sqrt(d1) * sqrt(d2))) + 1   (zero row / node: NaN)
 * pxsom_assign_metric: first strict minimum below DBL_MAX over nodes in ascending order, labels as pxsom_assign (0 when no
 * distance compared smaller, NaN included); dist_dev (optional) gets that distance, DBL_MAX for label 0.  Every (row, node)
 * pair is evaluated in binary64 (no screen).  Row views are not taken (PXSOM_ERR_UNSUPPORTED under one).
 * pxsom_train_online_metric: the loop of pxsom_train_online_ex with the BMU distance replaced (nearest starts at node 0,
 * `d[k] < d[nearest]`).  Metric 2 forwards to pxsom_assign_ex / pxsom_train_online_ex; an unknown metric is
 * PXSOM_ERR_INVALID_ARG before any HIP call.  Workspace: pxsom_assign_metric_workspace_bytes (for metric 2 it is
 * pxsom_assign_workspace_bytes); pxsom_assign_last_exact_rows reads n back on a metric 1 / 3 / 4 workspace. */
#define PXSOM_METRIC_MANHATTAN 1
#define PXSOM_METRIC_EUCLIDEAN 2
#define PXSOM_METRIC_CHEBYSHEV 3
#define PXSOM_METRIC_COSINE 4
size_t pxsom_assign_metric_workspace_bytes(int64_t n, int c, int k, int metric);
int pxsom_assign_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev,
                        int k, int32_t *labels_dev, double *dist_dev, void *workspace_dev,
                        size_t workspace_bytes, int metric, void *stream);
int pxsom_train_online_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, double *w_dev,
                              int xdim, int ydim, int rlen, double a0, double a1, double r0, double r1,
                              const int64_t *order_dev, int metric, int flags, void *stream);

/* ---- batch training and one-pass labelling under distf 1, 3, 4 (K6m; symbols added under ABI 9, none changed) ----------
 * pxsom_assign_sums_metric: labels AND batch statistics of a set of rows in one pass over x_dev, metric 1, 3 or 4.
 *   rows       row i takes part iff e0 <= i % phases < e1 (the row dealing of pxsom_batch_train_sched; 1, 0, 1: every row)
 *   labels_dev [n] int32 or NULL: pxsom_assign_metric's label of every row that takes part, bit for bit (same helpers, same
 *              order, first strict minimum below DBL_MAX, 0 when nothing compared smaller); the other entries are left untouched
 *   stats_dev  [k*c sums | k counts] binary64, ADDED into: a row with label b >= 1 adds its values -- binary64 rows rounded to
 *              sum_quantum as under "Reproducible statistics" above, binary32 / binary16 rows as they are -- to sums[b-1][:]
 *              and 1 to counts[b-1]; label-0 rows add nothing; a non-finite value of a labelled row (Chebyshev skips NaN
 *              channels in the search) is added in binary64 like any other.  With a quantum from pxsom_exact_sum_quantum every
 *              addition is exact: the same bits for any grid, any order, every run.  With quantum 0 the additions are binary64
 *              in unspecified order.  Counts are always exact.
 * One launch behind the codebook preparation of pxsom_assign_metric (the same workspace layout;
 * pxsom_metric_step_workspace_bytes(c, k, metric), 0 for an unknown metric, metric 2 or a shape outside the limits): a grid
 * sized to the CUs loops over the rows, each workgroup sums into a table [k*c | k] in LDS and adds its non-zero entries to
 * stats_dev at the end.  LIMIT: a table that does not fit 160 KiB of LDS beside the staging of rows wider than 32 channels
 * (k * (c + 1) * 8 bytes; 400 x 40 fits, 1024 x 64 does not) is not built -- every row is then added to stats_dev directly,
 * as pxsom_cluster_sums does for such tables; same results, but SLOWER than pxsom_assign_metric + pxsom_cluster_sums (1.12 -
 * 1.20 x at 65 536 x 64, K = 1024).  TWO LAUNCHES inside the entry -- pxsom_assign_metric, then the sums kernels with the
 * quantum -- replace the one pass where it measured slower than that pair (cosine on rows wider than 32 channels; every metric past the
 * LIMIT) whenever the
 * pair can run: the window is every row and labels_dev is given (its labels are then the pair's), or, in
 * pxsom_batch_train_sched_metric, the step is one phase or every row (its labels go to the workspace).  Same results.
 * Checks in the order and words of pxsom_assign_metric: unknown metric PXSOM_ERR_INVALID_ARG before any HIP call; metric 2
 * PXSOM_ERR_UNSUPPORTED (pxsom_assign_sums / pxsom_batch_accumulate are the Euclidean entries); then n, c, k, ldx, dtype, null
 * pointers, the window (0 <= e0 < e1 <= phases), sum_quantum (0 or a power of two), the workspace, an active row view.  n == 0
 * or no row in the window: PXSOM_OK, nothing touched.  Statement of record: tests/metric_reference.py (labels) with
 * orc_cluster_sums / oracle_binding.quantize (statistics); parity with pyFlowSOM unpinned.
 * pxsom_batch_train_sched_metric: pxsom_batch_train_sched_from under metric 1, 3 or 4.  State conventions unchanged
 * (wbuf[g % 2] holds W_g; step g leaves its statistics in ring[g % 3] and clears ring[(g+1) % 3]; the g_begin == 0 call
 * clears ring[0] and takes w0_dev); per step the pending update of step g - 1 (the launch of pxsom_batch_update), then
 * preparation + pxsom_assign_sums_metric's launch on the step's window [edges[g], edges[g+1]) -- rows are read where they lie.
 * Schedule position, threshold and alpha as pxsom_batch_train_sched; flags are ignored (they choose among Euclidean routes).
 * Workspace: pxsom_batch_train_sched_metric_workspace_bytes (the prepared codebook and the labels of the largest step).
 * comm must be NULL (PXSOM_ERR_UNSUPPORTED otherwise): a multi-rank run makes one call per step and all-reduces ring[g % 3]
 * in between.  n < 2^31.  pxsom_batch_train_sched_finish serves every metric. */
size_t pxsom_metric_step_workspace_bytes(int c, int k, int metric);
int pxsom_assign_sums_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w_dev, int k,
                             int phases, int e0, int e1, int32_t *labels_dev, double *stats_dev, double sum_quantum,
                             void *workspace_dev, size_t workspace_bytes, int metric, void *stream);
size_t pxsom_batch_train_sched_metric_workspace_bytes(int64_t n, int c, int k, int dtype, int phases,
                                                      const int32_t *edges_host, int steps_per_pass, int metric);
int pxsom_batch_train_sched_metric(const void *x_dev, int64_t n, int c, int64_t ldx, int dtype, const double *w0_dev,
                                   double *wbuf_dev, double *stats_ring_dev, int xdim, int ydim, int phases,
                                   const int32_t *edges_host, int steps_per_pass, int g_begin, int g_end, int num_passes,
                                   double a0, double a1, double r0, double r1, double sum_quantum, void *workspace_dev,
                                   size_t workspace_bytes, int flags, pxsom_comm *comm, int metric, void *stream);

/* ---- the launch an online training call would make (host arithmetic, no GPU call; works without a device) --------
 * pxsom_train_online[_ex] (metric 2) and pxsom_train_online_metric (1, 3, 4) pick one of their kernel forms from
 * k = xdim * ydim and c alone; this query runs the same planning function the launch runs and fills out[0 .. 6]:
 *   [0] family     PXSOM_ONLINE_LANES_PER_NODE (Euclidean, small maps) or PXSOM_ONLINE_THREAD_PER_NODE
 *   [1] CH, channels per lane            | CMAX, the register width of a node (0: the codebook is not in registers)
 *   [2] L, lanes per node                | MAXT, the kernel's thread bound
 *   [3] in_place   CMAX 0 only: the codebook does not fit the LDS beside the row ring and is trained where it lies
 *   [4] threads of the one workgroup   [5] chunk: steps whose rows are gathered ahead together   [6] LDS bytes
 * Returns PXSOM_OK, or the status and pxsom_last_error() message the training call gives for the shape (c or the grid
 * past PXSOM_MAX_CHANNELS / PXSOM_MAX_NODES, a dtype or metric it does not know, no LDS for the row ring); the record is
 * then all -1.  The dtype is validated and does not change the form.  A symbol added under ABI 9, none changed.
 * pxsom_train_online_routes: the same for `count` shapes at once -- shapes [count][5] = (c, xdim, ydim, dtype, metric),
 * out [count][1 + 7] = (status, record); host pointers.  Returns PXSOM_OK unless the table itself is bad. */
#define PXSOM_ONLINE_LANES_PER_NODE 0
#define PXSOM_ONLINE_THREAD_PER_NODE 1
#define PXSOM_ONLINE_ROUTE_FIELDS 7
int pxsom_train_online_route(int c, int xdim, int ydim, int dtype, int metric, int32_t *out);
int pxsom_train_online_routes(int64_t count, const int32_t *shapes, int32_t *out);

/* ---- cell cluster masks: border erosion + label lookup over a segmentation image (K10) ----------------------
 * reference: ark/utils/data_utils.py erode_mask (skimage.segmentation.find_boundaries, then np.where(edges == 0, seg, 0)),
 * relabel_segmentation / label_cells_by_cluster / map_segmentation_labels.  One stream-ordered pass over seg_dev [h, w]
 * (row stride ld elements, ld >= w) of seg_dtype (PXSOM_SEG_U8 .. PXSOM_SEG_I64); per pixel:
 *   1. erosion (erode_mode != PXSOM_SEG_ERODE_NONE): the pixel is a boundary pixel when an in-image neighbour holds a
 *      different label (4-neighbourhood for connectivity 1, 8-neighbourhood for connectivity >= 2; a neighbour outside the
 *      image counts as equal: scipy's reflect border of dilation != erosion).  PXSOM_SEG_ERODE_INNER also requires
 *      label != background (compared as int64).  Labels are compared in seg_dtype.  A boundary pixel becomes 0.
 *   2. lookup (n_keys >= 0): key = (int32)label (two's-complement wrap, numpy's astype(np.int32)); the pixel gets
 *      values_dev[i] where keys_dev[i] == key, else `unassigned`.  n_keys < 0: no lookup, the (eroded) label itself is stored.
 *   3. store in out_dtype (PXSOM_SEG_I16 / PXSOM_SEG_I32 / PXSOM_SEG_F64, or seg_dtype itself): integer stores wrap as
 *      numpy's astype does; out_dev [h, w] with row stride ldo >= w.
 * values_dev is double [n_keys] for PXSOM_SEG_F64 output, int32 [n_keys] otherwise; `unassigned` is converted the same
 * way (it must be an int32 value for integer outputs).  keys_dev [n_keys] int32 MUST be sorted ascending without
 * duplicates, with key_min = keys[0] and key_max = keys[n_keys - 1]: the library does not check this (the Python wrapper
 * does).  Table route: a dense index LUT over [key_min, key_max] built in the workspace when
 * pxsom_segmask_workspace_bytes(n_keys, key_min, key_max) > 0 (and PXSOM_SEGMASK_FORCE_SEARCH is not set), else a binary
 * search over keys_dev; both give identical results.  Bad dtype / mode / connectivity / sizes / strides / workspace:
 * PXSOM_ERR_INVALID_ARG before any HIP call.  In-place (out_dev == seg_dev) is allowed when out and seg share dtype and
 * stride and there is no erosion. */
#define PXSOM_SEG_U8 0
#define PXSOM_SEG_I16 1
#define PXSOM_SEG_U16 2
#define PXSOM_SEG_I32 3
#define PXSOM_SEG_U32 4
#define PXSOM_SEG_I64 5
#define PXSOM_SEG_F64 6      /* output only */
#define PXSOM_SEG_F32 7      /* pxsom_gaussian_blur_plane / pxsom_zero_by_seg images only */
#define PXSOM_SEG_ERODE_NONE 0
#define PXSOM_SEG_ERODE_THICK 1
#define PXSOM_SEG_ERODE_INNER 2
#define PXSOM_SEGMASK_FORCE_SEARCH 1
size_t pxsom_segmask_workspace_bytes(int64_t n_keys, int32_t key_min, int32_t key_max);
int pxsom_segmask(const void *seg_dev, int seg_dtype, int h, int w, int64_t ld, int erode_mode, int connectivity,
                  int64_t background, const int32_t *keys_dev, const void *values_dev, int64_t n_keys, int32_t key_min,
                  int32_t key_max, double unassigned, void *out_dev, int out_dtype, int64_t ldo, void *workspace_dev,
                  size_t workspace_bytes, int flags, void *stream);

/* ---- channel edits: smooth_channels and filter_with_nuclear_mask (K11) ----------------------------------------------
 * The PXSOM_SEG_* codes name the dtypes of both entries.  Which entry takes which code:
 *   pxsom_segmask              seg: U8 .. I64          out: I16, I32, F64 or seg's own
 *   pxsom_gaussian_blur_plane  plane: U8, I16, U16, I32, F32
 *   pxsom_zero_by_seg          img: U8, I16, U16, I32, F32    seg: U8 .. I64
 *
 * pxsom_gaussian_blur_plane: scipy.ndimage.gaussian_filter(plane, sigma) on ONE contiguous [h, w] plane in the plane's
 * own dtype (reference: pixel_cluster_utils.smooth_channels).  Axis 0, then axis 1; each pass computes in binary64 in
 * scipy's symmetric-kernel order without FMA contraction (as pxsom_gaussian_blur_hwc) and stores its result in the
 * plane's dtype, as scipy stores each pass in the output array: float32 rounds to nearest, integers truncate toward zero
 * (a C cast).  weights_host / radius as for pxsom_gaussian_blur_hwc; radius > 64 (sigma >= 16.125 at truncate 4) is
 * PXSOM_ERR_UNSUPPORTED.  out_dev may equal in_dev; tmp_dev is a same-size plane of the same dtype, distinct from both.
 * (Skipping an axis for sigma <= 1e-15 is the caller's: this entry always runs both passes.)
 *
 * pxsom_zero_by_seg: img[i] = 0 where seg[i] > 0 (exclude = 1) or seg[i] == 0 (exclude = 0), i < n; img and seg hold n
 * elements each, contiguous (filter_with_nuclear_mask's img[seg > 0] = 0 / img[seg == 0] = 0).
 * Bad pointers, sizes, dtype codes or flags: PXSOM_ERR_INVALID_ARG before any HIP call, for both entries. */
int pxsom_gaussian_blur_plane(const void *in_dev, void *out_dev, void *tmp_dev, int h, int w, int dtype,
                              const double *weights_host, int radius, void *stream);
int pxsom_zero_by_seg(void *img_dev, int img_dtype, const void *seg_dev, int seg_dtype, int64_t n, int exclude,
                      void *stream);

/* ---- cell table: per-cell counts, centroid sums and channel values of a segmented image (K12) -----------------------
 * reference: ark/segmentation/marker_quantification.py compute_marker_counts under fast_extraction (regionprops label,
 * coords, centroid) with ark/segmentation/signal_extraction.py and segmentation_utils.find_nuclear_label_id.
 * seg_dev [h, w] (row stride ld >= w) of seg_dtype PXSOM_SEG_U8 .. PXSOM_SEG_I64; img_dev a contiguous interleaved
 * [h, w, c] image of img_dtype PXSOM_SEG_U8, _I16, _U16, _I32, _F32 or _F64.  keys_dev [n_keys] int32, sorted ascending
 * without duplicates and without 0, key_min = keys[0], key_max = keys[n_keys - 1] (not checked here: the Python wrapper
 * does); cell i is the set of pixels whose label, cast to int32, equals keys[i] (label 0 is background).  Outputs per cell i:
 *   count_dev[i] (int64)          pixels of the cell
 *   sums_dev[2i], [2i + 1]        sum of row and of column indices (int64, exact; centroid = sum / count in binary64)
 *   bbox_dev[4i .. 4i + 3]        row min, row max, column min, column max (int32; INT32_MAX, -1 for an absent key)
 *   values_dev[i * c + j]         channel j as binary64, by mode:
 *     PXSOM_CELLQUANT_TOTAL     np.sum(img[rows, cols], axis=0) in the image's dtype: integers exactly, float32 / float64
 *                               in numpy's order -- for c >= 2 the pixels one after another in raster order, for c == 1
 *                               numpy's pairwise sum over buffers of 8192 (bit-equal)
 *     PXSOM_CELLQUANT_POSITIVE  count of img > threshold (compared in binary64: for a float32 image pass the threshold
 *                               rounded to float32, as numpy compares)
 *     PXSOM_CELLQUANT_CENTER    w . img[rows, cols] in binary64, w = 1 - d / (max d + 1), d the Chebyshev distance to the
 *                               centroid; summed in raster order (the reference's BLAS order is not reproduced)
 * nuc_dev (optional, [h, w], row stride ldn, nuc_dtype, keys nuc_keys_dev as for keys_dev): nuc_out_dev[i] = index in
 * nuc_keys of the nucleus with the most pixels in cell i, the smaller index on a tie, -1 when none.  The overlap table
 * holds nuc_capacity distinct nuclei per cell (1 .. 128, 0 = 128); a cell meeting more takes a slower exact route.
 * Workspace: pxsom_cellquant_workspace_bytes with the same sizes, table ranges and flags (n_nuc_keys < 0: no nuclear image);
 * key tables take a dense LUT by the K10 rule unless PXSOM_CELLQUANT_FORCE_SEARCH; both routes give identical results.
 * Bad pointers, dtype codes, sizes, modes, flags or workspace: PXSOM_ERR_INVALID_ARG before any HIP call. */
#define PXSOM_CELLQUANT_TOTAL 0
#define PXSOM_CELLQUANT_POSITIVE 1
#define PXSOM_CELLQUANT_CENTER 2
#define PXSOM_CELLQUANT_FORCE_SEARCH 1
size_t pxsom_cellquant_workspace_bytes(int h, int w, int c, int img_dtype, int mode, int64_t n_keys, int32_t key_min,
                                       int32_t key_max, int64_t n_nuc_keys, int32_t nuc_key_min, int32_t nuc_key_max,
                                       int flags);
int pxsom_cellquant(const void *seg_dev, int seg_dtype, int64_t ld, const void *nuc_dev, int nuc_dtype, int64_t ldn,
                    int h, int w, const void *img_dev, int img_dtype, int c, const int32_t *keys_dev, int64_t n_keys,
                    int32_t key_min, int32_t key_max, const int32_t *nuc_keys_dev, int64_t n_nuc_keys,
                    int32_t nuc_key_min, int32_t nuc_key_max, int mode, double threshold, int nuc_capacity,
                    int64_t *count_dev, int64_t *sums_dev, int32_t *bbox_dev, double *values_dev, int32_t *nuc_out_dev,
                    void *workspace_dev, size_t workspace_bytes, int flags, void *stream);

/* ---- cell morphology: the raw integers of the regionprops columns of generate_cell_table (K17) ------------------------
 * reference: ark/segmentation/marker_quantification.py get_single_compartment_props (skimage regionprops area,
 * eccentricity, axis lengths, perimeter, convex_area) and ark/segmentation/regionprops_extraction.py (centroid_dif,
 * num_concavities), by their documented algorithms in integer geometry; parity with skimage itself is not pinned.
 * Symbols added under ABI 9, none changed.  seg_dev, keys_dev and the cells: as for pxsom_cellquant; a label past int32
 * is background.
 *
 * pxsom_region_shape: per cell i, shape_dev[6i .. 6i + 5] (int64, every entry written) =
 *   sum r^2, sum c^2, sum r c over the cell's pixels (image coordinates), then the number of border pixels in each weight
 *   class of skimage.measure.perimeter(neighbourhood=4): a border pixel has a 4-neighbour that is not the cell or lies
 *   outside the image, its code is 1 + 2 * (4-neighbours that are border pixels of the cell) + 10 * (diagonal ones);
 *   codes 5, 7, 15, 17, 25, 27 weigh 1, codes 21, 33 weigh sqrt 2, codes 13, 23 weigh (1 + sqrt 2) / 2.
 * count_dev, sums_dev, bbox_dev: all NULL, or all given and then written as pxsom_cellquant writes them.  Integer atomics
 * only: the same input gives the same bits.  Workspace: pxsom_region_shape_workspace_bytes (the dense LUT of the K10 rule,
 * 0 under PXSOM_REGION_FORCE_SEARCH; both routes give identical results).
 *
 * pxsom_region_hull: per cell i whose bounding box (bbox_dev, count_dev as pxsom_cellquant or pxsom_region_shape wrote
 * them) is at most 64 x 64, hull_dev[4i .. 4i + 3] (int64) =
 *   the pixels of the convex image -- centres inside or ON the hull of the diamond points (r +- 1/2, c), (r, c +- 1/2) of
 *   the cell's pixels, decided in doubled integer coordinates -- their row sum and column sum, and the number of
 *   concavities: 4-connected components of (convex image minus cell) with area a and perimeter p (the rule above on the
 *   component alone, p = (n1 + n2 * sqrt 2) + n3 * ((1 + sqrt 2) / 2) in binary64 without contraction) for which
 *   (a > small_concavity_minimum and p * p / a < max_compactness) or a > large_concavity_minimum.
 * left_out_dev[i] (int32) = 1 for a cell with a larger box: its hull_dev entries are 0 and the caller computes them
 * elsewhere.  An absent key (count 0) gives zeros.  A box outside the image is treated as an absent key, never read.
 * The box is expected tight; in a box that is not, the pixels of the key inside it are the cell (none: zeros).
 * Bad dtype codes, sizes, flags, NaN thresholds, pointers or workspace: PXSOM_ERR_INVALID_ARG before any HIP call. */
#define PXSOM_REGION_FORCE_SEARCH 1
size_t pxsom_region_shape_workspace_bytes(int64_t n_keys, int32_t key_min, int32_t key_max, int flags);
int pxsom_region_shape(const void *seg_dev, int seg_dtype, int64_t ld, int h, int w, const int32_t *keys_dev,
                       int64_t n_keys, int32_t key_min, int32_t key_max, int64_t *shape_dev, int64_t *count_dev,
                       int64_t *sums_dev, int32_t *bbox_dev, void *workspace_dev, size_t workspace_bytes, int flags,
                       void *stream);
int pxsom_region_hull(const void *seg_dev, int seg_dtype, int64_t ld, int h, int w, const int32_t *keys_dev,
                      int64_t n_keys, const int64_t *count_dev, const int32_t *bbox_dev, double small_concavity_minimum,
                      double max_compactness, double large_concavity_minimum, int64_t *hull_dev, int32_t *left_out_dev,
                      void *stream);

/* ---- neighbourhood matrix: per-cell neighbour counts by phenotype, from the centroids (K13) -------------------------
 * reference: ark/analysis/spatial_analysis_utils.py calc_dist_matrix (cdist(...).astype(float32), one N x N matrix per
 * FOV) and compute_neighbor_counts (dist < distlim, dist == 0 removed unless self_neighbor, one-hot dot).  One
 * stream-ordered launch covers the cohort and the N x N matrix is never built.
 *   xy_dev   [n, 2] binary64 centroids, 16-byte aligned
 *   type_dev [n] int32 in [0, n_types); WITHIN each FOV the rows MUST be sorted by type, ascending (not checked here: the
 *            Python wrapper sorts and restores the caller's order)
 *   seg_dev  [n_fovs + 1] int64 offsets, non-decreasing, seg[0] = 0, seg[n_fovs] = n: FOV f is rows seg[f] .. seg[f + 1];
 *            an empty FOV is allowed
 * For cells i and j of one FOV (j = i included): s = fl(fl(dx * dx) + fl(dy * dy)) in binary64 without contraction; j
 * is a neighbour of i when s < s_lim and (self_neighbor or s > s_zero).  counts_dev[i * n_types + type[j]] (int32) is
 * the number of such j; every entry of counts_dev [n, n_types] is written (the caller need not clear it).  With s_lim the
 * smallest double whose float32(sqrt(s)) >= distlim and s_zero the largest whose float32(sqrt(s)) == 0 the test is
 * float32(sqrt(s)) < distlim and != 0 exactly: sqrt and the cast are correctly rounded and monotone.
 * No workspace.  Offsets are clamped to [0, n] and a type that is out of range or out of order is not stored, so bad
 * device-side input gives wrong rows, never a write outside counts_dev.  Bad sizes, flag, NaN thresholds or null /
 * misaligned pointers: PXSOM_ERR_INVALID_ARG before any HIP call. */
int pxsom_neighbor_counts(const double *xy_dev, const int32_t *type_dev, const int64_t *seg_dev, int64_t n_fovs,
                          int64_t n, int n_types, double s_lim, double s_zero, int self_neighbor, int32_t *counts_dev,
                          void *stream);

/* ---- close-pair counts between cell sets, per FOV, from the centroids (K20) -------------------------------------------
 * reference: ark/analysis/spatial_analysis_utils.py compute_close_cell_num (the float32 distance matrix binarised with
 * < dist_lim and > 0, subset to the rows positive for marker or phenotype j and the columns positive for k, summed) and
 * the target / reference interaction totals of ark/analysis/neighborhood_analysis.py compute_mixing_score.  One
 * stream-ordered launch covers the cohort; neither the N x N matrix nor an N x sets table is built.  Symbol added under
 * ABI 9, none changed.
 *   xy_dev        [n, 2] binary64 centroids, 16-byte aligned; n < 2^31
 *   member_q_dev  [n] uint64: bit s says that the cell, as the first of a pair, is in row set s
 *   member_c_dev  [n] uint64: bit t says that the cell, as the second of a pair, is in column set t (the two pointers
 *                 may be equal).  Bits at or above n_sets_q / n_sets_c are ignored.
 *   seg_dev       [n_fovs + 1] int64 offsets as for pxsom_neighbor_counts (clamped to [0, n] on the device; an empty FOV
 *                 is allowed); the rows need no order inside a FOV
 *   n_sets_q, n_sets_c   1 .. 64
 *   s_lim, s_zero, self_neighbor   the pair test of pxsom_neighbor_counts: cells a and b of one FOV (b = a included)
 *                 count when s = fl(fl(dx * dx) + fl(dy * dy)) < s_lim and (self_neighbor or s > s_zero)
 * out_dev [n_fovs, n_sets_q, n_sets_c] int64: out[f, s, t] = the number of ordered pairs (a, b) of FOV f that count with
 * bit s of member_q[a] and bit t of member_c[b] set.  The entry clears out_dev itself (one memset on the stream before
 * the launch): the caller need not.  Integer additions only: the result does not depend on the grid and is the same
 * on every run.  No workspace.  Every index into out_dev is built from f < n_fovs, s < n_sets_q, t < n_sets_c, so bad
 * device-side input gives wrong counts, never a store outside out_dev.  Bad sizes, set counts, flag, NaN thresholds or
 * null / misaligned pointers: PXSOM_ERR_INVALID_ARG before any HIP call. */
int pxsom_close_pair_counts(const double *xy_dev, const uint64_t *member_q_dev, const uint64_t *member_c_dev,
                            const int64_t *seg_dev, int64_t n_fovs, int64_t n, int n_sets_q, int n_sets_c, double s_lim,
                            double s_zero, int self_neighbor, int64_t *out_dev, void *stream);

/* ---- cell-distance analysis: per cell, the mean distance to its k nearest cells of every phenotype (K14) -------------
 * reference: ark/analysis/cell_neighborhood_stats.py calculate_mean_distance_to_cell_type over calc_dist_matrix's float32
 * matrix (the columns of one phenotype, where(dist > 0), np.sort per row, [:, :k].mean(axis=1)).  One stream-ordered
 * launch covers the cohort and the N x N matrix is never built.
 *   xy_dev, type_dev, seg_dev, n_fovs, n, n_types: as for pxsom_neighbor_counts (rows of a FOV sorted by type)
 *   k        1 .. 32 (the device route's limit: the k smallest live in registers)
 *   s_zero   the largest double whose float32(sqrt(s)) == 0 (som_device.neighbor_thresholds)
 * For cell i and type t take every j of i's FOV with type[j] == t (j = i included), s = fl(fl(dx * dx) + fl(dy * dy)) in
 * binary64 without contraction, and keep those with s > s_zero.  Fewer than k kept: means_dev[i * n_types + t] = NaN.
 * Otherwise the k smallest s, ascending, each mapped to float32(sqrt(s)) (sqrt correctly rounded in binary64, then
 * rounded to float32), are summed in float32 in the order numpy's pairwise row reduction uses -- a fold from 0 for
 * k < 8; else eight strided accumulators over the first k - k % 8 terms, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
 * remaining terms in order -- and divided by float32(k).  Every entry of means_dev [n, n_types] (float32) is written
 * (the caller need not clear it); a row no FOV holds is NaN.
 * No workspace.  Offsets are clamped to [0, n] and a type that is out of range or out of order is not stored, so bad
 * device-side input gives wrong rows, never a write outside means_dev.  Bad sizes, k outside 1 .. 32, a NaN s_zero or
 * null / misaligned pointers: PXSOM_ERR_INVALID_ARG before any HIP call. */
int pxsom_nearest_type_means(const double *xy_dev, const int32_t *type_dev, const int64_t *seg_dev, int64_t n_fovs,
                             int64_t n, int n_types, int k, double s_zero, float *means_dev, void *stream);

/* ---- silhouette coefficients of the rows of a matrix under several labelings at once (K15) ---------------------------
 * reference: sklearn.metrics.silhouette_samples / silhouette_score (Euclidean), which
 * ark/analysis/spatial_analysis_utils.py compute_kmeans_silhouette calls once per k.  Stream-ordered launches cover every
 * labeling and the N x N matrix is never built.
 *   x_dev        [n, d] binary64, row-major; 1 <= d <= 64 and 2 <= n < 2^31 (the device route's limits)
 *   labels_dev   [n_labelings, n] int32, values in [0, k)
 *   order_dev    [n_labelings, n] int32: for every labeling a permutation of 0 .. n - 1 that lists the rows of cluster 0,
 *                then those of cluster 1, ... (a stable argsort of the labels)
 *   k            2 .. 32 (the device route's limit); a labeling may leave clusters empty
 *   counts_dev   [n_labelings, k] int32, written: the cluster sizes
 *   sums_dev     [n_labelings, n, k] binary64, written:
 *                  S[m, i, c] = sum over j with labels[m, j] == c of sqrt(sum_t (x[i, t] - x[j, t])^2)
 *                every difference rounded once, every square added by one fused multiply-add in the order of t, the square
 *                root correctly rounded, the distances of a cluster added one by one in the order `order` lists them:
 *                no floating-point atomic anywhere, the same input gives the same bits.  Equal rows are at distance 0.
 *   samples_dev  [n_labelings, n] binary64, written: with c_i = labels[m, i],
 *                  a = S[i, c_i] / (n_{c_i} - 1), b = min over c != c_i with n_c > 0 of S[i, c] / n_c,
 *                  s = (b - a) / max(a, b), and s = 0 when n_{c_i} == 1 or the quotient is NaN (silhouette_samples' rules)
 *   scores_dev   [n_labelings] binary64, written: the mean of samples[m, :], reduced in a fixed order
 * Every entry of the four outputs is written (the caller need not clear them).  A label outside [0, k) is counted nowhere
 * and used as no index (its sample is NaN), run boundaries are clamped to [0, n] and an entry of order_dev outside [0, n)
 * stands for a row of zeros: bad device-side input gives wrong rows, never an access outside the arrays.  d, k, n or
 * n_labelings outside their limits, or a null pointer: PXSOM_ERR_INVALID_ARG before any HIP call. */
int pxsom_silhouette(const double *x_dev, int64_t n, int d, const int32_t *labels_dev, const int32_t *order_dev,
                     int n_labelings, int k, int32_t *counts_dev, double *sums_dev, double *samples_dev,
                     double *scores_dev, void *stream);

/* ---- Lloyd's k-means of the rows of a matrix for several problems at once (K19) ---------------------------------------
 * reference: sklearn.cluster.KMeans (Lloyd) as ark/analysis/spatial_analysis_utils.py fits it: once per k of a sweep, or
 * with ten restarts.  Every (k, restart) is one problem over the same rows; one iteration is one pass over the rows per
 * group of still-active problems (the grouping rule and its LDS bytes: csrc/pxsom_kmeans.hip).  Symbols added under ABI
 * 9, none changed.
 *   x_dev          [n, d] binary64, row-major, finite; 1 <= d <= 64, n < 2^31
 *   k_host         [n_problems] int32 on the host, every k in 1 .. 32 and <= n; 1 <= n_problems <= 4096
 *   centres_dev    [sum of k, d] binary64: problem p's rows follow those of problem p - 1.  In: the initial centres.
 *                  Out: the final ones.
 *   tol_host       [n_problems] binary64 >= 0, max_iter_host [n_problems] int32 >= 1, on the host
 *   labels_dev     [n_problems, n] int32, written: 0 .. k_p - 1
 *   inertia_host   [n_problems] binary64, iters_host [n_problems] int32, written on the host
 *   workgroups     0: twice the CU count; otherwise the grid of the assignment kernel (the results do not depend on it)
 * The rule: distance = sum_j (x_j - c_j)^2 with j ascending and every operation rounded on its own (no
 * fused multiply-add), first minimum wins; sums over fixed blocks of 256 rows folded in block order (no floating-point
 * atomic: the same input gives the same bits for any grid and any grouping); centre = sum / count; an empty cluster
 * moves to the row farthest from its own centre (several: ascending clusters take the farthest rows in order, ties to the
 * lower row); a problem stops when no label changed, or after one closing assignment pass when
 * sum ||new - old||^2 <= tol or max_iter is reached; inertia is the sum of the winning distances of the last
 * assignment.  n = 0 returns at once (iterations and inertia 0, nothing else written).  The call synchronises the stream
 * once per iteration to read three numbers per problem.  Workspace: pxsom_kmeans_workspace_bytes (0 for sizes the entry
 * does not take).  pxsom_kmeans_group_count: how many groups, so passes over the rows, the first iteration of these
 * problems takes (a host-side function; a negative status for bad sizes).  Sizes outside the limits, k > n, a bad tol
 * or max_iter, null pointers: PXSOM_ERR_INVALID_ARG before any HIP call; a short workspace: PXSOM_ERR_WORKSPACE. */
size_t pxsom_kmeans_workspace_bytes(int64_t n, int d, int n_problems, const int32_t *k_host);
int pxsom_kmeans_group_count(int d, int n_problems, const int32_t *k_host);
int pxsom_kmeans_lloyd(const double *x_dev, int64_t n, int d, int n_problems, const int32_t *k_host, double *centres_dev,
                       const double *tol_host, const int32_t *max_iter_host, int32_t *labels_dev, double *inertia_host,
                       int32_t *iters_host, void *workspace_dev, size_t workspace_bytes, int workgroups, void *stream);

/* ---- object masks: connected-component labelling and the passes around it (K16) --------------------------------------
 * reference: ark/segmentation/ez_seg/ez_object_segmentation.py _create_object_mask (filters.gaussian, a threshold,
 * morphology.remove_small_holes, measure.label(connectivity=2), regionprops_table area, map_array), which
 * create_object_masks and ark/utils/masking_utils.py wrap.  Symbols added under ABI 9, none changed.
 *
 * pxsom_label_components: skimage.measure.label / scipy.ndimage.label of a binary plane.
 *   fg_dev      [h, w] uint8, row stride ld >= w; a pixel is foreground when != 0 (invert = 0) or == 0 (invert = 1)
 *   connectivity 1 (4-neighbourhood) or 2 (8-neighbourhood)
 *   labels_dev  [h, w] int32, row stride ldo >= w, every pixel written: 0 for background; the component whose first
 *               pixel in raster order comes earliest is 1, the next 2, ...
 *   n_dev       [1] int32: the number of components
 *   areas_dev   [capacity] int32, every entry written: areas[0] the background pixels, areas[l] the pixels of label
 *               l < capacity, 0 past n.  A label >= capacity is counted nowhere: capacity = (h * w + 1) / 2 + 1 holds
 *               every image (a 4-connected checkerboard has the most components).
 * Integer arithmetic only (union-find with atomicMin on the parent index, int32 atomic adds for the areas): the same
 * input gives the same bits on every run.  Workspace: pxsom_label_components_workspace_bytes(h, w) (one int32 per pixel
 * and one count per 256 pixels; 0 for sizes the entry does not take).  Bad sizes, strides, connectivity, flag, capacity,
 * pointers or workspace: PXSOM_ERR_INVALID_ARG before any HIP call; h * w beyond int32: PXSOM_ERR_UNSUPPORTED.
 *
 * pxsom_components_select: one pass that rewrites a label image from its area table (labels_dev [h, w] int32, row
 * stride ldl; areas_dev [capacity]; a label >= capacity counts as area 0 and is never an index).
 *   PXSOM_SELECT_FILL  out_dev uint8 [h, w]: out = (fg != 0) | (label != 0 && area[label] < area_hi), labels being those of
 *                      the INVERTED plane under connectivity 1: morphology.remove_small_holes(fg, area_hi), strict <, no
 *                      special case for a hole that touches the border.  fg_dev [h, w] uint8, row stride ldf; area_lo unused.
 *   PXSOM_SELECT_KEEP  out_dev int32 [h, w]: out = label when area_lo <= area[label] <= area_hi, else 0; labels are not
 *                      renumbered (map_array(labels, all, all * keep)).  fg_dev unused; out_dev may be labels_dev.
 *
 * pxsom_gaussian_blur_plane_mode: pxsom_gaussian_blur_plane with scipy's border mode as an argument -- PXSOM_BLUR_REFLECT
 * (the K11 entry's, same bits) or PXSOM_BLUR_NEAREST (the index clamped to the line: skimage.filters.gaussian's default) --
 * and PXSOM_SEG_F64 planes beside U8, I16, U16, I32 and F32.  Same arithmetic order (correlate1d's symmetric branch in
 * binary64, no FMA contraction, each pass stored in the plane's dtype), same radius <= 64 limit (PXSOM_ERR_UNSUPPORTED).
 *
 * pxsom_binarize_plane: the uint8 foreground (1 / 0) of a contiguous [h, w] PXSOM_SEG_F32 or _F64 plane, out_dev row
 * stride ldo; compared in binary64 (float32 widens exactly):
 *   PXSOM_BIN_POSITIVE  v > 0
 *   PXSOM_BIN_LEVEL     !(v < level) && v > 0          (np.where(v < p, 0, v) > 0)
 *   PXSOM_BIN_LOCAL     v > local_dev[i]               (local_dev: a contiguous plane of the same dtype)
 * Bad arguments: PXSOM_ERR_INVALID_ARG before any HIP call, for all four entries. */
#define PXSOM_SELECT_FILL 0
#define PXSOM_SELECT_KEEP 1
#define PXSOM_BLUR_REFLECT 0
#define PXSOM_BLUR_NEAREST 1
#define PXSOM_BIN_POSITIVE 0
#define PXSOM_BIN_LEVEL 1
#define PXSOM_BIN_LOCAL 2
size_t pxsom_label_components_workspace_bytes(int h, int w);
int pxsom_label_components(const uint8_t *fg_dev, int h, int w, int64_t ld, int connectivity, int invert,
                           int32_t *labels_dev, int64_t ldo, int32_t *n_dev, int32_t *areas_dev, int64_t capacity,
                           void *workspace_dev, size_t workspace_bytes, void *stream);
int pxsom_components_select(int mode, const uint8_t *fg_dev, int64_t ldf, const int32_t *labels_dev, int64_t ldl,
                            const int32_t *areas_dev, int64_t capacity, int h, int w, int64_t area_lo, int64_t area_hi,
                            void *out_dev, int64_t ldo, void *stream);
int pxsom_gaussian_blur_plane_mode(const void *in_dev, void *out_dev, void *tmp_dev, int h, int w, int dtype,
                                   const double *weights_host, int radius, int border, void *stream);
int pxsom_binarize_plane(const void *plane_dev, int dtype, int h, int w, int mode, double level, const void *local_dev,
                         uint8_t *out_dev, int64_t ldo, void *stream);

/* ---- K22: the sign of the Meijering ridge filter on a binary plane ("projection" object masks) ------------------------
 * reference: _create_object_mask(object_shape_type="projection"): skimage.filters.meijering(mask, sigmas=range(1, 5),
 * black_ridges=False), of which only `> 0` is used.  skimage 0.19's filter is taken by its algorithm as restated below;
 * parity with skimage itself is unpinned.  A symbol added under ABI 9, none changed.
 *
 * pxsom_ridge_sign: out = OR over the scales s of (aux_s < 0), where with x = (fg != 0) as binary64
 *   g   = scipy.ndimage.gaussian_filter(x, sigma_s, mode="reflect", truncate=4): axis 0 first, then axis 1; each pass is
 *         correlate1d's symmetric branch (tmp = in * w[0]; for d = r .. 1: tmp += (in[-d] + in[+d]) * w[d]), the line
 *         extended by reflection however short it is
 *   g0  = np.gradient(g, axis=0), g1 = np.gradient(g, axis=1): unit spacing, edge_order 1 -- (f[i+1] - f[i-1]) / 2.0 inside,
 *         f[1] - f[0] and f[n-1] - f[n-2] at the two ends
 *   Hrr = s2 * np.gradient(g0, axis=0), Hrc = s2 * np.gradient(g0, axis=1), Hcc = s2 * np.gradient(g1, axis=1)
 *   d = Hrr - Hcc; r = sqrt(d*d + 4.0*(Hrc*Hrc)); t = Hrr + Hcc; e_hi = (t + r) / 2.0; e_lo = (t - r) / 2.0
 *   (big, small) = |e_lo| >= |e_hi| ? (e_lo, e_hi) : (e_hi, e_lo);  aux = big + alpha * small
 * in binary64 with one rounding per operation, no FMA contraction and a correctly rounded square root.
 *   fg_dev        [h, w] uint8, row stride ld >= w; a pixel counts as 1 when != 0
 *   weights_host  the 2 r + 1 weights of each scale's symmetric kernel, concatenated (host memory)
 *   radii_host    [n_scales] the radius r of each scale;  scales_host [n_scales] the factor s2 (sigma squared)
 *   out_dev       [h, w] uint8, row stride ldo >= w, every pixel written 1 or 0; must not overlap fg_dev
 * One launch, no workspace.  PXSOM_ERR_INVALID_ARG before any HIP call: a null pointer, h < 2 or w < 2 (np.gradient's
 * minimum), ld < w or ldo < w, n_scales outside 1 .. 8, a radius < 1, a factor that is not finite and > 0, a non-finite
 * alpha, out overlapping fg.  PXSOM_ERR_UNSUPPORTED: a radius > 16 (sigma = 4 is the reference's largest), h * w beyond
 * int32. */
int pxsom_ridge_sign(const uint8_t *fg_dev, int h, int w, int64_t ld, const double *weights_host, const int *radii_host,
                     const double *scales_host, int n_scales, double alpha, uint8_t *out_dev, int64_t ldo, void *stream);

/* ---- merging ez_seg object masks into the cell segmentation (K18) -----------------------------------------------------
 * reference: ark/segmentation/ez_seg/merge_masks.py merge_masks_single (skimage.morphology.label of both masks, one
 * full-image logical_and per candidate cell of every object).  Symbols added under ABI 9, none changed.
 *
 * pxsom_label_regions: skimage.measure.label(img, background=0, connectivity) of an integer label plane: a component is
 * a maximal set of pixels of ONE non-zero value joined under the 4- (connectivity 1) or 8-neighbourhood (2); touching
 * regions of different values stay apart, a negative value is a label like any other.
 *   seg_dev     [h, w] of a label dtype (PXSOM_SEG_U8 .. PXSOM_SEG_I64), row stride ld >= w elements
 *   labels_dev, n_dev, areas_dev, capacity, workspace: as for pxsom_label_components, with the same numbering (by first
 *               pixel in raster order) and the same stages after the tile and border passes; an image of one value gives
 *               the bits pxsom_label_components gives.  capacity = h * w + 1 holds every image (a two-value checkerboard
 *               under connectivity 1 makes every pixel a region).
 *   Workspace: pxsom_label_regions_workspace_bytes(h, w).  Same error rules as pxsom_label_components.
 *
 * pxsom_pair_overlaps: the pairs of labels two planes share.  a_dev, b_dev [h, w] int32, row strides lda, ldb; a pixel
 * belongs to the pair (a, b) when 1 <= a <= n_a and 1 <= b <= n_b -- any other value is counted nowhere and is never an
 * index.  pairs_dev [capacity, 3] int32 receives one row (a, b, pixels) per pair with pixels > 0, sorted by (a, b); rows
 * past the count are not written.  n_dev [2] int32: n_dev[1] = the RUNS of the image -- stretches of one pair inside a row
 * and inside an aligned group of 64 pixels of the flat raster order -- which bounds the number of distinct pairs;
 * n_dev[0] = the number of pairs, or -1 (and nothing written to pairs_dev) when the runs exceed capacity.
 *   Called with pairs_dev == NULL (capacity, workspace ignored) only the runs are counted: n_dev = {0, runs}; a caller
 *   sizes pairs_dev and the workspace from that and calls again.  The table behind the list has >= 2 * capacity slots and
 *   takes one insertion per run, and none when runs > capacity: it cannot overflow whatever the planes hold.  No dense
 *   n_a x n_b table, integer atomics only, a sort of the table: the same input gives the same bytes on every run.
 *   Workspace: pxsom_pair_overlaps_workspace_bytes(capacity) (0 for a capacity outside 1 .. 2^27).
 *
 * pxsom_merge_apply: one pass over both planes with two int32 tables of `table` entries (indexed by b):
 *   merged[p]    = winner[b[p]] != 0 ? winner[b[p]] : a[p]
 *   remaining[p] = removed[b[p]] != 0 ? 0 : b[p]
 * a b[p] outside [0, table) has no winner and is not removed.  All four planes [h, w] int32 with their own row strides.
 * Bad sizes, strides, counts, capacity, pointers or workspace: PXSOM_ERR_INVALID_ARG, the limit in the message, before
 * any HIP call, for all three entries. */
size_t pxsom_label_regions_workspace_bytes(int h, int w);
int pxsom_label_regions(const void *seg_dev, int dtype, int h, int w, int64_t ld, int connectivity, int32_t *labels_dev,
                        int64_t ldo, int32_t *n_dev, int32_t *areas_dev, int64_t capacity, void *workspace_dev,
                        size_t workspace_bytes, void *stream);
size_t pxsom_pair_overlaps_workspace_bytes(int64_t capacity);
int pxsom_pair_overlaps(const int32_t *a_dev, int64_t lda, const int32_t *b_dev, int64_t ldb, int h, int w, int32_t n_a,
                        int32_t n_b, int32_t *pairs_dev, int64_t capacity, int32_t *n_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream);
int pxsom_merge_apply(const int32_t *a_dev, int64_t lda, const int32_t *b_dev, int64_t ldb, int h, int w,
                      const int32_t *winner_dev, const int32_t *removed_dev, int64_t table, int32_t *merged_dev, int64_t ldm,
                      int32_t *remaining_dev, int64_t ldr, void *stream);

/* ---- K21: nuclei re-cut at cell borders (ark.segmentation.segmentation_utils.split_large_nuclei) ----------------------
 * Two passes over a cell plane and a nuclear plane [h, w], each of its own label dtype (PXSOM_SEG_U8 .. PXSOM_SEG_I64) and
 * row stride (ldc, ldn >= w elements); the choice between the passes is the host's, over per-cell tables.  A label names
 * cell i (nucleus j) when it equals cell_keys_dev[i] (nuc_keys_dev[j]): int32 key tables, sorted ascending and unique,
 * with their smallest and largest key (the K10 rule: a dense LUT in the workspace unless PXSOM_NUCSPLIT_FORCE_SEARCH, else
 * a binary search; both routes give identical results).  0, a value no int32 holds and a label in neither table name
 * nothing; whatever the planes hold, no label value is ever used as an index.
 *
 * pxsom_nuclear_overlaps:
 *   area_dev [n_nuc] int64      the pixels of every nucleus in the whole plane
 *   best_dev [n_cells, 2] int32 per cell the index of the nucleus with the most pixels inside the cell, the smaller index
 *                               (label) on a tie, -1 for none, and that number of pixels (0 for none)
 *   n_dev [2] int32             n_dev[1] = the RUNS of the image: stretches of one (cell label, nuclear label) pair, both
 *                               non-zero, inside a row and inside an aligned group of 64 pixels of the flat raster order,
 *                               which bounds the distinct (cell, nucleus) pairs; n_dev[0] = the distinct pairs of labels
 *                               that are both in their table, or -1 -- and area_dev, best_dev untouched -- when the runs
 *                               exceed capacity.
 *   Called with area_dev == NULL and best_dev == NULL (capacity, workspace ignored) only the runs are counted:
 *   n_dev = {0, runs}; a caller sizes the workspace from that and calls again.  The pair table has >= 2 * capacity slots
 *   and takes at most one insertion per run, and none when runs > capacity: it cannot overflow.  No n_cells x n_nuc table,
 *   no index planes, integer atomics only (the per-cell choice is a 64-bit maximum): the same input gives the same bytes
 *   on every run.  Workspace: pxsom_nuclear_overlaps_workspace_bytes (0 for a capacity outside 1 .. 2^27).
 *
 * pxsom_split_apply: out_dev [h, w] of the nuclear plane's dtype, row stride ldo.  With c, j the indices of a pixel's cell
 * and nucleus (-1: none):
 *   out[p] = (c >= 0 && j >= 0 && chosen[c] == j && cell_value[c] >= 0) ? cell_value[c]
 *          : (j >= 0 ? nuc_value[j] : nuc[p])
 * chosen_dev [n_cells] int32, cell_value_dev [n_cells] int64 (-1: the cell splits nothing), nuc_value_dev [n_nuc] int64 (the
 * label itself, or 0 for a remnant that is dropped); the values must fit the dtype.  Workspace:
 * pxsom_split_apply_workspace_bytes (the LUTs; may be 0).
 *
 * Bad sizes (h * w <= 2^31 - 1), strides, dtype codes, flags, key counts, pointers, capacity or workspace:
 * PXSOM_ERR_INVALID_ARG, the limit in the message, before any HIP call, for both entries. */
#define PXSOM_NUCSPLIT_FORCE_SEARCH 1
size_t pxsom_nuclear_overlaps_workspace_bytes(int64_t capacity, int64_t n_cells, int32_t cell_min, int32_t cell_max,
                                              int64_t n_nuc, int32_t nuc_min, int32_t nuc_max, int flags);
int pxsom_nuclear_overlaps(const void *cell_dev, int cell_dtype, int64_t ldc, const void *nuc_dev, int nuc_dtype, int64_t ldn,
                           int h, int w, const int32_t *cell_keys_dev, int64_t n_cells, int32_t cell_min, int32_t cell_max,
                           const int32_t *nuc_keys_dev, int64_t n_nuc, int32_t nuc_min, int32_t nuc_max, int64_t *area_dev,
                           int32_t *best_dev, int64_t capacity, int32_t *n_dev, void *workspace_dev, size_t workspace_bytes,
                           int flags, void *stream);
size_t pxsom_split_apply_workspace_bytes(int64_t n_cells, int32_t cell_min, int32_t cell_max, int64_t n_nuc, int32_t nuc_min,
                                         int32_t nuc_max, int flags);
int pxsom_split_apply(const void *cell_dev, int cell_dtype, int64_t ldc, const void *nuc_dev, int nuc_dtype, int64_t ldn, int h,
                      int w, const int32_t *cell_keys_dev, int64_t n_cells, int32_t cell_min, int32_t cell_max,
                      const int32_t *nuc_keys_dev, int64_t n_nuc, int32_t nuc_min, int32_t nuc_max, const int32_t *chosen_dev,
                      const int64_t *cell_value_dev, const int64_t *nuc_value_dev, void *out_dev, int64_t ldo,
                      void *workspace_dev, size_t workspace_bytes, int flags, void *stream);

/* ---- fibre object tables: per-label Euler numbers and k nearest points (K23) -----------------------------------------
 * reference: ark/segmentation/fiber_segmentation.py -- regionprops_table's euler_number column and the
 * cdist(...).argsort()[1 : 1 + k] neighbours of calculate_fiber_alignment.  Symbols added under ABI 9, none changed.
 *
 * pxsom_region_euler: per key i, euler_dev[i] (int64, every entry written) = the Euler number of (seg == keys[i]) under
 * 8-connectivity, objects minus holes, the plane padded by a zero border -- by bit quads: over every 2 x 2 window of the
 * padded plane and every distinct non-zero label l in it, the four bits (window == l) give +1 for one bit set, -1 for
 * three, -2 for two on a diagonal and 0 otherwise; the total is 4 E.  seg_dev, seg_dtype, ld, keys_dev, key_min, key_max,
 * flags and the workspace rule (pxsom_region_euler_workspace_bytes): as for pxsom_region_shape; a label past int32 is
 * background; h and w at most 2^31 - 129.  One streaming pass, integer atomics only: the same input gives the same bits.
 *
 * pxsom_nearest_indices:
 *   xy_dev    [n, 2] binary64 points, 16-byte aligned; any order inside a FOV
 *   seg_dev   [n_fovs + 1] int64 offsets, as for pxsom_neighbor_counts
 *   k         1 .. 32 (the device route's limit: the k nearest live in registers)
 *   idx_dev   [n, k] int32, every entry written: the positions in 0 .. n - 1 of the k nearest OTHER points of the row's
 *             FOV, nearest first; -1 from the first entry the FOV has no point for, and for a row no FOV holds
 * Order: s = fl(fl(dx * dx) + fl(dy * dy)) in binary64 without contraction, ties to the lower position.  Point i is
 * excluded by identity, so a point on the same coordinates as i is a neighbour.  A candidate whose s is not below +inf
 * (overflow, NaN) is never a neighbour.  No workspace; n <= 2^31 - 1.  Offsets are clamped to [0, n], so bad device-side
 * input gives wrong rows, never a write outside idx_dev.  Bad sizes, k, null / misaligned pointers:
 * PXSOM_ERR_INVALID_ARG before any HIP call. */
size_t pxsom_region_euler_workspace_bytes(int64_t n_keys, int32_t key_min, int32_t key_max, int flags);
int pxsom_region_euler(const void *seg_dev, int seg_dtype, int64_t ld, int h, int w, const int32_t *keys_dev,
                       int64_t n_keys, int32_t key_min, int32_t key_max, int64_t *euler_dev, void *workspace_dev,
                       size_t workspace_bytes, int flags, void *stream);
int pxsom_nearest_indices(const double *xy_dev, const int64_t *seg_dev, int64_t n_fovs, int64_t n, int k,
                          int32_t *idx_dev, void *stream);

/* ---- spatial-LDA featurisation: per cell, sums of feature rows over the cells within a radius (K24) -------------------
 * reference: ark/spLDA/processing.py featurize_cell_table over spatial_lda's featurize_samples (behaviour as DESIGN.md K24
 * states it; parity with spatial_lda itself unpinned).  Symbol added under ABI 9, none changed.  One stream-ordered launch
 * covers the cohort.
 *   xy_dev     [n, 2] binary64 centroids, 16-byte aligned; any order inside a FOV
 *   feat_dev   [n, n_feat] binary64, row-major; may be null when n_feat == 0
 *   seg_dev    [n_fovs + 1] int64 offsets, as for pxsom_neighbor_counts (clamped to [0, n] on the device)
 *   n_feat     >= 0 (at most 8 * 65535); 0: only the counts are produced and sums_dev may be null
 *   s_lim      cell j of the FOV of cell i (j = i included) is in i's neighbourhood when
 *              s = fl(fl(dx * dx) + fl(dy * dy)) < s_lim, binary64 without contraction (som_device.radius_threshold
 *              gives the s_lim for which this is sqrt(s) < radius, or <= radius, exactly)
 *   counts_dev [n] int32, every entry written: the size of the neighbourhood; 0 for a row no FOV holds or with NaN
 *              coordinates
 *   sums_dev   [n, n_feat] binary64, every entry written: the sum of feat[j, t] over the neighbourhood in ascending row
 *              order, one plain add per member starting from +0.0.  A member is taken by a select, not a product: a NaN
 *              or infinite feature reaches exactly the cells within the radius of its cell.
 * Every row is a query and every row of its FOV a candidate.  No atomics and no workspace: each output word is written
 * once by its owner, the same input gives the same bits, the caller need not clear anything.  Offsets are clamped, so
 * bad device-side input gives wrong rows, never an access outside the arrays.  Bad sizes, a NaN s_lim or null /
 * misaligned pointers: PXSOM_ERR_INVALID_ARG before any HIP call; n == 0 returns PXSOM_OK without a launch. */
int pxsom_neighborhood_sums(const double *xy_dev, const double *feat_dev, const int64_t *seg_dev, int64_t n_fovs,
                            int64_t n, int n_feat, double s_lim, double *sums_dev, int32_t *counts_dev, void *stream);

/* ---- fibre segmentation, from the ridge map to the inputs of the watershed (K25) --------------------------------------
 * reference: ark/segmentation/fiber_segmentation.py segment_fibers, between frangi and watershed:
 *   fg = ridges > ridge_cutoff;  dist = gaussian_filter(distance_transform_edt(fg), 1)
 *   t0, t1 = threshold_multiotsu(dist, 3) (the 256-bin histogram here, the choice on the host)
 *   markers = 0, 1 where dist < t0, 2 where dist > t1;  elevation = sobel(gaussian_filter(dist, sobel_blur)) as int32
 * (the two blurs are pxsom_gaussian_blur_plane_mode).  Symbols added under ABI 9, none changed.  Planes are [h, w] with
 * contiguous rows and a row stride in elements; h * w <= 2^31 - 1 (PXSOM_ERR_UNSUPPORTED beyond).  Null or misaligned
 * pointers, sizes < 1, strides < w, NaN scalars: PXSOM_ERR_INVALID_ARG before any HIP call; a short or null workspace:
 * PXSOM_ERR_WORKSPACE.  Integer atomics or none: the same input gives the same bits on every run.
 *
 * pxsom_distance_transform_edt: scipy.ndimage.distance_transform_edt(fg != 0).
 *   fg_dev   [h, w] uint8, row stride ld; 0 is background
 *   sq_dev   [h, w] int32, row stride ldsq, or NULL: the exact squared distance to the nearest background pixel (0 on the
 *            background)
 *   out_dev  [h, w] binary64, row stride ldo, or NULL: sqrt((double)sq), correctly rounded -- scipy's bits.  One of
 *            the two outputs must be given.
 *   A plane WITHOUT a background pixel has no nearest one: sq = INT32_MAX and out = +inf at every pixel (scipy measures
 *   to a point outside the image there).  h * h + w * w <= INT32_MAX, PXSOM_ERR_UNSUPPORTED beyond: every intermediate
 *   is then an int32.  Workspace: pxsom_distance_transform_edt_workspace_bytes(h, w) (the int32 column distances and a
 *   summary per band of 256 rows; 0 for refused sizes), 8-byte aligned.
 *
 * pxsom_plane_greater: out_dev [h, w] uint8 (row stride ldo) = plane > level, 1 / 0; a NaN pixel is 0.
 *
 * pxsom_plane_minmax: minmax_dev[0] = the smallest, minmax_dev[1] = the largest value of the plane; both NaN when the
 * plane holds a NaN.  Workspace: pxsom_plane_minmax_workspace_bytes().
 *
 * pxsom_plane_histogram: counts_dev [nbins] int64 (cleared here), nbins in 1 .. 1024, over edges_dev [nbins + 1]
 * ascending binary64 edges: bin i counts e[i] <= v < e[i + 1], the last bin also v == e[nbins]; a value outside
 * [e[0], e[nbins]] or NaN is counted nowhere.  With the edges numpy makes -- np.linspace(lo, hi, nbins + 1) -- the counts
 * are np.histogram(plane, nbins, (lo, hi))[0]: the kernel estimates a bin and then moves it until the edge test holds, so
 * the rounding of the estimate never shows.
 *
 * pxsom_sobel_magnitude: m = sqrt((a * a + b * b) / 2) with a, b = scipy.ndimage.sobel(plane, axis = 0, 1,
 * mode="reflect") / 4, binary64 without contraction in scipy's term order (difference [-1, 0, 1] along the axis, then
 * [1, 2, 1] along the other) -- scipy's bits, for any size from 1 x 1; the reflected border is resolved per index.
 *   out_dev     [h, w] binary64, row stride ldo, or NULL
 *   out_i32_dev [h, w] int32, row stride ldi, or NULL: m converted toward zero (numpy's astype for finite m < 2^31)
 *   One of the two must be given; neither may overlap the plane.
 *
 * pxsom_class_markers: out_dev [h, w] int32 (row stride ldo) = 0, then 1 where v < t0, then 2 where v > t1, compared in
 * binary64; a NaN pixel is 0. */
size_t pxsom_distance_transform_edt_workspace_bytes(int h, int w);
int pxsom_distance_transform_edt(const uint8_t *fg_dev, int h, int w, int64_t ld, double *out_dev, int64_t ldo,
                                 int32_t *sq_dev, int64_t ldsq, void *workspace_dev, size_t workspace_bytes, void *stream);
int pxsom_plane_greater(const double *plane_dev, int h, int w, int64_t ld, double level, uint8_t *out_dev, int64_t ldo,
                        void *stream);
size_t pxsom_plane_minmax_workspace_bytes(void);
int pxsom_plane_minmax(const double *plane_dev, int h, int w, int64_t ld, double *minmax_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);
int pxsom_plane_histogram(const double *plane_dev, int h, int w, int64_t ld, const double *edges_dev, int nbins,
                          int64_t *counts_dev, void *stream);
int pxsom_sobel_magnitude(const double *plane_dev, int h, int w, int64_t ld, double *out_dev, int64_t ldo,
                          int32_t *out_i32_dev, int64_t ldi, void *stream);
int pxsom_class_markers(const double *dist_dev, int h, int w, int64_t ld, double t0, double t1, int32_t *out_dev,
                        int64_t ldo, void *stream);

/* ---- fibre segmentation, the Frangi ridge filter (K26) -------------------------------------------------------------------
 * reference: ark/segmentation/fiber_segmentation.py segment_fibers, `frangi(contrast_adjusted, sigmas=fiber_widths,
 * black_ridges=False) * 10000`, in skimage 0.19's 2-D statement as recalled (parity with skimage itself is unpinned).
 * Symbol added under ABI 9, none changed.
 *
 * pxsom_frangi_scale: one scale.  g_dev is gaussian_filter(x, sigma, mode="reflect") (pxsom_gaussian_blur_plane_mode),
 * s2 = sigma^2, bsq = 2 beta^2, gsq = 2 gamma^2.  Per pixel, in binary64 without contraction:
 *   g0, g1 = np.gradient(g, axis=0), np.gradient(g, axis=1)        ((f[i+1] - f[i-1]) / 2 inside, one-sided at both ends)
 *   hrr, hrc, hcc = s2 * np.gradient(g0, axis=0), s2 * np.gradient(g0, axis=1), s2 * np.gradient(g1, axis=1)
 *   d = hrr - hcc;  r = sqrt(d*d + 4*(hrc*hrc));  t = hrr + hcc;  e_hi, e_lo = (t + r) / 2, (t - r) / 2
 *   big, small = the eigenvalue of larger and of smaller magnitude (|e_lo| >= |e_hi| takes e_lo as big: K22's rule)
 *   den = |big|, 1e-10 where that is 0;  q = small / den;  rb = q*q;  rg = small*small + big*big
 *   v = exp_neg(-rb / bsq) * (1 - exp_neg(-rg / gsq)),  0 where big > 0
 *   out = np.maximum(first ? 0 : out, v) * scale                   (a NaN on either side stays)
 * exp_neg(t), t <= 0, is the contract's own exponential in plain binary64 operations: 0 for t < -708, NaN for NaN, else
 * k = rint(t * 1.4426950408889634), r = (t - k * 0.6931471803691238) - k * 1.9082149292705877e-10, the degree-13 Taylor
 * polynomial of exp(r) by Horner over the literals 1 / k!, times 2^k built from its bit pattern.  No maths-library call:
 * the result is tests/frangi_reference.py's, bit for bit.
 *   g_dev    [h, w] binary64, row stride ldg
 *   out_dev  [h, w] binary64, row stride ldo; read unless `first`; must not overlap g
 *   scale    applied after the maximum: 1.0 except on the last scale of a fold
 * h, w >= 2 (np.gradient's demand).  Null or misaligned pointers, h or w < 2, strides < w, s2 / bsq / gsq not finite or
 * not > 0, out overlapping g: PXSOM_ERR_INVALID_ARG before any HIP call; h * w > 2^31 - 1 or h > 4 * 65535:
 * PXSOM_ERR_UNSUPPORTED.  No atomics, no workspace: the same input gives the same bits on every run. */
int pxsom_frangi_scale(const double *g_dev, int64_t ldg, int h, int w, double s2, double bsq, double gsq, int first,
                       double scale, double *out_dev, int64_t ldo, void *stream);

/* ---- fibre segmentation, adaptive histogram equalisation (K27) ------------------------------------------------------------
 * reference: ark/segmentation/fiber_segmentation.py segment_fibers, its front:
 *   blurred = gaussian_filter(channel, sigma=blur);  contrast_adjusted = equalize_adapthist(blurred / np.max(blurred),
 *   kernel_size=fov_len / contrast_scaling_divisor)
 * in skimage 0.19's statement of equalize_adapthist for a 2-D plane, a scalar kernel size k and 256 bins, as recalled
 * (tests/clahe_reference.py is the same statement in numpy; parity with skimage itself is unpinned).  The blur is
 * pxsom_gaussian_blur_plane_mode, its maximum pxsom_plane_minmax.  Symbols added under ABI 9, none changed.  Planes are
 * [h, w] with contiguous rows and a row stride in elements.
 *
 * pxsom_plane_divide: out = plane / divisor in binary64 (the division by the maximum); out may be the plane itself (same
 * pointer and stride) or must not overlap it.
 *
 * pxsom_clahe_quantize: rescale_intensity to the 2^14 grey levels.  With lo, hi the plane's minimum and maximum:
 *   lo != hi:  gray = uint16(rint((clip(v, lo, hi) - lo) / (hi - lo) * 16383 + 0))        (rint: half to even)
 *   lo == hi:  gray = uint16(rint(clip(v, 0, 16383)))                                       (the constant-plane rule)
 * in binary64 without contraction.  A NaN pixel gives 0.
 *
 * pxsom_clahe_equalize: gray [h, w] uint16 in 0 .. 16383 -> out [h, w] binary64 in [0, 1].
 *   tile (ty, tx), ty < nty = ceil(h / k), tx < ntx = ceil(w / k), covers rows [ty k, (ty + 1) k) and the columns alike;
 *     an index i >= S of an axis of length S is read at 2 (S - 1) - i (numpy's 'reflect' pad; k <= S: one reflection)
 *   hist[256] of gray / 65 over the tile;  clip_histogram(hist, min(clim, k k)) as the statement has it, loop and all
 *   map[b] = int(min(cumsum(hist)[b] * map_scale + 0, 16383)), map_scale = 16383 / (k k) from the host, binary64
 *   pixel (y, x): p = y + k / 2, b = p / k, j = p % k; rows of tiles clamp(b - 1), clamp(b) in [0, nty - 1] with weights
 *     1 - j / k, j / k (binary64); columns alike; raw = uint16(float32 sum over (0,0), (0,1), (1,0), (1,1), in this order,
 *     of float32(double(map[tile][gray / 65]) * (row weight * column weight))), truncated
 *   out = (raw - min) / (max - min) over the plane's own minimum and maximum, which stay on the device (integer atomics);
 *     min == max: out = clip(raw, 0, 1)
 *   maps_out_dev  [nty, ntx, 256] uint16, 8-byte aligned, or NULL: receives the tile maps
 *   raw_out_dev   [h, w] uint16, row stride ld_raw, or NULL: receives raw
 *   workspace     pxsom_clahe_workspace_bytes(h, w, k) bytes (0 for refused sizes), 16-byte aligned
 * A grey value above 16383 is counted in, and mapped through, bin 255: no access leaves the buffers.
 *
 * Null or misaligned pointers, h or w < 2, strides < w, k < 1 or k > min(h, w), clim < 1, lo, hi or map_scale not finite,
 * lo > hi, map_scale <= 0, a divisor that is 0 or not finite, buffers that overlap, a short workspace:
 * PXSOM_ERR_INVALID_ARG before any HIP call; h * w > 2^31 - 1 or h > 4 * 65535: PXSOM_ERR_UNSUPPORTED.  Integer atomics
 * only: the same input gives the same bits on every run. */
int pxsom_plane_divide(const double *plane_dev, int h, int w, int64_t ld, double divisor, double *out_dev, int64_t ldo,
                       void *stream);
int pxsom_clahe_quantize(const double *src_dev, int h, int w, int64_t ld, double lo, double hi, uint16_t *gray_dev,
                         int64_t ld_gray, void *stream);
size_t pxsom_clahe_workspace_bytes(int h, int w, int k);
int pxsom_clahe_equalize(const uint16_t *gray_dev, int h, int w, int64_t ld, int k, int clim, double map_scale,
                         double *out_dev, int64_t ld_out, uint16_t *maps_out_dev, uint16_t *raw_out_dev, int64_t ld_raw,
                         void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- fibre segmentation, the marker watershed (K28) ---------------------------------------------------------------------
 * reference: ark/segmentation/fiber_segmentation.py segment_fibers,
 *   segmentation = watershed(elevation_map.astype(np.int32), threshed.astype(np.int32)) - 1
 * pxsom_watershed is skimage 0.19's watershed(image, markers) at its defaults (connectivity 1, no mask, no compactness, no
 * watershed line) as recalled; tests/watershed_reference.py is the same statement in Python, and parity with skimage itself
 * is unpinned.  Symbols added under ABI 9, none changed.  The statement: a priority flood over a heap keyed (value, age).
 * Every pixel with a non-zero marker is pushed in raster order (markers of one value pop in raster order; skimage leaves
 * that to its heap); a popped pixel gives its label to each still unlabelled 4-neighbour, visited in the order -W, -1, +1,
 * +W, and pushes it: a pixel is labelled when it is pushed, and the first neighbour popped decides.  Any non-zero marker
 * value is a label, negative ones included.  A plane without a marker returns all zeros.
 *
 * The device computes that result in rounds (csrc/pxsom_watershed.hip states them): per level the frontier claims its
 * neighbours with atomicMin on a 64-bit key per pixel, basins below the level are taken whole through
 * pxsom_label_components, and the winners are emitted in key order by an exclusive scan.  The rounds are driven from the
 * host inside the entry, which therefore SYNCHRONISES the stream once per round (a 40-byte read-back).  Rounds and levels
 * are each at most h * w; crossing that bound returns PXSOM_ERR_HIP ("internal error") instead of launching again.
 *   elev_dev     [h, w] int32, row stride lde: the elevation, any int32 values
 *   markers_dev  [h, w] int32, row stride ldm
 *   out_dev      [h, w] int32, row stride ldo, every pixel written; must not overlap either input
 *   workspace    pxsom_watershed_workspace_bytes(h, w) bytes (about 54 per pixel; 0 for refused sizes), 16-byte aligned
 *   stats_host   NULL, or four int64 on the HOST: rounds, levels visited, rounds that took the basin path, pixels the flood
 *                labelled (the markers themselves are not counted)
 * Null or misaligned pointers, h or w < 1, strides < w, out overlapping an input: PXSOM_ERR_INVALID_ARG before any HIP call;
 * a short or null workspace: PXSOM_ERR_WORKSPACE; a plane beyond what pxsom_label_components takes (h * w > 2^31 - 1):
 * PXSOM_ERR_UNSUPPORTED.  Integer atomics only, and no label depends on their order: the same input gives the same bits on
 * every run. */
size_t pxsom_watershed_workspace_bytes(int h, int w);
int pxsom_watershed(const int32_t *elev_dev, int64_t lde, const int32_t *markers_dev, int64_t ldm, int h, int w,
                    int32_t *out_dev, int64_t ldo, void *workspace_dev, size_t workspace_bytes, int64_t *stats_host,
                    void *stream);

/* ---- cell overlays, Mesmer inputs and coloured masks (K29) --------------------------------------------------------------
 * reference: ark/utils/plot_utils.py create_overlay (:567-603) and save_colored_masks (:876), ark/segmentation/
 * segmentation_utils.py save_segmentation_labels (:217-219).  Symbols added under ABI 9, none changed.
 * tests/overlay_reference.py is the same statement in numpy; skimage's rescale_intensity is taken as recalled (0.19).
 *
 * pxsom_percentile_f32_listq: np.percentile(x[kept], [q...]) of float32 columns with the arithmetic numpy uses for a LIST
 * of q on a float32 array, which is not pxsom_quantile_f32's (a scalar q): the virtual index q (m - 1), its floor and the
 * fraction g are binary64, b - a is binary32, and the interpolation a + d g (g < 0.5) or b - d (1 - g) is binary64.
 * q_host [n_q] holds the quantiles q / 100 in [0, 1]; out_dev [n_q, c] binary64, NaN for a column without a kept value.
 * Same radix select, keep modes and workspace as pxsom_quantile_f32 (pxsom_quantile_workspace_bytes(n, c)).
 *
 * pxsom_overlay_rgb: one pass over contiguous [h, w] planes.  Per pixel, first the border test of each label plane,
 * find_boundaries(labels, connectivity=1, mode="inner") as pxsom_segmask states it: an in-image 4-neighbour holds another
 * label (compared in the label dtype; a neighbour outside the image counts as equal) and the pixel's own label is not 0.
 * Then per output byte j (0 red, 1 green, 2 blue), from plane j of plane_dtype (PXSOM_SEG_U8, _I16, _U16, _I32 or _F32):
 *   PXSOM_OVERLAY_ZERO     0 (an absent channel, or one whose maximum is 0); the plane may be NULL
 *   PXSOM_OVERLAY_RESCALE  y = clip(x, lo, hi); y = (y - lo) / (hi - lo) * 255.0 + 0.0; the C cast to uint8   (lo < hi)
 *   PXSOM_OVERLAY_CLIP     clip(clip(x, lo, hi), 0, 255) cast to uint8                                         (lo == hi)
 * with numpy 2's arithmetic: for a float32 plane every operation is binary32 and lo, hi, hi - lo (formed in binary64) and
 * 255.0 are each rounded to binary32 first; for an integer plane everything is binary64.  One rounding per operation (no
 * contraction), correctly rounded division.  A NaN pixel gives an unspecified byte.  Then a border pixel of seg sets the
 * three bytes to 255, and after that a border pixel of alt sets red 255, green and blue 0.
 *   r_dev, g_dev, b_dev   the planes of the three output bytes, each NULL under PXSOM_OVERLAY_ZERO
 *   modes_host [3], ranges_host [3][2] = (lo, hi) per output byte, on the HOST; ignored without rgb_dev
 *   seg_dev    [h, w] of seg_dtype (PXSOM_SEG_U8 .. PXSOM_SEG_I64);  alt_dev NULL or [h, w] of alt_dtype
 *   rgb_dev    NULL or uint8 [h, w, 3];  borders_dev NULL or uint8 [h, w], 255 on a border pixel of seg and 0 elsewhere
 * Sizes < 1, a null seg, no output at all, unknown dtype or mode, a mode without its plane, a range that is not finite or
 * does not fit the mode, an output overlapping a label plane: PXSOM_ERR_INVALID_ARG before any HIP call.
 *
 * pxsom_colorize: out[p, :] = table[mask[p], :] for a contiguous [h, w] mask (PXSOM_SEG_U8, _I16, _U16 or _I32), a uint8
 * table [n_rows, n_cols] with n_cols 3 or 4 and a uint8 output [h, w, n_cols].  status_dev (one int32, zeroed by the call)
 * gets PXSOM_COLORIZE_BAD_INDEX when an index lies outside [0, n_rows); such a pixel is written as zeros.  Negative indices
 * are refused although numpy would wrap them (as pxsom_cluster_mask refuses them). */
#define PXSOM_OVERLAY_ZERO 0
#define PXSOM_OVERLAY_RESCALE 1
#define PXSOM_OVERLAY_CLIP 2
#define PXSOM_COLORIZE_BAD_INDEX 1
int pxsom_percentile_f32_listq(const float *x_dev, int64_t n, int c, int64_t ldx, const double *q_host, int n_q,
                               int keep_mode, double *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int pxsom_overlay_rgb(const void *r_dev, const void *g_dev, const void *b_dev, int plane_dtype, const int32_t *modes_host,
                      const double *ranges_host, const void *seg_dev, int seg_dtype, const void *alt_dev, int alt_dtype,
                      int h, int w, uint8_t *rgb_dev, uint8_t *borders_dev, void *stream);
int pxsom_colorize(const void *mask_dev, int mask_dtype, int h, int w, const uint8_t *table_dev, int n_rows, int n_cols,
                   uint8_t *out_dev, int32_t *status_dev, void *stream);

/* ---- PCA scores and exact t-SNE of the cell table (K30) ------------------------------------------------------------------
 * reference: ark/analysis/dimensionality_reduction.py visualize_dimensionality_reduction, which hands the marker columns
 * to sklearn's PCA() or TSNE().  Symbols added under ABI 9, none changed.  tests/tsne_reference.py is the same statement in
 * numpy, pinned to scikit-learn 1.7.2 itself by tests/test_tsne.py.  All arithmetic is binary64, no floating-point atomic,
 * no waiting between workgroups; every sum runs over a fixed partition in a fixed order (csrc/pxsom_embed.hip states it),
 * so the same input gives the same bits on every run.  x_dev is a contiguous [n, c] matrix of dtype PXSOM_F32 or PXSOM_F64.
 *
 * pxsom_column_moments: mean_dev [c] and cov_dev [c, c] (centred products over n - 1; two passes; rows in blocks of 256
 * folded in block order).  2 <= c <= PXSOM_MAX_CHANNELS, n >= 2.  cov is exactly symmetric.
 * pxsom_project_rows: scores_dev [n, 2] = (x - mean) . axes_dev [2, c], channels ascending.
 * pxsom_pair_sqdist_f32: d2_dev [n, n] float32, d2[i, j] = sum_t (x_it - x_jt)^2 in binary64, t ascending, one rounding per
 * operation, then one rounding to float32 (sklearn's cast in _joint_probabilities); the diagonal is 0.
 *
 * pxsom_tsne_affinities: per row the search of sklearn/manifold/_utils.pyx _binary_search_perplexity as written there
 * (beta from 1, at most 100 evaluations, doubling or halving while a bound is infinite, then bisection, stop at
 * |H - log perplexity| <= 1e-5; 1e-5, 1e-8 and the perplexity taken as the binary32 nearest to them; j = i left out; a
 * zero sum replaced by 1e-8).  joint = 0 leaves the conditional rows in p_dev [n, n]; joint != 0 goes on to
 * P = max((Pc + Pc^T) / max(sum P, eps), eps), eps = 2^-52, in place (the dense form of _joint_probabilities; the
 * diagonal holds eps and no sum reads it).  beta_dev [n] and steps_dev [n] (the index of the last evaluation) say which
 * path each row took.
 *
 * pxsom_tsne_step: one iteration of sklearn's _gradient_descent on _kl_divergence for two components (one degree of
 * freedom), three launches in stream order and a fourth with want_error:
 *   Z = sum_{i != j} n_ij, n_ij = 1 / (1 + |y_i - y_j|^2): row sums, then one workgroup folds them into the one Z that
 *   every workgroup of the gradient launch reads;
 *   q_ij = max(n_ij * (1 / Z), eps), the reciprocal formed once per thread (two roundings where n_ij / Z has one);
 *   grad_i = 4 sum_j (e p_ij - q_ij) n_ij (y_i - y_j), a stream over P (each row read once);
 *   with want_error: error = sum_{i != j} e p_ij log(max(e p_ij, eps) / q_ij) and the norm of grad * gains, into
 *   error_and_gradnorm_dev [2];
 *   then per parameter, one rounding per operation: gains += 0.2 where update * grad < 0, else gains *= 0.8;
 *   gains = max(gains, min_gain); grad *= gains; update = momentum * update - learning_rate * grad; y_out = y_in + update.
 * e is the scalar `exaggeration`; P is never rewritten.  y_in_dev and y_out_dev are different [n, 2] buffers (y_in 16-byte
 * aligned); update_dev and gains_dev [n, 2] are updated in place; grad_dev is NULL or gets the gradient [n, 2] before the
 * gains.
 *
 * workspace: pxsom_tsne_workspace_bytes(n) bytes (0 for a refused n), 16-byte aligned, for both entries; P (8 n^2 bytes) and
 * d2 (4 n^2 bytes) are the caller's.  2 <= n <= PXSOM_TSNE_MAX_ROWS.  Sizes outside the limits: PXSOM_ERR_UNSUPPORTED; null
 * pointers, misalignment, y_in == y_out, non-finite parameters: PXSOM_ERR_INVALID_ARG; a short, null or misaligned
 * workspace: PXSOM_ERR_WORKSPACE; all before any HIP call. */
#define PXSOM_TSNE_MAX_ROWS 1048576
size_t pxsom_tsne_workspace_bytes(int64_t n);
int pxsom_column_moments(const void *x_dev, int64_t n, int c, int dtype, double *mean_dev, double *cov_dev, void *stream);
int pxsom_project_rows(const void *x_dev, int64_t n, int c, int dtype, const double *mean_dev, const double *axes_dev,
                       double *scores_dev, void *stream);
int pxsom_pair_sqdist_f32(const void *x_dev, int64_t n, int c, int dtype, float *d2_dev, void *stream);
int pxsom_tsne_affinities(const float *d2_dev, int64_t n, double perplexity, int joint, double *beta_dev, int32_t *steps_dev,
                          double *p_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int pxsom_tsne_step(const double *p_dev, int64_t n, const double *y_in_dev, double *y_out_dev, double *update_dev,
                    double *gains_dev, double exaggeration, double momentum, double learning_rate, double min_gain,
                    int want_error, double *error_and_gradnorm_dev, double *grad_dev, void *workspace_dev,
                    size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PXSOM_H */
