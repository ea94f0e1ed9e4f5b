/*
 * srgnn_hip.h -- C-ABI of libsrgnn_hip.so, the MI355X (gfx950) implementation of the spectral
 * feature-propagation hot path of yyysyyy/Scalable-Roubust-GNN.
 *
 * Paths below are relative to "/root/reference/Scalable Spectral Robust GNN/" (SSRG/).
 *
 * Two groups of entry points:
 *
 *  (A) Drop-in replacements with the reference's exact signatures (host pointers, synchronous).
 *      The reference binds them through numpy.ctypeslib in operators/utils.py:17-47 and :49-79;
 *      pointing that load_library call at this library moves the product onto the GPU unchanged.
 *
 *  (B) Device entry points (device pointers, asynchronous on the caller's HIP stream) used by the
 *      device-resident K-hop driver and by the row-partitioned multi-GPU path, and those of the
 *      runner's baselines: graph convolution, graph attention, the Cluster-GCN batch extraction
 *      (srg_csr_induced_f32), neighbour sampling for GraphSAGE (srg_csr_sample_f32) and the edge head of
 *      link classification (srg_pair_gather_add_f32, srg_pair_segment_sum_f32).
 *
 * Conventions for (B):
 *   - Status: 0 on success, a negative SRG_ERR_* code on failure; srg_last_error() (thread-local)
 *     then holds a message.  Nothing is launched when an argument check fails.
 *   - Ownership: the caller owns every buffer.  The library allocates nothing on these paths.
 *   - CSR: int64 row pointers (nnz may exceed 2^31), int32 column ids, row-major dense panels with
 *     explicit leading dimensions (64-bit element offsets: N*d may exceed 2^31).
 *   - Column ids are trusted on (B): validate a matrix once with srg_csr_validate() before use.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Every launch of an entry
 *     goes to the device `stream` belongs to (the current device for the null stream); the entry
 *     makes that device current for its duration and restores the caller's afterwards.
 *   - Threads: entries may be called concurrently from several host threads.  Hub rows fork onto a
 *     library-owned side stream per (device, caller stream) with its own fork / join events; the
 *     fork sequence is serialised by a library mutex.
 */
#ifndef SRGNN_HIP_H_
#define SRGNN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------------- */
#define SRG_OK 0
#define SRG_ERR_INVALID (-1)   /* bad argument (shape, null pointer, alignment, out-of-range id) */
#define SRG_ERR_HIP (-2)       /* a HIP runtime call failed */
#define SRG_ERR_ALLOC (-3)     /* device allocation failed (host-compat entries only) */

/* ---- SpMM flags ------------------------------------------------------------------------------ */
/* Default (0): every output element Y[i,c] is ONE sequential fp32 fma chain over row i's nonzeros
 * in stored CSR order, starting from +0.0f -- bit-identical to FloatCSRMulDenseOMP
 * (SSRG/operators/csrc/matmul.c:23-40) given a zeroed answer (SSRG/operators/utils.py:38).  Rows of X
 * that row i does not reference never influence Y[i,:] (a NaN or Inf in them stays out), fp32 subnormals
 * are kept, not flushed, and an empty row under SRG_SPMM_ACCUMULATE returns Y's bits unchanged. */
#define SRG_SPMM_ACCUMULATE 0x1u   /* chains start from Y's current content (matmul.c contract) */
#define SRG_SPMM_NT_STORE 0x2u     /* non-temporal stores of Y */
/* Diagnostic: one light row per wave.  By default d <= 32 runs 64 / S rows per wave (S = the power
 * of two >= d lanes per row), and d = 64 / 128 / 256 runs 512 / d light rows per wave (two 16-byte
 * column chunks per lane).  Results are identical either way. */
#define SRG_SPMM_WIDE_ROWS 0x4
/* Diagnostic: hub workgroups always use 256-nonzero windows (72 KB of LDS, two per CU).  By default
 * they do only when a launch has more hub workgroups than CUs.  Results are identical either way. */
#define SRG_SPMM_HUB_W256 0x8
/* The hub rows' workgroups are forked onto the library's hub side stream of (device, `stream`) and
 * NOT joined back into `stream` before the call returns: later launches on `stream` run beside
 * them (srgnn/dist.py issues the halo row chunks there).  The caller must srg_hub_join(stream)
 * before anything reads the hub rows, and before the next NOJOIN fork from the same stream (one
 * outstanding fork per caller stream). */
#define SRG_SPMM_HUB_NOJOIN 0x10u
/* Packed light rows keep 2 gathers per row in flight instead of 4: better for the short rows of a
 * column block (srgnn.spmm.hop passes it for column-blocked hops; products 7.15 -> 7.01 ms per hop),
 * worse for whole rows.  Results are identical either way. */
#define SRG_SPMM_PACKED_U2 0x20u
/* With SRG_SPMM_HUB_NOJOIN, after an unjoined NOJOIN fork from the same stream: the hub rows'
 * workgroups are appended to the hub side stream without a new fork from `stream` (and without
 * the dispatch delay).  For the column blocks of one hop: X is unchanged during the hop and only
 * the side stream touches the hub rows, so block b's hub span needs no order against block b-1's
 * main launch -- only against block b-1's hub span, which the side stream gives.  One join at the
 * end of the hop.  Without a pending fork it is an ordinary fork.  Results are identical.
 * The pending state belongs to the (device, stream handle) pair: join (srg_hub_join) a stream with
 * an unjoined NOJOIN fork before destroying it, or a new stream that reuses the handle value would
 * inherit the pending fork and its first CONTINUE launch would skip its own fork. */
#define SRG_SPMM_HUB_CONTINUE 0x80u
/* Tolerance mode (EXACT, FAST, ACCUMULATE).  The hub rows (the first n_hub of
 * row_order) are not one chain each: a hub row's entries are cut into 64 consecutive segments,
 * each an exact fp32 fma chain in CSR order (slice waves of the span kernel, into a scratch panel
 * taken from the stream-ordered pool with hipMallocAsync / hipFreeAsync on the hub side stream),
 * and the 64 partial sums are added in segment order (from Y's content with ACCUMULATE).  Results
 * are deterministic and within fp32 re-association error of the reference chain (the tests hold
 * them to the forward-error bound and 1e-5 relative); every other row is bit-exact.  The longest
 * row's latency drops ~64-fold: the straggler of a row-partitioned hop.  Plain and span entries
 * only (the aggregation / send / Chebyshev epilogues run exact).
 * DIAGNOSTIC / tolerance studies only: no configuration measured so far gains from it (one GPU:
 * the top row's exact chain runs beside the hop; 8 ranks: the hub group is bound by its share of
 * HBM beside the chunks, not by the top row's chain -- 1.09-1.11 ms per hop against 1.05-1.08
 * exact), so no default path sets it. */
#define SRG_SPMM_FAST 0x40u
/* The row kernel's launch reserves LDS so that at most 5 of its 4-wave blocks share a CU (gfx950's
 * 160 KiB of LDS per CU): fewer rows gather at once and the L2 re-serves more of
 * the lines they re-read.  For panels far beyond the caches (srgnn.spmm passes it for hops over
 * panels of >= 512 MiB): products 5.84 -> 5.81 ms per hop; arxiv's 87 MB panel is 3 % faster without.
 * Results are identical either way. */
#define SRG_SPMM_CAP_WAVES 0x200u

/* =============================================================================================
 * (A) drop-in entry points
 * ============================================================================================= */

/* Replaces FloatCSRMulDenseOMP, declared at SSRG/operators/csrc/matmul.h:5, defined at
 * SSRG/operators/csrc/matmul.c:23-40, bound at SSRG/operators/utils.py:34-45.
 * answer[mat_row*mat_col] += A * mat, A = CSR(data, indices, indptr) with mat_row rows; the
 * reference's caller passes a zeroed answer.  Host pointers; the product runs on the current HIP
 * device; returns after the result is back in `answer`.  The reference returns nothing and checks
 * nothing; here a failed check or HIP error leaves `answer` untouched and is reported through
 * srg_last_error_code()/srg_last_error(). */
void FloatCSRMulDenseOMP(float answer[], float data[], int indices[], int indptr[], float mat[],
                         int mat_row, int mat_col);

/* Replaces FloatCSRMulDense, SSRG/operators/csrc/cudamatmul.c:28-146 (declared void at
 * cudamatmul.h:4, defined int), bound at SSRG/operators/utils.py:65-77 (cuSPARSE CSR_ALG2 SpMM,
 * alpha = 1, beta = 0).  Overwrites answer with A * mat.  Returns 0 (EXIT_SUCCESS) or 1. */
int FloatCSRMulDense(float answer[], int data_nnz, float data[], int indices[], int indptr[],
                     float mat[], int mat_row, int mat_col);

/* =============================================================================================
 * (B) device entry points
 * ============================================================================================= */

/* One hop: Y[r,:] = A[r,:] * X for the local rows r in [0, n_rows).
 *   indptr[n_rows+1] int64, indices[nnz] int32 (ids into X's rows), values[nnz] fp32;
 *   row_order: optional (NULL) int32 permutation of [0, n_rows) giving the order in which rows are
 *              scheduled (srgnn plans pass rows by decreasing length so hubs start first);
 *   n_hub:     the first n_hub rows of row_order are hub rows: one workgroup per 32-column slice
 *              with producer waves keeping 64 KiB of gathers in flight (launched on a library-owned
 *              side stream, forked from and joined back into `stream` with events);
 *   n_heavy:   the next n_heavy rows are worked on in 32-column slices, one wave per slice (long
 *              power-law rows); both 0 without a row_order.
 *   Neither scheduling argument changes any result: every output element is one fma chain.
 *   X: ldx >= d; Y: ldy >= d.  Device pointers.  Replaces one call of csr_sparse_dense_matmul
 *   (SSRG/operators/utils.py:17-47) inside GraphOp.propagate (SSRG/operators/base_operator.py:33-35). */
int srg_spmm_csr_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                     int64_t n_rows, const int32_t* row_order, int64_t n_hub, int64_t n_heavy,
                     const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, uint32_t flags,
                     void* stream);

/* K hops: panels[k] = A * panels[k-1] for k = 1..K, panels[0] = X (read only).  `panels` is a
 * HOST array of K+1 device pointers, all with leading dimension ld.  Replaces the hop loop of
 * GraphOp.propagate, SSRG/operators/base_operator.py:32-35 (with the per-hop host round trips of
 * utils.py:38-47 removed).  A square (n_rows == rows of X).  Given no schedule (row_order NULL,
 * n_hub = n_heavy = 0) and flags within NT_STORE | FAST, the hops run through a plan built for them
 * (srg_plan_build with automatic choices -- no hub rows under FAST, so FAST changes no bit there, as
 * before the planner -- released after the hops; the call then synchronises `stream` while it plans
 * and releases, and allocates the plan's memory for its duration, so it cannot be captured into a HIP
 * graph); with a schedule, or other flags, every hop is one launch over the caller's CSR (capturable). */
int srg_propagate_khop_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                           int64_t n_rows, const int32_t* row_order, int64_t n_hub,
                           int64_t n_heavy, float* const* panels,
                           int64_t ld, int32_t d, int32_t K, uint32_t flags, void* stream);

/* One launch of a column-blocked hop, as srgnn.csr.DeviceCSR holds a column block (or block 0's two
 * parts): a CSR over the row space (row_end == NULL: row_beg has row_space + 1 entries) or row spans of
 * a shared CSR (row_end != NULL: row r's entries are [row_beg[r], row_end[r])), the schedule
 * (row_order: n_rows row ids, the first n_hub hub rows, then n_heavy slice-wave rows) and the launch's
 * SRG_SPMM_* flags (ACCUMULATE for blocks 1.., PACKED_U2, HUB_NOJOIN / HUB_CONTINUE for chained hub
 * spans, NT_STORE, FAST). */
typedef struct srg_hop_launch {
    const int64_t* row_beg;
    const int64_t* row_end;
    const int32_t* indices;
    const float* values;
    const int32_t* row_order;
    int64_t n_rows;
    int64_t n_hub;
    int64_t n_heavy;
    uint32_t flags;
    /* optional (row_end != NULL only): the spans by schedule slot, slot_beg[i] / slot_end[i] = the span
     * of row row_order[i] (n_rows entries each, or both NULL): the packed light rows read these,
     * so consecutive slots read consecutive addresses */
    const int64_t* slot_beg;
    const int64_t* slot_end;
} srg_hop_launch;

/* K column-blocked hops: for k = 1..K, the n_launch launches of `launches` (a HOST array) run in
 * order with X = panels[k-1], Y = panels[k]; with join_hub, the hub side stream (forked by the
 * first HUB_NOJOIN launch of the hop) is joined back into `stream` at the end of every hop.  The
 * device-resident form of srgnn.spmm.propagate's blocked hop loop: bitwise the one-launch hops
 * (the same fma chains, continued across the blocks).  panels: HOST array of K+1 device pointers
 * of leading dimension ld.  A plan with HUB_NOJOIN launches over K > 1 hops needs join_hub (else
 * SRG_ERR_INVALID: hop k+1 would read hub rows still being written); with join_hub = 0 (K = 1) the
 * caller must srg_hub_join(stream) after the call, before anything reads the hub rows. */
int srg_propagate_plan_f32(const srg_hop_launch* launches, int32_t n_launch, int32_t join_hub,
                           float* const* panels, int64_t ld, int32_t d, int32_t K, void* stream);

/* ---- the one-GPU planner (csrc/srg_plan.hip) ------------------------------------------------------
 * The layout of a square operator for a run of `hops` hops over d-column panels, built on the device:
 * column blocks as row spans (col_blocks: 0 = automatic -- 12..16 blocks, one per ~100 MiB, for panels
 * of 512 MiB .. 16 GiB at d >= 64 and runs of >= 4 hops, 4 for larger panels, else 1), block 0 as its cut rows' spans and its whole rows (rows of
 * <= 48 entries), per-launch schedules by decreasing span length with their hub / slice-wave counts,
 * the hub spans chained on the side stream, spans by schedule slot and, for runs of at least
 * SRG_PLAN_MIN_HOPS_TO_COMPACT hops when it fits in a quarter of the free memory, compact copies of
 * the ids and values in launch order.  The same layout srgnn.spmm.prepare gives a DeviceCSR (the
 * srgnn package builds its K-hop runs with this planner).  Replaces the reference's per-hop
 * csr_sparse_dense_matmul setup inside GraphOp.propagate (SSRG/operators/base_operator.py:32-35,
 * utils.py:17-47), which re-reads the scipy CSR every hop.
 * Unlike the other (B) entries the plan allocates device memory (hipMalloc: the schedules, the spans
 * by slot, the copies -- srg_plan_describe's device_bytes -- and a scratch arena freed before it
 * returns) and synchronises `stream` while it builds.  The plan BORROWS indptr / indices / values (span
 * layouts read them every hop): they must outlive it.  values may be NULL with SRG_PLAN_SPANS: such a
 * plan serves srg_plan_cheby_step_f64 only (which brings its fp64 values per call).  indptr[n_rows + 1], indices / values
 * [indptr[n_rows] - indptr[0]], column ids in [0, n_rows) (not validated here: srg_csr_validate).
 * hub_threshold / heavy_threshold: SRG_PLAN_AUTO (per launch, from its nnz: hub rows > max(2048,
 * nnz / 1024) entries, slice-wave rows > max(96, nnz / 100000) for the one-launch hop, nnz / 30000 for
 * a column block's), SRG_PLAN_NONE (no such rows) or a row length that holds for every launch, as a
 * DeviceCSR built with explicit thresholds schedules its blocks (srgnn.csr.make_schedule). */
typedef struct srg_plan srg_plan;
#define SRG_PLAN_MIN_HOPS_TO_CUT 4       /* automatic column blocks for runs of at least this many hops */
#define SRG_PLAN_MIN_HOPS_TO_COMPACT 6   /* automatic compact copies (when they fit) from this many */
#define SRG_PLAN_COMPACT 0x1u        /* copy the entries in launch order whatever the run length */
#define SRG_PLAN_SPANS 0x2u          /* never copy: spans of the caller's arrays */
#define SRG_PLAN_SPLIT_BLOCK0 0x4u   /* block 0 as two launches (default: panels < 16 GiB) */
#define SRG_PLAN_WHOLE_BLOCK0 0x8u   /* block 0 as one launch */
#define SRG_PLAN_WHOLE_HUBS 0x10u    /* with an explicit hub_threshold (column-blocked plans): rows longer than it
                                        are whole hub rows -- cut nowhere, one launch of their own first in the
                                        hop -- as SRG_PLAN_AUTO does for rows > max(2048, nnz / 1024) */
#define SRG_PLAN_WHOLE_MAX_SHIFT 16
#define SRG_PLAN_WHOLE_MAX(n) ((uint32_t)(n) << SRG_PLAN_WHOLE_MAX_SHIFT)   /* block 0's whole rows: at most n
                                        entries (1..65535; 0 = the default 48) -- the fp64 steps' partial sums are
                                        1 KB per row per block, so their break-even row length differs */
#define SRG_PLAN_AUTO (-1)
#define SRG_PLAN_NONE (-2)
typedef struct {
    int64_t n_rows, nnz;
    int64_t device_bytes;            /* device memory the plan holds */
    int32_t d;                       /* the panel width it was built for (any width runs it) */
    int32_t col_blocks;              /* column blocks per hop (1: the one-launch hop) */
    int32_t n_launch;                /* k_spmm launches per hop */
    int32_t compact, split_block0, hub_chain;
    int32_t device;
    int32_t hub_rows_whole;          /* rows of the whole hub rows' launch (first in the hop; 0: none) */
} srg_plan_desc;
int srg_plan_build(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                   int32_t d, int32_t hops, int32_t col_blocks, int64_t hub_threshold, int64_t heavy_threshold,
                   uint32_t opts, void* stream, srg_plan** plan);
/* The device memory srg_plan_build would take for these arguments (the ids and values are not read) --
 * keep_bytes for the plan's life,
 * scratch_bytes during the build -- and the choices it would make (resolved_opts: SRG_PLAN_COMPACT or
 * SPANS | SPLIT_BLOCK0 or WHOLE_BLOCK0; resolved_col_blocks).  One pass over indptr (synchronises
 * `stream`); nothing is allocated.  With srg_plan_build_in, a host puts the plan in memory of its own
 * allocator (srgnn: torch's caching allocator, so a plan competes for the same cached blocks as the
 * panels instead of beside them). */
int srg_plan_query(const int64_t* indptr, int64_t n_rows, int32_t d, int32_t hops, int32_t col_blocks,
                   int64_t hub_threshold, int64_t heavy_threshold, uint32_t opts, void* stream, size_t* keep_bytes,
                   size_t* scratch_bytes, uint32_t* resolved_opts, int32_t* resolved_col_blocks);
/* srg_plan_build into the caller's memory: `keep` (>= keep_bytes of srg_plan_query for the same
 * arguments and the resolved opts / col_blocks, 256-byte aligned) holds the plan until srg_plan_destroy
 * returns; `scratch` (>= scratch_bytes) only until this call returns.  The plan never frees either. */
int srg_plan_build_in(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows, int32_t d,
                      int32_t hops, int32_t col_blocks, int64_t hub_threshold, int64_t heavy_threshold, uint32_t opts,
                      void* keep, size_t keep_bytes, void* scratch, size_t scratch_bytes, void* stream,
                      srg_plan** plan);
/* Releases the plan after every reader of its memory.  The plan records, per stream its work was
 * enqueued on (its build, propagates, hops, graph replays, the row-span completion), an event after
 * that work with the hub side stream already joined; destroy makes `stream` wait for all of them,
 * joins the hub side stream of `stream`, drains `stream` (a host synchronisation), destroys the
 * executable graphs and only then frees the memory (srg_plan_build's; srg_plan_build_in's memory may
 * be reused by its owner once destroy returns).  Launches a caller ran itself from srg_plan_launch's
 * descriptors must be ordered before `stream` by the caller.  A plan is used by one host thread at a
 * time (a propagate over a width other than 64 / 128 / 256 completes its row-indexed spans in place;
 * srg_plan_launch does so up front). */
int srg_plan_destroy(srg_plan* plan, void* stream);
int srg_plan_describe(const srg_plan* plan, srg_plan_desc* desc);
/* Launch i of one hop over a d-column panel, as srg_plan_propagate_f32 runs it (flags included), and
 * whether the hops join the hub side stream at their ends: for callers that drive
 * srg_propagate_plan_f32 themselves, and for layout tests.  A compact plan built for a 64 / 128 / 256
 * column panel keeps row-indexed spans for its hub and slice-wave rows only (its light rows read the
 * spans by slot); the first srg_plan_launch call (or a propagate over another width) completes them,
 * enqueued on `stream`. */
int srg_plan_launch(const srg_plan* plan, int32_t i, int32_t d, srg_hop_launch* launch, int32_t* join_hub,
                    void* stream);
/* K hops through the plan: panels[k] = A * panels[k-1], k = 1..K (HOST array of K+1 device pointers
 * of leading dimension ld, d columns; any d, the layout was chosen for the build's d).  flags:
 * SRG_SPMM_NT_STORE, SRG_SPMM_FAST.  Bitwise srg_propagate_khop_f32's hops (FAST: its tolerance).
 * Repeated with the same panels, d, K, flags and a non-null stream, the call replays the K hops as a
 * HIP graph captured on its second occurrence (the same launches and arguments: the same bits). */
int srg_plan_propagate_f32(const srg_plan* plan, float* const* panels, int64_t ld, int32_t d, int32_t K,
                           uint32_t flags, void* stream);
/* One hop through the plan between panels of their own leading dimensions: Y = A * X (X: ldx, Y: ldy,
 * d columns; Y must not alias X) and, when agg is not NULL, the aggregation step fused into the
 * epilogue of the launch where each row's chain ends: agg = (agg_init ? 0 : agg) + w * Y (lda),
 * srg_hop_accumulate_f32's arithmetic, so bitwise the hop followed by that step.  A plan whose block 0
 * is one launch (panels >= 16 GiB) runs the hop, then that step.  flags: SRG_SPMM_NT_STORE,
 * SRG_SPMM_FAST (not with agg).  The aggregating hop of srgnn.aggregate's hop loop: the reference's
 * MessageOp.aggregate -> combine over the hop list (SSRG/operators/base_operator.py:49-59) folded
 * into the hops as they are produced. */
int srg_plan_hop_f32(const srg_plan* plan, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d,
                     uint32_t flags, float* agg, int64_t lda, float w, int32_t agg_init, void* stream);
/* One fp64 Chebyshev order through the plan: srg_cheby_step_f64's recurrence and epilogue (below), bitwise,
 * with the plan's column blocks -- each block's launch gathers from one column block of Tc and continues
 * every row's chain from the fp64 partial sum the block before stored in Tn; the epilogue runs where the
 * chain ends (block 0's whole rows, the last block) -- and its whole hub rows as hub workgroups on the
 * hub side stream (joined before the call returns to `stream`'s order).  `values`: the operator's fp64
 * values (L for INIT, F for STEP: one plan serves both, the layout depends on indptr / indices only).  The
 * plan must read spans of the caller's arrays (SRG_PLAN_SPANS; its fp32 values may be NULL, the fp32
 * entry points then refuse it) with block 0 as two launches (SRG_PLAN_SPLIT_BLOCK0) when blocked; build it
 * for twice the panel width (the layout is sized by panel bytes).  Replaces pygsp cheby_op's per-order
 * L.dot (SSRG/models/base_scalable/base_model.py:236-265) for graphs whose fp64 panels outgrow the
 * Infinity Cache. */
int srg_plan_cheby_step_f64(const srg_plan* plan, const double* values, const double* Tc, const double* To, double* Tn,
                            int64_t ld, int32_t d, int mode, double a1, double a2, const double* coef_prev,
                            const double* coef, int32_t n_scales, double* R, int64_t r_stride, void* stream);

/* Chebyshev heat-kernel filter bank (wavelet basis), SSRG/models/base_scalable/base_model.py:
 * 184-191, 236-265 via pygsp cheby_op.  One fused launch per Chebyshev order:
 *   mode SRG_CHEBY_INIT (order 1):  Tn = (A*Tc - a2*Tc) / a1;   R_s  = (c0_s/2)*Tc + c1_s*Tn
 *   mode SRG_CHEBY_STEP (order k>=2): Tn = A*Tc - To;           R_s += ck_s*Tn
 * with A = L (combinatorial Laplacian) for INIT and A = F = (2/a1)(L - a2 I) for STEP (the caller
 * builds F's values).  R holds n_scales stacked panels: R + s*r_stride.  coef_prev (c0 per scale,
 * INIT only) and coef (c1 or ck per scale) are HOST arrays of n_scales <= 8 values.  fp64 follows
 * scipy's operation order (separate multiply and add, no fma); fp32 uses fma chains.  The fused steps
 * (srg_cheby_step_*, srg_cheby_step_hub_f64, srg_plan_cheby_step_f64) also take the epilogue's lean modes
 * below (SRG_CHEBY_INIT_T, SRG_CHEBY_STEP_FIRST with coef_prev = c0 then c1 per scale, | SRG_CHEBY_NO_T):
 * the same bits, four panel passes less per order-3 filter. */
#define SRG_CHEBY_INIT 0
#define SRG_CHEBY_STEP 1
int srg_cheby_step_f64(const int64_t* indptr, const int32_t* indices, const double* values,
                       int64_t n_rows, const int32_t* row_order, const double* Tc,
                       const double* To, double* Tn, int64_t ld, int32_t d, int mode, double a1,
                       double a2, const double* coef_prev, const double* coef, int32_t n_scales,
                       double* R, int64_t r_stride, void* stream);
/* srg_cheby_step_f64 with the first n_hub rows of row_order (its longest rows) as hub rows: each runs
 * as workgroups of 16-column slices, 8 waves gathering the row's X pieces into LDS for one wave's
 * chains, on the hub side stream beside the row waves of the other rows (srg_spmm_csr_f32's hub
 * fork; joined into `stream` before the call returns).  Bitwise srg_cheby_step_f64: the same chains
 * in the same order, the same epilogue.  Hub rows need an even d and ld and a 16-byte aligned Tc
 * (otherwise every row is a row wave).  mode | SRG_CHEBY_HUB_NOJOIN leaves the hub rows running (as
 * SRG_SPMM_HUB_NOJOIN): later launches on `stream` run beside them until the caller's srg_hub_join
 * (srgnn/dist.py forks a halo rank's hub group this way, then runs its row chunks).  Only this entry
 * takes the flag. */
#define SRG_CHEBY_HUB_NOJOIN 0x20
int srg_cheby_step_hub_f64(const int64_t* indptr, const int32_t* indices, const double* values,
                           int64_t n_rows, const int32_t* row_order, int64_t n_hub, const double* Tc,
                           const double* To, double* Tn, int64_t ld, int32_t d, int mode, double a1,
                           double a2, const double* coef_prev, const double* coef, int32_t n_scales,
                           double* R, int64_t r_stride, void* stream);
int srg_cheby_step_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                       int64_t n_rows, const int32_t* row_order, const float* Tc, const float* To,
                       float* Tn, int64_t ld, int32_t d, int mode, float a1, float a2,
                       const float* coef_prev, const float* coef, int32_t n_scales, float* R,
                       int64_t r_stride, void* stream);

/* The same Chebyshev order split in two for large graphs: a load-balanced srg_spmm_csr_f32 of
 * Tc into Tn (slice waves and hub workgroups for the high-degree rows), then this element-wise
 * epilogue turning Tn = A*Tc into the next T and updating R -- bit-identical to
 * srg_cheby_step_f32 (same fma chain, same epilogue arithmetic).  Every panel has its own leading
 * dimension (column blocks of S and R without copies); R_s = R + s*r_stride, rows ldr apart. */
/* Two-pass-saving modes of the epilogue (the split path of an order >= 2 filter):
 *   SRG_CHEBY_INIT_T (order 1):     Tn = (A*Tc - a2*Tc) / a1; R untouched (coef unused)
 *   SRG_CHEBY_STEP_FIRST (order 2): Tn = A*Tc - To with To = T0, Tc = T1;
 *                                   R_s = ((c0_s/2)*T0 + c1_s*T1) + c2_s*Tn
 *                                   coef_prev = [c0_0..c0_{ns-1}, c1_0..c1_{ns-1}], coef = c2
 *   | SRG_CHEBY_NO_T (any step):    Tn is not stored (the last order: no later step reads it)
 * INIT_T then STEP_FIRST gives the same bits as INIT then STEP (same operations, same order). */
#define SRG_CHEBY_INIT_T 2
#define SRG_CHEBY_STEP_FIRST 3
#define SRG_CHEBY_NO_T 0x10
int srg_cheby_epilogue_f32(float* Tn, int64_t ldn, const float* Tc, int64_t ldc, const float* To,
                           int64_t ldo, int64_t n_rows, int32_t d, int mode, float a1, float a2,
                           const float* coef_prev, const float* coef, int32_t n_scales, float* R,
                           int64_t ldr, int64_t r_stride, void* stream);

/* The split path's two launches in one: srg_spmm_csr_f32 of Tc into Tn (load-balanced: slice waves,
 * packed light rows, hub workgroups) with srg_cheby_epilogue_f32's arithmetic fused into the
 * store, so Tn receives the next T directly -- bit-identical to the split path.  Tn may be To
 * itself (same leading dimension): every element of T_{k-1} is read by its one owner before it is
 * overwritten, so an order of any depth needs two work panels.  Tn must not alias Tc, R no panel;
 * flags as srg_spmm_csr_f32 without SRG_SPMM_ACCUMULATE.  coef_prev / coef are host arrays. */
int srg_spmm_cheby_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                       int64_t n_rows, const int32_t* row_order, int64_t n_hub, int64_t n_heavy,
                       const float* Tc, int64_t ldc, float* Tn, int64_t ldn, int32_t d, uint32_t flags,
                       int mode, float a1, float a2, const float* To, int64_t ldo, const float* coef_prev,
                       const float* coef, int32_t n_scales, float* R, int64_t ldr, int64_t r_stride,
                       void* stream);

/* Hop aggregation without the K+1 panels (fused precompute of SGC / SSGC / GBP).  The reference
 * combines the hop list on the host (SSRG/operators/message_operator/{sum,mean,simple_weighted}_
 * message_op.py; operators/utils.py:426-437 one_dim_weighted_add); the host side plans the same
 * order of element-wise steps (Python sum(): left to right from +0; torch's CPU dim-0 sum: 16-term
 * blocks folded in levels).  Per element, separate multiply / add / correctly rounded divide:
 *   SRG_ACC_INIT: agg = 0 + w*y     SRG_ACC_ADD: agg = agg + w*y     SRG_ACC_DIV: agg = agg / w
 * agg and y are device panels [n_rows, d] with leading dimensions lda / ldy (y unused for DIV).
 * The selecting modes ({min,max,concat}_message_op.py; w is ignored) move values as their 32 bits:
 *   SRG_ACC_COPY: agg = y (not INIT with w = 1: 0 + (-0) is +0)
 *   SRG_ACC_MIN:  if (!isnan(agg) && !(y >= agg)) agg = y
 *   SRG_ACC_MAX:  if (!isnan(agg) && !(y <= agg)) agg = y
 * -- torch's CPU min / max of the stacked hops applied hop by hop: the first NaN wins and sticks, a
 * tie (-0 against +0 included) keeps the earlier hop.  Bit-identical to the reference. */
#define SRG_ACC_INIT 0
#define SRG_ACC_ADD 1
#define SRG_ACC_DIV 2
#define SRG_ACC_COPY 3
#define SRG_ACC_MIN 4
#define SRG_ACC_MAX 5
int srg_hop_accumulate_f32(float* agg, int64_t lda, const float* y, int64_t ldy, int64_t n_rows,
                           int32_t d, float w, int mode, void* stream);

/* One hop of the NAFS combination (SSRG/operators/message_operator/over_smooth_distance_op.py, the
 * model of models/nafs.py) without the K+1 panels: per row r of the hop panel y, all in fp32,
 *   s = ((x0[r].y[r]) / (sqrt(sum y[r]^2) + 1e-10f)) / n0[r]        e = expf(s)
 *   acc[r,:] = (INIT ? 0 : acc[r,:]) + e * y[r,:]     z[r] = (INIT ? 0 : z[r]) + e     e_out[r*lde] = e
 * with x0 hop 0 and n0[r] = sqrt(sum x0[r]^2) + 1e-10f.  SRG_SIM_HOP0 says y is hop 0 itself: x0 is
 * not read (may be NULL) and n0 is written.  After the last hop srg_row_divide_f32 (acc[r,:] /= z[r])
 * makes the weights e_k / sum_j e_j, the reference's softmax over the hops: s is a cosine, |s| <= 1, so
 * no row maximum is subtracted and every hop is folded in as it appears.  e_out (NULL, or one float
 * per row at stride lde) receives the hop's unnormalised weight.  Deterministic -- a row's bits
 * depend on d and on the panels' alignment (16-, 8- or 4-byte accesses), not on n_rows or the
 * launch -- and within (4d + 2T + 32) * 2^-24 * sum_k w_k |X_k[r,c]| of the exact value for T
 * hops; not bit-identical to torch's CPU result, whose reduction order depends on the
 * host's SIMD width.  x0, y, acc: device panels [n_rows, d] with leading dimensions ldx0 / ldy /
 * lda; n0, z: [n_rows]; acc must not alias x0 or y. */
#define SRG_SIM_INIT 0x1
#define SRG_SIM_HOP0 0x2
int srg_hop_simweight_f32(const float* x0, int64_t ldx0, const float* y, int64_t ldy, float* n0, float* acc,
                          int64_t lda, float* z, float* e_out, int64_t lde, int64_t n_rows, int32_t d,
                          uint32_t flags, void* stream);
/* acc[r, :] = acc[r, :] / z[r] (correctly rounded), acc [n_rows, d] with leading dimension lda. */
int srg_row_divide_f32(float* acc, int64_t lda, const float* z, int64_t n_rows, int32_t d, void* stream);

/* GAMLP's learnable hop attention (SSRG/operators/message_operator/learnable_weighted_messahe_op.py,
 * combination types gate / ori_ref / jk; the model of models/gamlp.py), forward and backward, without the
 * [H*n, (T+1)*d] panel the reference's torch composition builds.  Common arguments:
 * panels / ldp are HOST arrays of T device pointers [n, d] and their leading dimensions (elements, >= d;
 * column windows of wider panels pass as they are), 1 <= T <= SRG_HOP_MAX; the slice is the H = end - start
 * panels start .. end-1 (0 <= start < end <= T); w is the weight row of Linear(in_dim, 1), b its bias
 * (device), in_dim = R + d with R = 0 (gate), d (ori_ref: [hop 0 | hop]) or T*d (jk: [all hops | hop]).
 * All four are asynchronous on `stream`, deterministic (no atomics; a result's bits depend on the shapes,
 * the slice and the panels' alignment -- 16-, 8- or 4-byte accesses -- never on the device or the launch)
 * and within the bound of DESIGN.md §5.4.2 of the formula evaluated exactly; not bit-identical to torch's
 * CPU result, whose reductions depend on the host.  n == 0 is a no-op. */
#define SRG_HOP_MAX 32
#define SRG_HOP_GATE 0
#define SRG_HOP_ORI_REF 1
#define SRG_HOP_JK 2
#define SRG_HOP_PAIR_TRANSPOSE 0   /* gate:        S[i, h] = zflat[h*n + i] */
#define SRG_HOP_PAIR_FLAT 1        /* ori_ref, jk: S[i, h] = zflat[i*H + h], the reference's .view(-1, H) */
/* Scores, hop-major: zflat[h*n + i] = (ref(i) + hop(h, i)) + b  (gate: hop(h, i) + b), with
 *   ref(i)    = sum of w[t*d + c] * F_t[i, c] over the reference panels (jk: t = 0 .. T-1; ori_ref: t = 0)
 *   hop(h, i) = sum of w[R + c] * F_{start+h}[i, c].
 * S lanes per row (the power of two >= the row's 16-, 8- or 4-byte chunks, at most 64), lane l takes
 * chunks l, l + S, ... and folds their elements with fmas in that order: the reference part as one chain
 * per lane that runs on through the panels t ascending, each hop part as its own chain from +0; the S
 * partials of a part are added in an xor butterfly (distances S/2, S/4, .., 1); then the two adds above,
 * correctly rounded.  One pass: a panel row is loaded once for both of its parts. */
int srg_hop_scores_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t start, int32_t end,
                       int kind, const float* w, const float* b, float* zflat, int64_t n, int32_t d, void* stream);
/* Attend: a = 1 / (1 + expf(-S[i, h])), e = expf(a), P[i, h] = e_h / (e_0 + e_1 + .. + e_{H-1}) (the sum
 * left to right; adds and divides correctly rounded; a is in (0, 1), so no row maximum is subtracted),
 * out[i, :] = P[i,0]*F_start[i, :] + P[i,1]*F_{start+1}[i, :] + ... left to right with separate multiply
 * and add.  P: [n, H] contiguous, kept for the backward; out: [n, d], leading dimension ldo, no alias of a
 * slice panel.  H = 1 gives P = 1 and out = the panel's bits. */
int srg_hop_attend_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t start, int32_t end,
                       const float* zflat, int pairing, float* P, float* out, int64_t ldo, int64_t n, int32_t d,
                       void* stream);
/* Attend gradient for G = dL/dout [n, d] (leading dimension ldg): dP[i, h] = G[i, :] . F_{start+h}[i, :]
 * (the scores' lane layout: one fma chain per lane from +0, the butterfly), then per row
 *   t = P_0*dP_0 + P_1*dP_1 + ... (left to right)     da_h = P_h * (dP_h - t)
 *   dS_h = da_h * (a_h * (1 - a_h))                    a_h recomputed from zflat as in the forward
 * stored through the inverse pairing: dzflat[q] = dS[i, h] where S[i, h] = zflat[q].  dP: work [n, H];
 * dzflat: [H*n]; neither aliases zflat or P. */
int srg_hop_attend_grad_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t start, int32_t end,
                            const float* G, int64_t ldg, const float* zflat, const float* P, int pairing,
                            float* dP, float* dzflat, int64_t n, int32_t d, void* stream);
/* Parameter gradient: dw [in_dim] and db [1] (either may be NULL: not computed) from dzflat, in two stages.
 * s[i] = dz[0,i] + dz[1,i] + ... (left to right).  Stage 1: group q owns rows [q*rpg, (q+1)*rpg), rpg = the
 * smallest 32 * 2^k with rpg * 2048 >= n -- a function of n alone, never of the device; per group, panel
 * and column one fma chain from +0 over the rows ascending,
 *   ref part t: fma(s[i], F_t[i, c], .)        hop part h: fma(dz[h, i], F_{start+h}[i, c], .)
 * the group's hop parts added in ascending h, its bias part s[i0] + s[i0+1] + ...  Stage 2 adds the
 * groups' partials in group order.  `scratch`: device, 16-byte aligned, srg_hop_scores_grad_scratch_bytes()
 * bytes (s and the partials).  n == 0 stores zeros. */
int srg_hop_scores_grad_scratch_bytes(int64_t n, int32_t d, int32_t T, int32_t H, int kind, int64_t* bytes);
int srg_hop_scores_grad_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t start, int32_t end,
                            int kind, const float* dzflat, float* dw, float* db, void* scratch, int64_t n,
                            int32_t d, void* stream);

/* GAMLP's recursive hop attention (SSRG/operators/message_operator/iterate_learnable_weighted_message_op.py,
 * combination type recursive), forward and backward, without the reference's H^2 panel-sized steps
 * (DESIGN.md §5.4.3).  panels / ldp / T as above; the hops used are panels 0 .. end-1 (H = end, 1 <= end <= T:
 * the reference works with start == 0 only); w = [w_h | w_c] is the weight row of Linear(2d, 1) (w_h meets
 * the hop, w_c the running combination), b its bias.  With p_j = w_h . F_j[i, :] and q_j = w_c . F_j[i, :], per
 * row i:  W(0) = [1] (NaN where (p_0 + q_0) + b is NaN: the reference's one-column softmax of a NaN gate);
 * for k = 1 .. H-1:  r = sum_{j<k} W(k-1)_j q_j,  s = (p_k + r) + b,  g_k = 1 / (1 + expf(-s)),
 * W(k) = softmax([W(k-1)_0 .. W(k-1)_{k-1}, g_k]) (the reference re-softmaxes weights that were softmaxed
 * already; kept);  out[i, :] = sum_j W(H-1)_j F_j[i, :].  Asynchronous on `stream`, deterministic (no atomics;
 * the bits depend on the shapes and the panels' alignment only), within the bound of DESIGN.md §5.4.3 of the
 * formula evaluated exactly.  n == 0 is a no-op.
 * Scores, hop-major: zp[h*n + i] = p_h, zq[h*n + i] = q_h for h = 0 .. H-1: srg_hop_scores_f32's lane layout,
 * per panel row two fma chains per lane from +0 in chunk order (w[0:d] and w[d:2d]) from one load, one xor
 * butterfly each.  The bias is not added here. */
int srg_hop_recur_scores_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t end, const float* w,
                             float* zp, float* zq, int64_t n, int32_t d, void* stream);
/* Attend: the recurrence above, one thread per row: r = W_0*q_0 + W_1*q_1 + ... left to right with separate
 * multiply and add, s = (p_k + r) + b, g_k = 1 / (1 + expf(-s)), e_j = expf(W(k-1)_j), e_k = expf(g_k),
 * W(k)_j = e_j / (e_0 + e_1 + ... + e_k) (the sum left to right; every add, multiply and divide correctly
 * rounded; the arguments lie in (0, 1], so no row maximum is subtracted).  P [n, H] contiguous receives W(H-1);
 * out[i, :] = P[i,0]*F_0[i, :] + P[i,1]*F_1[i, :] + ... left to right with separate multiply and add (out: [n, d],
 * leading dimension ldo, no alias of a panel 0 .. end-1).  work: (H (H+1) / 2 + H) * n floats kept for the
 * backward, as vectors of n: vector k (k+1) / 2 + j holds W(k)_j (j <= k), vector H (H+1) / 2 + k holds g_k.
 * H = 1 gives P = 1 and out = the panel's bits. */
int srg_hop_recur_attend_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t end, const float* zp,
                             const float* zq, const float* b, float* work, float* P, float* out, int64_t ldo,
                             int64_t n, int32_t d, void* stream);
/* Attend gradient for G = dL/dout [n, d] (leading dimension ldg): dW(H-1)_j = G[i, :] . F_j[i, :] (the scores'
 * lane layout: one fma chain per lane from +0, the butterfly), then per row, for k = H-1 .. 1:
 *   t = W(k)_0*dW_0 + ... + W(k)_k*dW_k (left to right)     dx_j = W(k)_j * (dW_j - t)
 *   ds = dx_k * (g_k * (1 - g_k))                            dzp[k*n + i] = ds
 *   dzq[j*n + i] += ds * W(k-1)_j,   dW(k-1)_j = dx_j + ds * q_j      for j < k
 * (a dzq's first term stored as it is, the later ones added in descending k; dzp[0*n + i] = 0,
 * dzq[(H-1)*n + i] = 0).  zq and work as the forward left them; dzp, dzq: [H*n], no alias of each other or zq. */
int srg_hop_recur_attend_grad_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t end,
                                  const float* G, int64_t ldg, const float* zq, const float* work, float* dzp,
                                  float* dzq, int64_t n, int32_t d, void* stream);
/* Parameter gradient: dw [2d] = [sum_i sum_h dzp[h,i] F_h[i, :] | sum_i sum_h dzq[h,i] F_h[i, :]] and
 * db [1] = sum_i s[i], s[i] = dzp[0,i] + dzp[1,i] + ... (left to right); either may be NULL: not computed.
 * srg_hop_scores_grad_f32's two stages and its rpg: per group, panel and column two fma chains from +0 over the
 * rows ascending from one load, fma(dzp[h,i], F_h[i,c], .) and fma(dzq[h,i], F_h[i,c], .), each kind added over
 * h ascending; stage 2 adds the groups' partials in group order.  `scratch`: device, 16-byte aligned,
 * srg_hop_recur_scores_grad_scratch_bytes() bytes.  n == 0 stores zeros. */
int srg_hop_recur_scores_grad_scratch_bytes(int64_t n, int32_t d, int32_t H, int64_t* bytes);
int srg_hop_recur_scores_grad_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t end,
                                  const float* dzp, const float* dzq, float* dw, float* db, void* scratch, int64_t n,
                                  int32_t d, void* stream);

/* The eight panel-reading entries above over a mini-batch of rows, without gathering the panels first
 * (the reference's loop, models/base_scalable/base_model.py BaseSGModel.forward, gathers
 * feat[idx] from every hop for every batch).  Each takes its base entry's arguments plus, after ldp,
 *   rows   B int64 on the device: batch row r of panel t is panel row rows[r], at panels[t] + rows[r] * ldp[t];
 *   n_src  the panels' row count;
 * and n = B.  Everything that is not a panel -- zflat, zp, zq, P, dP, dz*, work, out, G, the scratch (the
 * *_scratch_bytes queries with n = B), the SRG_HOP_PAIR_FLAT pairing zflat[i*H + h], the groups of the
 * parameter gradient (rpg a function of B) and the order of every fma chain -- is indexed by the batch row,
 * ascending in batch order, never in source order; duplicates and any order of indices are fine.  A result's
 * bits are those of the base entry run on [B, d] copies of the indexed rows that have the panels' access
 * width (16, 8 or 4 bytes): the same loads feed the same operations in the same order.  rows == NULL is the
 * identity: the base entry itself, n_src is not looked at.
 * Out of range: an index outside [0, n_src) is never used as an address; its batch row reads as a row of
 * +0.0f in every panel (srg_gather_rows_f32's "no fault", with the value defined).  rows is device memory, so
 * an entry cannot check it: wrap negative indices and validate on the caller's side where that matters.
 * The parameter gradient loads 16 rows a step and fetches the next step's indices behind them, so the
 * index -> address -> row chain does not serialise; the order of its fmas is the base entry's.  No atomics;
 * asynchronous on `stream`; n == 0 as the base entries. */
int srg_hop_scores_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                            int32_t T, int32_t start, int32_t end, int kind, const float* w, const float* b,
                            float* zflat, int64_t n, int32_t d, void* stream);
int srg_hop_attend_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                            int32_t T, int32_t start, int32_t end, const float* zflat, int pairing, float* P,
                            float* out, int64_t ldo, int64_t n, int32_t d, void* stream);
int srg_hop_attend_grad_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                                 int32_t T, int32_t start, int32_t end, const float* G, int64_t ldg,
                                 const float* zflat, const float* P, int pairing, float* dP, float* dzflat, int64_t n,
                                 int32_t d, void* stream);
int srg_hop_scores_grad_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                                 int32_t T, int32_t start, int32_t end, int kind, const float* dzflat, float* dw,
                                 float* db, void* scratch, int64_t n, int32_t d, void* stream);
int srg_hop_recur_scores_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                                  int32_t T, int32_t end, const float* w, float* zp, float* zq, int64_t n, int32_t d,
                                  void* stream);
int srg_hop_recur_attend_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                                  int32_t T, int32_t end, const float* zp, const float* zq, const float* b,
                                  float* work, float* P, float* out, int64_t ldo, int64_t n, int32_t d, void* stream);
int srg_hop_recur_attend_grad_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows,
                                       int64_t n_src, int32_t T, int32_t end, const float* G, int64_t ldg,
                                       const float* zq, const float* work, float* dzp, float* dzq, int64_t n,
                                       int32_t d, void* stream);
int srg_hop_recur_scores_grad_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows,
                                       int64_t n_src, int32_t T, int32_t end, const float* dzp, const float* dzq,
                                       float* dw, float* db, void* scratch, int64_t n, int32_t d, void* stream);

/* srg_spmm_csr_f32 with the aggregation step fused into its epilogue: Y = A*X as above and, for
 * every element y stored, agg = (agg_init ? 0 : agg) + w*y (separate multiply / add) -- the same
 * result as srg_spmm_csr_f32 followed by srg_hop_accumulate_f32(INIT or ADD), one panel pass less.
 * agg: device panel [n_rows, d], leading dimension lda, must not alias Y. */
int srg_spmm_agg_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                     int64_t n_rows, const int32_t* row_order, int64_t n_hub, int64_t n_heavy,
                     const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, uint32_t flags,
                     float* agg, int64_t lda, float w, int agg_init, void* stream);

/* One column block of a hop over ROW SPANS: row r's entries are [row_beg[r], row_end[r]) of the
 * shared indices / values arrays (both int64 [n_rows]), otherwise srg_spmm_csr_f32 (agg == NULL)
 * or srg_spmm_agg_f32 (agg != NULL).  When every row of Â holds sorted column ids (utils.py:81-93
 * builds them so), the entries of row r whose ids fall in a column block are one span of the row,
 * so block b of a hop is this call with row_beg = split_b, row_end = split_{b+1} (split_0 =
 * indptr[0:n], split_B = indptr[1:n+1]): no copy of the ids or values.  Block 0 runs from +0.0f,
 * blocks 1.. with SRG_SPMM_ACCUMULATE continue every chain from the fp32 value the previous block
 * stored -- the same fmas in the same order as the one-launch hop, so the same bits.  row_order /
 * n_hub / n_heavy schedule the spans' lengths.  Replaces one call of csr_sparse_dense_matmul
 * (SSRG/operators/utils.py:17-47) inside GraphOp.propagate's hop loop (base_operator.py:33-35). */
int srg_spmm_span_f32(const int64_t* row_beg, const int64_t* row_end, const int32_t* indices,
                      const float* values, int64_t n_rows, const int32_t* row_order, int64_t n_hub,
                      int64_t n_heavy, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d,
                      uint32_t flags, float* agg, int64_t lda, float w, int agg_init, void* stream);

/* The last flat elements (< SRG_TAIL_MAX of them) of a torch dim-0 sum take its scalar row_sum
 * order (4 interleaved partials).  srg_tail_record_f32 stores w * y[flat_start + e] (flat index of
 * the row-major [n_rows, d] panel) into hist[e], one call per term with hist advanced by
 * SRG_TAIL_MAX floats; srg_tail_rowsum_f32 then writes 0 + row_sum(hist[0..n_terms)) into agg. */
#define SRG_TAIL_MAX 32
int srg_tail_record_f32(float* hist, const float* y, int64_t ldy, int32_t d, int64_t flat_start,
                        int32_t len, float w, void* stream);
int srg_tail_rowsum_f32(float* agg, int64_t lda, int32_t d, int64_t flat_start, int32_t len,
                        const float* hist, int32_t n_terms, void* stream);

/* construct_adj on the device (SSRG/operators/utils.py:81-93, adj_to_symmetric_norm): out[s] =
 * ((0 + v[p[s]]) + v[p[s]+1]) + ... over vals[seg_ptr[s] .. seg_ptr[s+1]) in fp64, left to right
 * -- the order in which scipy merges duplicate entries of adj + I (the row sums of the degrees
 * are srg_segment_sum_numpy_f64).  seg_ptr has n_seg + 1 entries; all pointers are device pointers. */
int srg_segment_sum_f64(const int64_t* seg_ptr, const double* vals, int64_t n_seg, double* out, void* stream);
/* The same in fp32: the directed families' fp32 normalisations (SSRG/operators/utils.py:195-424:
 * torch_scatter.scatter_add over fp32 edge weights, a sequential sum in element order). */
int srg_segment_sum_f32(const int64_t* seg_ptr, const float* vals, int64_t n_seg, float* out, void* stream);

/* The row degrees of adj_to_symmetric_norm in the order of scipy's csr.sum(1), which is
 * np.add.reduceat: out[s] = a[0] + pairwise(a[1:]) over a = vals[seg_ptr[s] .. seg_ptr[s+1]), with
 * numpy's pairwise sum (fewer than 8 elements left to right; up to 128 in eight strided accumulators
 * folded as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus the remainder left to right; longer runs split
 * at n/2 rounded down to a multiple of 8).  An empty segment gives +0.  fp64 only. */
int srg_segment_sum_numpy_f64(const int64_t* seg_ptr, const double* vals, int64_t n_seg, double* out,
                              void* stream);

/* fp64 Y = A * X (X [rows of A's columns, d], ldx; Y [n_rows, d], ldy) in scipy's csr_matvec(s)
 * order (each element from 0, adding the separately rounded product of every stored entry in
 * storage order): the W @ x step of the fast PPR power iteration in
 * adj_to_fast_ppr_approx_symmetric_norm (SSRG/operators/utils.py:284-291) and the stationary
 * distribution of the two-order operator (:338-356).  Not a hop kernel. */
int srg_spmm_csr_f64(const int64_t* indptr, const int32_t* indices, const double* values, int64_t n_rows,
                     const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t d, void* stream);

/* Row gather, the send-side pack of the multi-GPU halo exchange (srgnn/dist.py; no reference
 * counterpart -- the reference is single process): dst[i, :] = src[idx[i], :] for i < n_idx, a C
 * host's pack step before its RCCL sends.  src [n_src, d] / dst [n_idx, d] are device panels with
 * leading dimensions lds / ldd; idx is int64 on the device.  An index outside [0, n_src) leaves its
 * dst row unwritten (no fault).  Asynchronous on `stream`. */
int srg_gather_rows_f32(const float* src, int64_t lds, int64_t n_src, const int64_t* idx, int64_t n_idx,
                        float* dst, int64_t ldd, int32_t d, void* stream);

/* `stream` waits (on the device, not the host) for the hub workgroups of the last hub launch
 * forked from `stream` (an SRG_SPMM_HUB_NOJOIN one); no-op if none was forked. */
int srg_hub_join(void* stream);
/* Diagnostic: the number of live hub side streams over all devices (at most 8 per device; a caller
 * stream's entry is evicted, least recently used first, unless it has an unjoined NOJOIN fork). */
int srg_hub_side_streams(void);

/* Column-block split points of a device CSR for srg_spmm_span_f32 (asynchronous on `stream`):
 * splits[(b-1) * n_rows + r] = the first entry of row r with column id >= ceil(b * n_cols / n_blocks)
 * (binary search over the row's sorted ids), b = 1 .. n_blocks-1; splits: int64 [(n_blocks-1) * n_rows].
 * For any row the split points lie in [indptr[r], indptr[r+1]] and never decrease with b, so the
 * spans partition every row in CSR order and the blocked hop stays exact even for unsorted rows
 * (which only lose the blocks' locality).  n_blocks in [2, 64]. */
int srg_csr_col_splits(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                       int32_t n_blocks, int64_t* splits, void* stream);

/* Span copy (the compact column blocks of srgnn.csr.DeviceCSR: a launch's entries laid out in the
 * order it takes its rows): for i < n_order, row r = order[i] has its span [beg[r], end[r]) of
 * indices / values copied to [pos[i], pos[i] + end[r] - beg[r]) of out_indices / out_values, and
 * out_beg[r] / out_end[r] set to that range (pos: the exclusive prefix sum of the spans' lengths in
 * `order`; rows not in `order` keep their out_beg / out_end).  Asynchronous on `stream`. */
int srg_csr_copy_spans(const int32_t* order, int64_t n_order, const int64_t* beg, const int64_t* end,
                       const int32_t* indices, const float* values, const int64_t* pos, int32_t* out_indices,
                       float* out_values, int64_t* out_beg, int64_t* out_end, void* stream);

/* Mirror positions (device construct_adj, srgnn/construct.py; SSRG/operators/utils.py:91 transposes
 * A+I): for a CSR whose rows hold strictly increasing column ids, mirror[e] = the position of entry
 * (c, r) in row c for entry e = (r, c) (rows[e] = r, int64 [nnz]), or -1 when row c has no column r.
 * Every entry found <=> the structure is symmetric, and the transpose is then the same structure
 * with values[mirror].  Asynchronous on `stream`. */
int srg_csr_mirror(const int64_t* indptr, const int32_t* indices, const int64_t* rows, int64_t n_rows,
                   int64_t nnz, int64_t* mirror, void* stream);

/* Checks a device CSR: indptr[0] == 0, indptr non-decreasing, indptr[n_rows] == nnz, and every
 * column id in [0, n_cols).  Synchronous on `stream`.  Returns SRG_OK or SRG_ERR_INVALID. */
int srg_csr_validate(const int64_t* indptr, const int32_t* indices, int64_t n_rows,
                     int64_t nnz, int64_t n_cols, void* stream);

/* The induced sub-graph of a node set (srgnn.cluster, DESIGN.md 5.12: the Cluster-GCN mini-batches of the
 * reference's train_minibatch): row b < B of the result is row nodes[b] of the operator (indptr int64 from 0
 * to nnz, trusted; indices int32, NOT trusted), its entries filtered and relabelled through pos.
 *   pos given (int32 [n_cols], pos[nodes[b]] = b and -1 elsewhere): an entry with column id c is kept iff
 *     0 <= c < n_cols and pos[c] >= 0, and stored with column id pos[c]: scipy's A[S][:, S] for S = nodes.
 *   pos NULL (a row slice): every entry is kept and its id copied verbatim: scipy's A[S].
 * Kept entries keep the operator's stored order inside their row, duplicates stay duplicates, out_val is
 * the entry's value bit for bit and out_eid its index in indices / values.  nodes: int64 [B] on the device,
 * distinct, in any order; a nodes[b] outside [0, n_rows) gives an empty row and is never used as an address,
 * nor is a column id outside [0, n_cols).
 * Two passes over the same arguments, as srg_spgemm_f32: phase 0 writes cnt[b] = kept entries of row b
 * (int64 [B]); the caller forms ptr (int64 [B + 1], the exclusive prefix sum of cnt) and allocates the
 * outputs of ptr[B] entries; phase 1 writes row b's kept entries at ptr[b] .. of out_idx and, where not
 * NULL, out_val (needs values) and out_eid.  A kept entry's slot is its rank among its row's kept entries:
 * no atomics, the same bytes from run to run.  Row lengths, nnz and the output size are 64-bit; n_cols and
 * B are at most 2^31 - 1 (pos is int32).  B == 0 launches nothing; another phase, a negative size, n_cols
 * or B >= 2^31: SRG_ERR_INVALID.  Asynchronous on `stream`; neither allocates nor synchronises. */
int srg_csr_induced_f32(int phase, const int64_t* indptr, const int32_t* indices, const float* values,
                        int64_t n_rows, int64_t n_cols, const int64_t* nodes, int64_t B, const int32_t* pos,
                        int64_t* cnt, const int64_t* ptr, int32_t* out_idx, float* out_val, int64_t* out_eid,
                        void* stream);

/* The sampled row slice of a node set (srgnn.neighbor, DESIGN.md 5.13: the neighbour-sampled mini-batches
 * GraphSAGE is trained on): row b < B of the result is row v = nodes[b] of the operator (indptr int64,
 * trusted; indices int32, copied verbatim and never used as an address; values float or NULL), of stored
 * length len, cut to at most `fanout` entries:
 *   cnt = len       if fanout < 0 or len <= fanout: the row is copied in stored order, values bit for bit,
 *                   out_eid = indptr[v] + position;
 *   cnt = fanout    otherwise: the entries at the positions p_t = walk(t), t = 0 .. fanout - 1, of the keyed
 *                   bijection srg_sample_distinct_i64 documents (below), over m = len with no shift past a
 *                   query node and key = mix(seed + 0x9E3779B97F4A7C15 * (v + 1)).  The key is the node id,
 *                   not the batch position: a node's sample is a function of (seed, v, len, fanout) alone,
 *                   whatever batch it is in.  The positions are distinct by construction and are emitted in
 *                   ascending position, i.e. in stored order: a sampled row's fma chain is a sub-sequence
 *                   of the full row's.
 * The count is closed form, so there is no count phase: the caller forms ptr (int64 [B + 1], the exclusive
 * prefix sum of cnt) from indptr and allocates ptr[B] entries.  The entry trusts ptr[b + 1] - ptr[b] only
 * where it equals its own cnt: a row for which it does not is not written.  A nodes[b] outside [0, n_rows)
 * is an empty row and never an address.  out_val (needs values) and out_eid may be NULL.
 * The cycle walk is bounded by the domain size 4^h, which no cycle of a permutation exceeds; a row whose walk
 * hit the bound (a bijection's never does) is left unwritten.
 * 1 <= fanout <= SRG_SAMPLE_MAX_FANOUT or fanout < 0; fanout == 0, fanout > SRG_SAMPLE_MAX_FANOUT, a negative
 * size or B >= 2^31: SRG_ERR_INVALID.  A sampled row holds fewer than 2^31 entries (a longer one is not
 * written).  B == 0 launches nothing.  No atomics: the same bytes from run to run.  Asynchronous on `stream`;
 * neither allocates nor synchronises. */
#define SRG_SAMPLE_MAX_FANOUT 64
int srg_csr_sample_f32(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                       const int64_t* nodes, int64_t B, int32_t fanout, uint64_t seed, const int64_t* ptr,
                       int32_t* out_idx, float* out_val, int64_t* out_eid, void* stream);

/* ---- the edge head of link classification (srgnn.link) -------------------------------
 * Every base model of the reference ends its link-classification forward with
 * linear(cat(f[q[:, 0]], f[q[:, 1]], dim=-1)) (SSRG/models/base_scalable/simple_models.py).  With the weight
 * split by side, W = [W0 | W1], the dense products run once per distinct endpoint node (P = z [W0; W1]^T,
 * [U, 2C], through the caller's GEMM) and the two passes over the E query pairs below are C wide; nothing of
 * shape [E, 2h] exists.  All panels are row-major fp32 with leading dimensions in elements (a column window
 * of a wider panel is fine); rows are read and written 16 bytes at a time when C % 4 == 0 and every base
 * pointer and leading dimension allows it, 4 bytes at a time otherwise, with the same bits either way. */

/* out[e, c] = (P[q[e, 0], c] + P[q[e, 1], C + c]) + b[c] for e < E, c < C: this association, two fp32
 * roundings (one without b: b may be NULL).  P: [U, 2C] (ldp >= 2C); q: int64 [E, 2], contiguous, positions
 * in [0, U): a position outside that range reads as a row of +0.0f and is never used as an address; out:
 * [E, C] (ldo >= C).  E == 0 or C == 0 launches nothing.  E, U < 2^31 - 64; a negative size or a leading
 * dimension below its width: SRG_ERR_INVALID.  Asynchronous on `stream`; neither allocates nor
 * synchronises. */
int srg_pair_gather_add_f32(const float* P, int64_t ldp, int64_t U, const int64_t* q, const float* b, int64_t E,
                            int32_t C, float* out, int64_t ldo, void* stream);

/* The adjoint's segment sums: S[v, side * C + c] = the sum of g[e, c] over the slots (e, side) of node v,
 * i.e. over the e with q[e, side] == v.  The caller hands the incidence over: inc_ptr (int64 [U + 1],
 * trusted to ascend; clamped to [0, 2E]) and inc_slot (int64 [2E]; slot = 2 e + side, a node's slots
 * ascending: a stable sort of the 2E positions by node).  Every element is ONE sequential fp32 chain
 * ((+0.0f + g[e_1, c]) + g[e_2, c]) + ... over the node's slots of that side in stored order; the slots of
 * the other side are skipped, never added as + 0.  An empty segment gives +0.0f.  A slot outside [0, 2E) is
 * skipped and never used as an address.  g: [E, C] (ldg >= C); S: [U, 2C] (lds >= 2C), every element written.
 * No atomics: the same bits from run to run.  A node's segment is one lane group's serial chain (DESIGN.md
 * 5.14: a node with very many slots is not split).  U == 0 or C == 0 launches nothing.  E, U < 2^31 - 64; a
 * negative size or a leading dimension below its width: SRG_ERR_INVALID.  Asynchronous on `stream`; neither
 * allocates nor synchronises. */
int srg_pair_segment_sum_f32(const float* g, int64_t ldg, int64_t E, const int64_t* inc_ptr, const int64_t* inc_slot,
                             int64_t U, int32_t C, float* S, int64_t lds, void* stream);

/* ---- the sparse wavelet basis built on the device ---------------------------------------------------
 * SpectralModel.calculate_wavelet + normalize_matrices (SSRG/models/base_scalable/base_model.py:236-265,
 * 287-290) from the filter's dense output (srg_cheby_step_f64's R) to the L1-normalised CSR basis, without
 * the dense block leaving the device: threshold + compact per block (count, prefix sum by the caller,
 * fill), the blocks' rows appended (sp.hstack(blocks).tocsr()), sklearn's normalize(norm='l1') in place.
 * Every result is bit for bit the reference's; nothing is added atomically: run-to-run identical. */

/* Threshold and compact a dense fp64 block R [n_rows, w] (row stride ldr >= w, in elements; a column
 * window of a wider panel is fine) that holds columns col0 .. col0 + w - 1 of the matrix
 * (sub[sub < tol] = 0; csr_matrix(sub.astype(float32))): entry (i, c) survives iff
 *   !(R[i,c] < tolerance)  &&  (float)R[i,c] != 0.0f
 * -- a NaN entry and a NaN tolerance keep the entry (numpy's mask), -0 and fp64 values that round to fp32
 * zero are dropped, values that round to an fp32 subnormal are kept, +-Inf follow the comparison.  It is
 * stored as (float)R[i,c] (round to nearest even) with column id col0 + c, columns ascending in the row.
 * Two passes over the same arguments, as srg_spgemm_f32: phase 0 writes cnt[r] = survivors of row r (int64
 * [n_rows]); the caller forms ptr (the exclusive prefix sum of cnt) and allocates idx / val; phase 1 writes
 * row r's survivors at ptr[r] .. of idx / val.  The same bits whether the 16-byte path (R on 16 bytes,
 * ldr even) or the 8-byte path runs.  n_rows == 0 or w == 0 launches nothing; ldr < w, col0 < 0,
 * col0 + w > INT32_MAX or another phase: SRG_ERR_INVALID.  Asynchronous on `stream`. */
int srg_dense_sparsify_f64(int phase, const double* R, int64_t ldr, int64_t n_rows, int32_t w, double tolerance,
                           int32_t col0, int64_t* cnt, const int64_t* ptr, int32_t* idx, float* val, void* stream);
/* Appends the rows of one block's CSR to a CSR under construction: row r's entries
 * src_idx / src_val[src_ptr[r] .. src_ptr[r+1]) are copied to dst_idx / dst_val at cursor[r], then
 * cursor[r] += their count (cursor: int64 [n_rows], initially the final indptr[:-1]).  Calls on one stream
 * append in call order, so a row's entries follow block order: the hstack.  Asynchronous on `stream`. */
int srg_csr_append_rows_f32(const int64_t* src_ptr, const int32_t* src_idx, const float* src_val, int64_t n_rows,
                            int64_t* cursor, int32_t* dst_idx, float* dst_val, void* stream);
/* sklearn.preprocessing.normalize(M, norm='l1', axis=1) in place (_inplace_csr_row_normalize_l1): per
 * row, acc = the fp64 sum of |x| over the stored entries, left to right from +0 (one sequential chain);
 * if acc != 0 every value becomes (float)((double)x / acc), else the row is left as it is; a NaN acc is
 * != 0, so the row becomes NaN.  indptr: int64 [n_rows + 1].  Asynchronous on `stream`. */
int srg_csr_row_normalize_l1_f32(const int64_t* indptr, float* values, int64_t n_rows, void* stream);

/* ---- sparse x sparse: the wavelet model's phi * phi^-1 (torch_sparse.spspmm / spmm) ------------------
 * SpectralModel.preprocess (SSRG/models/base_scalable/base_model.py:208-219) multiplies the two sparse
 * wavelet bases with torch_sparse.spspmm and the product into the features with torch_sparse.spmm
 * (torch_sparse is absent here; its published CPU algorithms, which are scipy csr_matmat's arithmetic,
 * are restated): C[i,j] = ((0 + A[i,k1]*B[k1,j]) + A[i,k2]*B[k2,j]) + ... over row i of A in stored
 * order, each product rounded before it is added; sums equal to 0 dropped; columns ascending.
 * Two passes over the same arguments: phase 0 writes c_cnt[m] (entries per row of C); the caller
 * forms c_ptr (m + 1, exclusive prefix sum) and allocates C; phase 1 fills c_idx / c_val.
 * B with more than 16384 columns needs `scratch` (device, srg_spgemm_scratch_bytes() bytes, or any
 * smaller multiple of one row accumulator: fewer workgroups); B's row pointers index b_idx / b_val,
 * its column ids must be < n_cols.  SRG_SPGEMM_SERIAL_B: B's rows may repeat a column id (then each
 * B row is walked by one lane).  Asynchronous on `stream`. */
#define SRG_SPGEMM_SERIAL_B 0x1u
int srg_spgemm_scratch_bytes(int64_t m, int64_t n_cols, int64_t* bytes);
int srg_spgemm_f32(int phase, const int64_t* a_ptr, const int32_t* a_idx, const float* a_val, int64_t m,
                   const int64_t* b_ptr, const int32_t* b_idx, const float* b_val, int64_t n_cols,
                   int64_t* c_cnt, const int64_t* c_ptr, int32_t* c_idx, float* c_val, void* scratch,
                   int64_t scratch_bytes, uint32_t flags, void* stream);
/* The adjoint of C = A * B (A: m x k, B: k x n, C's pattern as srg_spgemm_f32 emits it) with respect to
 * the values of either operand, for G = dL/dC in C's entry order; one kernel serves both sides:
 *   out[e] = ((0 + D[r, j1] * R[c, j1]) + D[r, j2] * R[c, j2]) + ...   for every entry e = (r, c) of a
 * pattern P, over row c of R in stored order, every product rounded before it is added (no fma), from
 * +0; D[r, j] is +0 where row r of D stores no entry (j1, j2, ... are row c of R's column ids).
 *   dL/dA: P = A's pattern, D = G on C's CSR (m rows), R = B, n_cols = n:
 *          gA[(i,k)] = sum over row k of B in stored order of G[i,j] * B[k,j];
 *   dL/dB: P = B^T's pattern, D = G^T (n rows), R = A^T, n_cols = m, the transposes by a stable sort by
 *          column: gB[(k,j)] = sum over A's entries in column k, rows ascending and duplicates in stored
 *          order, of A[i,k] * G[i,j]; out is in B^T's entry order (the caller permutes it back).
 * With R's rows column-sorted these are scipy csr_matmat's chains of G * B^T and A^T * G sampled at the
 * patterns; duplicate entries of P each get the full value; an entry of C that the forward dropped (an
 * exact-zero sum) is a +0 of D.  p_ptr and d_ptr have m + 1 entries; p_idx indexes R's rows; d_idx and
 * r_idx are < n_cols; a row of D must not repeat a column id (R's and P's rows may).  out has one
 * float per entry of P.  n_cols > 16384 needs `scratch` (device): srg_spgemm_scratch_bytes(m, n_cols)
 * bytes are enough, any multiple of one accumulator (4 * n_cols bytes) does (fewer workgroups).  No
 * atomics: run-to-run identical.  Non-finite inputs are undefined.  Asynchronous on `stream`. */
int srg_spgemm_grad_f32(const int64_t* p_ptr, const int32_t* p_idx, int64_t m, const int64_t* d_ptr,
                        const int32_t* d_idx, const float* d_val, const int64_t* r_ptr, const int32_t* r_idx,
                        const float* r_val, int64_t n_cols, float* out, void* scratch, int64_t scratch_bytes,
                        void* stream);
/* torch_sparse.spmm(index, value, m, n, matrix) (index_select, mul, scatter_add): Y[r, :] = sum over
 * row r's entries in stored order of (v * X[c, :]), each product rounded, then added, from +0.  A CSR
 * whose rows hold the COO entries in index order (a stable sort by row). */
int srg_spmm_muladd_f32(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                        const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, void* stream);
/* The sampled dense-dense product (SDDMM): torch_sparse.spmm's gradient with respect to `value`.  For
 * every entry e = (r, c) of a CSR pattern (indptr: int64 [n_rows + 1] from 0 to nnz; indices: int32 [nnz],
 * rows of X) and panels G [n_rows, d] (row stride ldg) and X [., d] (row stride ldx), both strides in
 * elements and >= d (column windows of wider panels are fine):
 *   out[e] = ((((+0 + G[r,0]*X[c,0]) + G[r,1]*X[c,1]) + ...) + G[r,d-1]*X[c,d-1]),
 * columns ascending from +0, every product rounded to fp32 before it is added (no fma); d == 0 writes +0.
 * NaN, +-Inf, -0 and subnormals follow IEEE through this chain (nothing is flushed).  Duplicate entries
 * each get the full value.  perm (int64 [nnz], a permutation) may be NULL; if given, entry e's result
 * goes to out[perm[e]] (the caller's COO order, with perm the row sort's permutation), else to out[e].
 * nnz is passed because the host cannot read indptr[n_rows]; the pattern is trusted.  One lane runs one
 * entry's whole chain and nothing is added atomically: run-to-run identical, and the same bits whether
 * the aligned (16-byte loads) or the unaligned path runs.  n_rows == 0 or nnz == 0 is a no-op.
 * Asynchronous on `stream`. */
int srg_sddmm_f32(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const float* G,
                  int64_t ldg, const float* X, int64_t ldx, int32_t d, const int64_t* perm, float* out,
                  void* stream);
/* The two products of the fused graph-wavelet filter Y = phi * (theta (.) (phi^-1 * Z)) and of its adjoints
 * (srgnn.wavelet_conv), for narrow panels (d of 1 to 64; any d works).  CSR as for
 * srg_spmm_muladd_f32 (indptr: int64 [n_rows + 1] from 0 to nnz, trusted; a row holds fewer than 2^31
 * entries), X [., d] with row stride ldx and Y [n_rows, d] with row stride ldy, strides in elements and
 * >= d (column windows and unaligned bases are fine):
 *   Y[r, j] = chain over row r's entries e in stored order of fl( fl(v_e * scale[s_e]) * X[indices[e], j] ),
 *   s_e = r when scale_axis == 1, indices[e] when scale_axis == 0;
 * every chain starts from +0, every product is rounded before it is added, one output is one sequential
 * chain.  scale == NULL skips the rescale: the bits of srg_spmm_muladd_f32.  scale_axis must be 0 or 1
 * whether or not scale is given.  NaN, +-Inf, -0 and subnormals follow IEEE through the chain.  No
 * atomics: run-to-run identical.  n_rows == 0 or d == 0 is a no-op.  Asynchronous on `stream`. */
int srg_spmm_scaled_f32(const int64_t* indptr, const int32_t* indices, const float* values, const float* scale,
                        int32_t scale_axis, int64_t n_rows, const float* X, int64_t ldx, float* Y, int64_t ldy,
                        int32_t d, void* stream);
/* The row sums of a value-weighted sampled dense-dense product (the filter's gradient with respect to
 * theta): for every row k of the CSR, with G [., d] (row stride ldg; rows the column ids index) and
 * P [n_rows, d] (row stride ldp),
 *   out[k] = chain over row k's entries e in stored order of fl( v_e * s_e ),
 *   s_e    = chain over j ascending of fl( G[indices[e], j] * P[k, j] )   (srg_sddmm_f32's chain),
 * from +0, products rounded before they are added.  An empty row writes +0; d == 0 writes +0 to every
 * row.  IEEE special values pass through; no atomics.  n_rows == 0 is a no-op.  Asynchronous on `stream`. */
int srg_sddmm_rowsum_f32(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                         const float* G, int64_t ldg, const float* P, int64_t ldp, int32_t d, float* out,
                         void* stream);

/* ---- edge augmentation: nearest sampled candidates per node ----------------------------------------
 * edge_augument (SSRG/data_augument.py:73-103, helpers utils.py:29-38) gives every low-degree node edges to
 * the nearest of its randomly drawn candidate nodes, nearest in the L2 distance between feature rows.  The
 * two entries below are its per-node work for all low-degree nodes at once (srgnn.augment does the rest
 * with device sorts): the draw of the candidates and the distance + selection. */

/* Candidates per query row at most (the row's distance keys stay in LDS: 16 KiB per wave at the cap);
 * 4,096 = degree_level 40 at the reference's 100 candidates per missing edge. */
#define SRG_KNN_MAX_CAND 4096
/* Feature columns at most (the query row is kept in LDS beside the keys). */
#define SRG_KNN_MAX_D 8192
/* Query rows per kernel launch of both entries; more rows go out in further launches on the same stream.
 * Part of no result -- every row is computed alone -- and stated here so that a test can cross it. */
#define SRG_KNN_LAUNCH_ROWS 4194304

/* For query row r < n_query: the k_r = out_ptr[r+1] - out_ptr[r] nearest of the candidates
 * cand[cand_ptr[r] .. cand_ptr[r+1]) (M_r of them, node ids) to node query[r], nearest first, written to
 * sel[out_ptr[r] ..) and, when sel_dist is not NULL, their distances to sel_dist[out_ptr[r] ..).
 * X [n, d] fp32 with row stride ldx >= d in elements (a column window of a wider panel and an unaligned
 * base are fine); query / cand_ptr / cand / out_ptr / sel: int64 on the device.
 *
 * Distance (fp32, nothing fused, every operation rounded to nearest even, nothing flushed):
 *   t_j = fl(X[q, j] - X[c, j]),  s_j = fl(t_j * t_j),  dist = sqrt(S) correctly rounded,
 * where S adds the s_j in this order, a function of d alone:
 *   P = ceil(d / 4) pieces of 4 consecutive columns; G = the smallest power of two >= P, at most 64.
 *   Partial sum p_g, g < G, takes the pieces g, g + G, g + 2G, ... in that order and inside a piece the
 *   columns ascending, as one chain from +0: p_g = (((+0 + s_a) + s_b) + ...); a p_g without columns is +0.
 *   Then the halving tree: for h = G/2, G/4, ..., 1:  p_g = p_g + p_{g+h} for g < h.  S = p_0.
 * d == 0: every distance is +0.  A NaN distance is written to sel_dist as 0x7FC00000.
 *
 * Order: ascending distance; equal distances (and +0 against +0) by position in the row's candidate list,
 * earlier first; NaN distances after +Inf, in position order (torch.sort's NaN-last rule); candidates
 * whose id lies outside [0, n) after all of those, in position order -- such an id is never used as an
 * address, and its sel_dist is 0x7FC00000.  The same bits whatever M_r, k_r, the position, the stride and
 * the load path (16-byte loads when X lies on 16 bytes and ldx is a multiple of 4, else 4-byte loads).
 * No atomics touch the result: run-to-run identical.
 *
 * n_query == 0 launches nothing; k_r == 0 and M_r == 0 are legal rows (when no row asks for a result, nothing
 * is launched after the check and cand / sel may be NULL).  d < 0, d > SRG_KNN_MAX_D, ldx < d,
 * n < 0: SRG_ERR_INVALID at once.  The pointer arrays are checked on the device before the selection is
 * launched (this waits for `stream` once): a decreasing cand_ptr or out_ptr, k_r > M_r, query[r] outside
 * [0, n) or M_r > SRG_KNN_MAX_CAND: SRG_ERR_INVALID with a message, nothing selected.  The selection itself
 * is asynchronous on `stream`.  The check allocates two status words on `stream`, copies them to the host
 * and waits, on every call: the entry cannot be captured into a graph, and a caller who has checked the
 * arrays already still pays one synchronisation.
 *
 * The LDS of a wave is sized by the longest candidate list of the whole call (rounded up to 64), not by
 * its own row's, and a workgroup shrinks from four waves to two or one to stay within 64 KiB.  One list at
 * the cap (16 KiB of keys per wave) among many short ones therefore lowers the occupancy of every row of the
 * call: callers with a few very long lists among many short ones do better with one call per length class. */
int srg_knn_select_f32(const float* X, int64_t ldx, int64_t n, int32_t d, const int64_t* query,
                       const int64_t* cand_ptr, const int64_t* cand, const int64_t* out_ptr, int64_t n_query,
                       int64_t* sel, float* sel_dist, void* stream);

/* Draws the candidates: row r < n_query receives M_r = cand_ptr[r+1] - cand_ptr[r] distinct node ids in
 * [0, n), none equal to query[r], at cand[cand_ptr[r] ..); entry t of row r is a function of (seed, r, t,
 * n, query[r]) only.  This is NOT the reference's random stream (Python's random.sample over a list it
 * mutates): it is a keyed bijection of [0, n - 1) evaluated at t = 0 .. M_r - 1, so the ids are distinct by
 * construction, shifted past the query node (x >= query[r] becomes x + 1).  Integer arithmetic only
 * (uint64, wrapping), so that a host restates it bit for bit:
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   key = mix(seed + 0x9E3779B97F4A7C15 * (r + 1))
 *   m = n - 1;  h = the smallest h >= 1 with 4^h >= m;  mask = 2^h - 1
 *   F_i(R) = mix(key ^ (0xD6E8FEB86659FD93 * (i + 1)) ^ R) & mask
 *   perm(x): L = x >> h, R = x & mask; four rounds i = 0..3: (L, R) = (R, L ^ F_i(R)); result (L << h) | R
 *            (a Feistel network: a bijection of [0, 4^h))
 *   x = perm(t); while x >= m: x = perm(x)   (cycle walking: t < m, so the walk returns below m)
 * query[r] outside [0, n), a decreasing cand_ptr or M_r > n - 1: SRG_ERR_INVALID, checked on the device
 * before the draw is launched (the same check as above: it waits for `stream` once, so no graph capture).
 * n_query == 0 launches nothing. */
int srg_sample_distinct_i64(const int64_t* query, const int64_t* cand_ptr, int64_t n_query, int64_t n,
                            uint64_t seed, int64_t* cand, void* stream);

/* ---- graph convolution restricted to a batch of rows ------------------------------------------------
 * The reference's GCN (Layer2GraphConvolution, SSRG/models/simple_models.py) multiplies by the whole
 * operator in its last layer and reads output[idx] only.  The two entries below are that product for the
 * batch's rows alone and its adjoint (srgnn.graph_conv); the full products go through the
 * planned hop.  fp32; CSR as for srg_spmm_csr_f32 (indptr int64 from 0 to nnz, indices int32, trusted);
 * panels are row-major with row strides in elements, >= d (column windows and unaligned bases are fine).
 * Neither entry uses atomics or scratch: run-to-run identical.  16-byte loads when d and both strides are
 * multiples of 4 and both panels lie on 16 bytes, else 4-byte loads: the same bits either way.  A row is
 * one wave's serial chain, so a row of L entries costs its length whatever else runs.
 * Both are asynchronous on `stream` and make no host synchronisation. */

/* Y[b, :] = A[rows[b], :] X for b < B: per element the chain acc = fmaf(values[e], X[indices[e], j], acc)
 * over row rows[b]'s entries in stored order from +0.0f -- the bits of srg_spmm_csr_f32 for that row.
 * rows: int64 [B] on the device, in any order, repeats allowed.  An id outside [0, n_rows) gives a row of
 * +0 and is never used as an address.  X [n_cols, d], ldx; Y [B, d], ldy.  B == 0 or d == 0 is a no-op. */
int srg_gconv_rows_f32(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                       const int64_t* rows, int64_t B, const float* X, int64_t ldx, float* Y, int64_t ldy,
                       int32_t d, void* stream);

/* The adjoint: dX = A[rows, :]^T G over the rows of the transposed operator (indptr_t, indices_t, values_t;
 * n rows, column ids in [0, n)).  pos: int32 [n] on the device, pos[r] = b where rows[b] = r and -1 where r
 * is not in the batch (the ids of a batch are unique).  For every row c < n,
 *   dX[c, j] = chain over row c's entries e in stored order, from +0.0f, of
 *              acc = fmaf(values_t[e], G[pos[indices_t[e]], j], acc)
 * taken over the entries with pos[indices_t[e]] in [0, B) only.  Every other entry is skipped, not
 * multiplied by zero: an Inf or NaN value outside the batch does not reach dX.  A row without a member
 * entry is +0; all n rows are written.  A column id outside [0, n) and a position outside [0, B) are never
 * used as addresses.  G [B, d], ldg; dX [n, d], ldx.  n == 0 or d == 0 is a no-op; B == 0 writes +0. */
int srg_gconv_rows_adjoint_f32(const int64_t* indptr_t, const int32_t* indices_t, const float* values_t, int64_t n,
                               const int32_t* pos, int64_t B, const float* G, int64_t ldg, float* dX, int64_t ldx,
                               int32_t d, void* stream);

/* ---- graph attention: the aggregation of a GAT layer, forward and backward --------------------------
 * GATConv's aggregation (srgnn.gat) is a sparse product whose values are a softmax, over
 * each target's incoming edges, of a leaky-ReLU score per edge and head.  A is a CSR over targets: row
 * i < n_rows holds the sources j in [0, n_src) of i's incoming edges (indptr int64 from 0 to nnz, trusted;
 * indices int32, NOT trusted: an id outside [0, n_src) is skipped everywhere and never used as an address).
 * Hf [n_src, H*C] (row stride ldh) holds the transformed features, heads side by side; a_src [n_src, H] and
 * a_dst [n_rows, H] are contiguous.  Per row i, head h, over the row's valid entries e with source j_e:
 *   s_e = a_src[j_e,h] + a_dst[i,h];  l_e = s_e > 0 ? s_e : slope * s_e;  m = max_e l_e;  p_e = expf(l_e - m)
 *   z = sum_e p_e;  acc[c] = fmaf(p_e, Hf[j_e,h*C+c], acc[c]) from +0.0f in stored order;  out = acc / z.
 * Row sums of length L (z, da_dst, da_src) are taken in this order, a function of the positions alone: lane
 * l of 64 adds the terms at positions l, l + 64, ... in that order from +0.0f, then p_l = p_l + p_{l+w} for
 * l < w, w = 32, 16, ..., 1; the sum is p_0.  Sums over a head's C columns (D, dalpha) are one fmaf chain
 * from +0.0f, columns ascending.  Nothing uses atomics, allocates or synchronises; every result is run-to-run
 * identical, the same with 16-byte loads (C and the strides multiples of 4, bases on 16 bytes) as with
 * 4-byte loads, and head h of an H-head call has the bits of a one-head call on that head's columns.
 * A row is one wave's serial work (DESIGN.md 5.11 states a long row's cost).  Asynchronous on `stream`. */

/* Heads at most. */
#define SRG_GAT_MAX_HEADS 32
/* H * C at most (the width of a row of Hf, out, G and dHf). */
#define SRG_GAT_MAX_WIDTH 65536
/* Rows (and per-row-and-head items) per kernel launch of the three entries; more go out in further launches
 * on the same stream.  Part of no result; stated here so that a test can cross it. */
#define SRG_GAT_LAUNCH_ROWS 4194304

/* out [n_rows, H*C] (row stride ldo), M [n_rows, H] = m and Z [n_rows, H] = z, both kept for the backward.
 * A row without a valid entry gives out = +0, M = 0, Z = 0.  n_rows == 0 is a no-op; nnz == 0 or n_src == 0
 * launches no kernel and zeroes out, M and Z.  H outside [1, SRG_GAT_MAX_HEADS], C < 1,
 * H*C > SRG_GAT_MAX_WIDTH, a row stride < H*C, a negative size: SRG_ERR_INVALID. */
int srg_gat_attend_f32(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows, int64_t n_src,
                       const float* a_src, const float* a_dst, float slope, const float* Hf, int64_t ldh, int32_t H,
                       int32_t C, float* out, int64_t ldo, float* M, float* Z, void* stream);

/* The per-edge part of the backward, with G = dL/dout [n_rows, H*C] (row stride ldg) and out, M, Z as the
 * forward left them; alpha_e = expf(l_e - M[i,h]) / Z[i,h]:
 *   D[i,h]  = chain over c of G[i,h*C+c] * out[i,h*C+c]                 (scratch [n_rows, H] of the caller)
 *   ds[e,h] = (alpha_e * (chain over c of G[i,h*C+c] * Hf[j_e,h*C+c] - D[i,h])) * (s_e > 0 ? 1 : slope)
 *             written to dS [nnz, H] in A's order; +0 for a skipped entry
 *   da_dst[i,h] = the row sum of ds[., h] over row i.
 * n_rows == 0 is a no-op; nnz == 0 or n_src == 0 zeroes da_dst and launches nothing. */
int srg_gat_edge_grad_f32(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows, int64_t n_src,
                          const float* a_src, const float* a_dst, float slope, const float* Hf, int64_t ldh,
                          int32_t H, int32_t C, const float* out, int64_t ldo, const float* M, const float* Z,
                          const float* G, int64_t ldg, float* D, float* dS, float* da_dst, void* stream);

/* The part of the backward that runs over the transpose At (n_src rows; indices_t are targets in
 * [0, n_rows), skipped when outside) and perm (entry t of At is entry perm[t] of A; an index outside
 * [0, nnz) is skipped):
 *   dHf[j,h*C+c] = chain from +0.0f over row j of At in stored order of fmaf(alpha_t, G[i_t,h*C+c], .)
 *   da_src[j,h]  = the row sum over row j of At of dS[perm[t], h]
 * A target whose Z[i,h] is 0 (a row of A without a valid entry, which a consistent At never names) adds
 * nothing to dHf; srg_gat_edge_grad_f32 writes ds = +0 for the entries of such a row.
 * Either result may be NULL and is then not computed (dS and perm are read for da_src only; a_src, a_dst,
 * M, Z and G for dHf only).  n_src == 0 is a no-op; nnz == 0 or n_rows == 0 zeroes the results. */
int srg_gat_attend_adjoint_f32(const int64_t* indptr_t, const int32_t* indices_t, const int64_t* perm, int64_t nnz,
                               int64_t n_rows, int64_t n_src, const float* a_src, const float* a_dst, float slope,
                               int32_t H, int32_t C, const float* M, const float* Z, const float* G, int64_t ldg,
                               const float* dS, float* dHf, int64_t ldd, float* da_src, void* stream);

/* ---- graph attention for a batch of rows: the last layer, whose output the loss reads at a batch only ----
 * The three entries above for the rows of a batch: the same arithmetic in the same orders,
 * so for finite operands every result has the bits the full entries give with G zero outside the batch.
 *   rows  int64 [B]         the batch's target ids, unique; NOT trusted: an id outside [0, n_rows) is never an
 *                           address
 *   pos   int32 [n_rows]    pos[rows[b]] = b and -1 elsewhere; NOT trusted: a value outside [0, B) is no member
 *   eptr  int64 [B + 1]     the prefix sum of the batch rows' lengths, eptr[b + 1] - eptr[b] =
 *                           indptr[rows[b] + 1] - indptr[rows[b]], nnzB = eptr[B]; trusted as indptr is, but
 *                           no compact position at or past nnzB is read or written
 * out, M, Z, G, D and da_dst are compact: row b belongs to rows[b].  a_src, a_dst and Hf are the full tables
 * (a_dst is read at the row's id).  dS is compact [nnzB, H]: entry k of row rows[b] is at eptr[b] + k.
 * B outside [0, 2^31 - 64) or nnzB < 0: SRG_ERR_INVALID, with the checks of the full entries. */

/* out [B, H*C] (row stride ldo), M [B, H], Z [B, H]: row b is what srg_gat_attend_f32 gives for row rows[b].
 * An id outside [0, n_rows) gives out = +0, M = Z = 0.  B == 0 is a no-op; nnz == 0, n_src == 0 or
 * n_rows == 0 launches no kernel and zeroes out, M and Z. */
int srg_gat_attend_rows_f32(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows, int64_t n_src,
                            const int64_t* rows, int64_t B, const float* a_src, const float* a_dst, float slope,
                            const float* Hf, int64_t ldh, int32_t H, int32_t C, float* out, int64_t ldo, float* M,
                            float* Z, void* stream);

/* The per-edge part of the backward for the batch, with G = dL/dout [B, H*C] (row stride ldg) and out, M, Z as
 * srg_gat_attend_rows_f32 left them: D [B, H] (scratch of the caller), dS [nnzB, H] and da_dst [B, H] as in
 * srg_gat_edge_grad_f32, da_dst[b] summed over [eptr[b], eptr[b + 1]).  A row whose id is out of range
 * writes nothing to dS.  B == 0 is a no-op; nnz == 0, n_src == 0 or n_rows == 0 zeroes da_dst and launches
 * nothing.  dS may be NULL when nnzB == 0. */
int srg_gat_edge_grad_rows_f32(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows,
                               int64_t n_src, const int64_t* rows, int64_t B, const int64_t* eptr, int64_t nnzB,
                               const float* a_src, const float* a_dst, float slope, const float* Hf, int64_t ldh,
                               int32_t H, int32_t C, const float* out, int64_t ldo, const float* M, const float* Z,
                               const float* G, int64_t ldg, float* D, float* dS, float* da_dst, void* stream);

/* The part over the transpose At (and A's own indptr, for an entry's place in its row).  Entry t of row j of
 * At, with target i = indices_t[t], is a member when i lies in [0, n_rows) and b = pos[i] in [0, B):
 *   dHf[j,h*C+c] = chain from +0.0f over the member entries of row j in stored order of
 *                  fmaf(expf(l_t - M[b,h]) / Z[b,h], G[b,h*C+c], .); a member with Z[b,h] == 0 adds nothing
 *   da_src[j,h]  = the row sum over row j of At, in the order of the section above, of
 *                  dS[eptr[b] + (perm[t] - indptr[i]), h] for the members whose perm[t] lies in [0, nnz) and
 *                  whose compact position lies in [eptr[b], eptr[b + 1]) and below nnzB
 * Every other entry is skipped, not multiplied by zero, and leaves its position out of the row sum; no value
 * of indices_t, pos or perm is an address before it is range-checked.  A pos that names another member's
 * position is not detected: that entry is computed with the other row's M, Z and G.  All n_src rows of
 * dHf [n_src, H*C] (row stride ldd) and da_src [n_src, H] are written; either may be NULL and is then not
 * computed.  n_src == 0 is a no-op; nnz == 0, n_rows == 0 or B == 0 zeroes the results. */
int srg_gat_attend_rows_adjoint_f32(const int64_t* indptr_t, const int32_t* indices_t, const int64_t* perm, int64_t nnz,
                                    int64_t n_rows, int64_t n_src, const int32_t* pos, int64_t B,
                                    const int64_t* indptr, const int64_t* eptr, int64_t nnzB, const float* a_src,
                                    const float* a_dst, float slope, int32_t H, int32_t C, const float* M,
                                    const float* Z, const float* G, int64_t ldg, const float* dS, float* dHf,
                                    int64_t ldd, float* da_src, void* stream);

/* ---- multi-GPU: communicators and the row-partitioned K-hop propagation ---------------------------
 * SURVEY.md §8(b) item 5, for C / C++ hosts (the Python package drives the same kernels through
 * torch.distributed: srgnn/dist.py).  RCCL is loaded at run time.  Rank r owns rows
 * [row_starts[r], row_starts[r+1]) of Â and of every hop panel.  srg_dist_propagate_khop_f32 is
 * SURVEY §8(e)'s all-gather, chunked by owner and overlapped with the SpMM: per hop every pair of
 * ranks swaps its blocks of the previous panel (grouped ncclSend / ncclRecv on a stream of that
 * pair: all links at once, lower ranks first), and each rank multiplies its rows in P column blocks
 * (block q = the entries whose columns rank q owns: a span of every row, since Â's rows hold sorted
 * ids), in ascending q, block q as soon as rank q's rows have arrived, blocks 1.. continuing the
 * chains (SRG_SPMM_ACCUMULATE).  Every hop is bitwise the one-GPU hop (each row's fma chain is
 * unchanged).  Rows with unsorted column ids are rejected (SRG_ERR_INVALID).  The halo exchange
 * below (srg_halo_*) moves only the referenced rows and is the faster path.  Replaces the
 * reference's single-process hop loop, SSRG/operators/base_operator.py:32-35. */
typedef struct srg_comm srg_comm;
#define SRG_COMM_ID_BYTES 128
/* RCCL unique id (SRG_COMM_ID_BYTES bytes) to share out of band before srg_comm_init_rank. */
int srg_comm_unique_id(void* id_out);
/* One rank per process: `device` is this process's HIP device. */
int srg_comm_init_rank(int nranks, const void* id, int rank, int device, srg_comm** comm);
/* One process driving ndev devices (devices == NULL: 0 .. ndev-1); rank i = devices[i]. */
int srg_comm_init_all(int ndev, const int* devices, srg_comm** comm);
int srg_comm_destroy(srg_comm* comm);
int srg_comm_size(const srg_comm* comm);

/* One local rank's share (device pointers on `device`). */
typedef struct {
    int device;
    const int64_t* indptr;        /* [n_rows + 1], rebased to 0 */
    const int32_t* indices;       /* global column ids (rows of the gathered panel) */
    const float* values;
    int64_t row0, n_rows;         /* must equal the rank's row_starts block */
    const int32_t* row_order;     /* optional schedule, as srg_spmm_csr_f32 */
    int64_t n_hub, n_heavy;
    float* x_full;                /* [row_starts[P], ld] gather buffer */
    float* const* panels;         /* HOST array of K + 1 pointers, each [n_rows, ld]; panels[0] = own X rows */
    void* stream;                 /* hipStream_t of `device` (NULL: its null stream) */
} srg_shard_f32;

/* panels[k] = (rank's rows of Â) * (panel k-1 gathered from every rank), k = 1..K, for every local
 * shard (shards[i] belongs to the communicator's i-th local rank).  Asynchronous on each shard's
 * stream, apart from one host sync per call (the owner split points and the sortedness check);
 * library-owned pair streams carry the exchange, and scratch for the split points comes from the
 * stream-ordered pool ((P - 1) * n_rows int64 per shard, freed at the end of the call). */
int srg_dist_propagate_khop_f32(srg_comm* comm, const srg_shard_f32* shards, int n_shards,
                                const int64_t* row_starts, int64_t ld, int32_t d, int32_t K);

/* ---- multi-GPU: the halo-exchange partition (the default multi-GPU path) -----------------------
 * The row-partitioned K-hop of srg_dist_propagate_khop_f32 moves every rank's whole block each hop
 * (an all-gather, 2.6x the bytes on the products graph at 8 ranks) and computes after the exchange.
 * The halo path moves only the remote rows each rank's rows reference, and overlaps that exchange
 * with the hop: a rank's rows are cut into C nnz-balanced row chunks plus one group of hub rows;
 * per hop the hub group is forked beside the chunks, and after each chunk's launch its rows that
 * peers need are packed and sent (grouped ncclSend / ncclRecv on a comm stream that waits only for
 * that pack), while the next chunks compute; the hub group's rows go last.  Low-degree halo rows
 * whose own columns are all local ("ghost rows") are computed locally instead of received.  Every
 * row keeps its entries in CSR order, so the hops are bitwise the one-GPU hops.  The same plan as
 * the Python package's srgnn/dist.py HaloPartitionedOperator runs on (it builds its shares with this
 * planner).  Replaces the reference's single-process hop loop, SSRG/operators/base_operator.py:32-35;
 * SURVEY.md §8(b) item 5, §8(e). */
#define SRG_HALO_AUTO (-1)     /* threshold chosen as the Python plan does (csr.auto_*_threshold) */
#define SRG_HALO_NONE (-2)     /* hub_threshold: no hub rows */
typedef struct srg_halo_plan srg_halo_plan;
typedef struct srg_halo_share srg_halo_share;
typedef struct {
    int64_t row0, n_rows;          /* own rows [row0, row0 + n_rows) of the global operator */
    int64_t n_recv, n_ghost, halo; /* panel rows after the own ones: received, then ghosts */
    int64_t nnz_local;             /* entries of the local CSR (own rows + ghost rows) */
    int64_t n_groups, hub_rows, send_rows;
    int32_t ghost_max_degree, chunks, nranks, rank;
} srg_halo_info;
/* Rank `rank`'s share, from the GLOBAL CSR on the host (int64 indptr[n+1] from 0, int32 column ids;
 * the same arrays on every rank).  chunks in [1, 250]; hub_threshold / heavy_threshold a row length,
 * SRG_HALO_AUTO, or (hub) SRG_HALO_NONE; ghost_max_degree >= 0 (0: no ghost rows) or SRG_HALO_AUTO:
 * the cap among 0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64 that minimises the modelled hop, max over
 * ranks of max(local SpMM bytes incl. ghost rows at 8.4e12 B/s, busiest peer link at link_bps per
 * direction; a row is 4d bytes on both sides, so d cancels) -- deterministic from the global graph
 * and link_bps, so every rank picks the same cap (pass every rank the same link_bps, e.g. the minimum
 * over ranks of a measured rate; <= 0: 64e9).  srg_halo_plan_info reports the cap taken.  Host-only:
 * needs no device; up to 16 host threads.  Validates the CSR (SRG_ERR_INVALID). */
int srg_halo_plan_build(const int64_t* indptr, const int32_t* indices, int64_t n, int32_t nranks, int32_t rank,
                        int32_t chunks, int64_t hub_threshold, int64_t heavy_threshold, int32_t ghost_max_degree,
                        double link_bps, srg_halo_plan** plan);
int srg_halo_plan_destroy(srg_halo_plan* plan);
int srg_halo_plan_info(const srg_halo_plan* plan, srg_halo_info* info);
/* Read-only view of one of the plan's host arrays (diagnostics and tests): *data points into the plan
 * (valid until it is destroyed), *count elements of the type given beside each selector. */
#define SRG_HALO_STARTS 0             /* int64 [nranks + 1] row blocks */
#define SRG_HALO_LOCAL_INDPTR 1       /* int64 [n_rows + halo + 1] */
#define SRG_HALO_LOCAL_INDICES 2      /* int32 [nnz_local] panel row ids */
#define SRG_HALO_GHOST_POSITIONS 3    /* int64: global entry positions of the ghost rows' entries */
#define SRG_HALO_HALO_IDS 4           /* int64 [halo] global ids of the halo rows, panel order */
#define SRG_HALO_GROUP_OFFSETS 5      /* int64 [n_groups] */
#define SRG_HALO_GHOST_SEND 6         /* int64 own local rows sent as peers' ghosts (X only) */
#define SRG_HALO_GHOST_SEND_COUNTS 7  /* int64 [nranks] */
#define SRG_HALO_GHOST_RECV_COUNTS 8  /* int64 [nranks] */
#define SRG_HALO_CHUNK_RANGES 9       /* int64 [chunks + 1] local row bounds of the chunks */
#define SRG_HALO_HUB_THRESHOLDS 10    /* int64 [nranks] */
#define SRG_HALO_VIEW_ORDER 11        /* int32 schedule of view `index` (chunks, hub group, ghosts) */
#define SRG_HALO_VIEW_META 12         /* int64 [4]: rows, hub rows, slice rows (d > 32), slice rows (d <= 32) */
#define SRG_HALO_SEND_ROWS 13         /* int64 own local rows sent in group `index`, peers ascending */
#define SRG_HALO_SEND_COUNTS 14       /* int64 [nranks] of group `index` */
#define SRG_HALO_RECV_COUNTS 15       /* int64 [nranks] of group `index` */
int srg_halo_plan_array(const srg_halo_plan* plan, int32_t what, int32_t index, const void** data, int64_t* count);
/* The share on `device`: local CSR (values gathered from the GLOBAL fp32 host array `values`),
 * schedules, send lists, a send buffer for panels up to d_max columns, a comm stream and events.
 * The plan must outlive the share.  The row chunks run in column blocks when d_max's panel asks for
 * them (srg_halo_share_col_blocks' automatic rule). */
int srg_halo_share_create(const srg_halo_plan* plan, const float* values, int device, int32_t d_max,
                          srg_halo_share** share);
int srg_halo_share_destroy(srg_halo_share* share);
/* Column blocks of the row chunks' launches (srgnn/dist.py HaloPartitionedOperator.chunk_blocks):
 * each chunk runs as n_blocks span launches over the own rows' spans whose GLOBAL column ids lie in
 * [ceil(b n / B), ceil((b+1) n / B)), rows of <= 48 entries whole in block 0, later blocks continuing
 * the chains (ACCUMULATE): bitwise the unblocked hop, with column locality for wide panels.
 * n_blocks in [1, 64] (1: unblocked) applies to every d; SRG_HALO_AUTO (the share's default) picks 8
 * for local panels ([own | halo] rows x d x 4 B) of >= 8 GiB at d >= 256, else 1, per call's d
 * Builds the split points and schedules on the host and uploads them (synchronous). */
int srg_halo_share_col_blocks(srg_halo_share* share, int32_t n_blocks);
/* Panel 0 from the WHOLE feature matrix X [n, ldx] on the share's device (as GraphOp.propagate is
 * handed the whole feature): own rows, then the halo rows gathered by global id.  Then pass
 * SRG_HALO_X_HALO_FILLED to srg_halo_propagate_f32 (no exchange of X). */
int srg_halo_fill_x_halo(const srg_halo_share* share, const float* X, int64_t ldx, float* panel0, int64_t ld,
                         int32_t d, void* stream);
/* K hops for the local shares of `comm` (shares[i] is the communicator's i-th local rank; for a
 * loopback communicator, ranks 0 .. nranks-1 in order).  panels: per share, a HOST array of K + 1
 * device pointers, each a [n_rows + halo, d] panel (ld == d: the halo rows are RCCL buffers) on the
 * share's device; panel 0's own rows hold X's rows of the rank, its halo is exchanged first unless
 * flags has SRG_HALO_X_HALO_FILLED.  streams: per share (NULL array or entries: the null stream).
 * Asynchronous on those streams; every panel k's own rows (and halo, k < K) are bitwise the one-GPU
 * hop k.  d <= the shares' d_max. */
#define SRG_HALO_X_HALO_FILLED 0x1u
int srg_halo_propagate_f32(srg_comm* comm, srg_halo_share* const* shares, int n_shards, float* const* const* panels,
                           int64_t ld, int32_t d, int32_t K, uint32_t flags, void* const* streams);
/* A communicator of nranks virtual ranks in ONE process on one device whose exchange is device-to-
 * device copies on a library stream: srg_halo_propagate_f32 then runs every rank's share (its
 * kernels, packs, groups and offsets) on one GPU -- the tests' and a single-GPU host's rehearsal of
 * the RCCL path.  Serves srg_halo_propagate_f32 only. */
int srg_comm_init_loopback(int nranks, int device, srg_comm** comm);

/* ---- diagnostics ----------------------------------------------------------------------------- */
const char* srg_last_error(void);   /* thread-local message of the last failure ("" if none) */
int srg_last_error_code(void);      /* thread-local status of the last call (SRG_OK if fine)  */
void srg_clear_error(void);
const char* srg_version(void);      /* build identification, incl. the offload arch          */

/* ---- test hooks ------------------------------------------------------------------------------ */
/* Every kernel family sends a large grid out in several launches (of at most 2^23 blocks, 2^24 one-wave
 * blocks, or SRG_GAT_LAUNCH_ROWS / SRG_KNN_LAUNCH_ROWS rows), and the grid-stride kernels clip their
 * grids.  srg_debug_launch_cap sets a process-wide upper bound on the blocks of ONE launch, so that
 * tests cross those chunk boundaries and stride trips at a few thousand rows; it returns the previous
 * bound (0: none), and blocks <= 0 removes the bound.  A bound above a site's own cap changes nothing
 * there.  It changes scheduling only, never results; it is read once per entry call, so set it while
 * no other thread is inside the library.  Not for production use. */
int64_t srg_debug_launch_cap(int64_t blocks);
/* The number of kernel launches issued through the chunk walk so far: monotonic, process-wide. */
int64_t srg_debug_chunk_launches(void);

#ifdef __cplusplus
}
#endif
#endif /* SRGNN_HIP_H_ */
