/*
 * redclust_hip.h — C ABI of libredclust_hip.so: the MI355X (gfx950) implementation of RedClust.jl's
 * per-iteration Gibbs label sweep and the observables computed from the same device-resident data.
 *
 * The reference (RedClust.jl v1.2.2, pure Julia) has no FFI seam on this path: sample_labels_Gibbs! is an
 * ordinary Julia function.  This header DEFINES the seam; each entry point cites the reference code it
 * replaces (path:line under the reference checkout).  The Julia-side binding (ccall stubs keeping
 * runsampler / MCMCData / MCMCOptionsList / MCMCResult unchanged) is shown in INTEGRATION.md and
 * julia/RedClustHIP.jl; the Python host (redclust.jl_amd/) binds the same symbols through ctypes.
 *
 * Conventions
 *   - every function returns int32_t: 0 = RC_OK, negative = error class; rc_last_error() gives the text.
 *     Nothing aborts and nothing throws across the boundary.
 *   - labels are Julia Int = int64_t, 1-based, in 1..n (src/types.jl:1,135); matrices are n×n Float64,
 *     column-major == row-major because MCMCData enforces exact symmetry (src/types.jl:149-151).
 *   - the caller owns every host buffer and keeps it alive for the duration of the call; the library owns
 *     all device memory behind rc_ctx.  One rc_ctx is not thread-safe; distinct contexts are independent.
 *   - uniforms: the m uniforms sample_logweights (src/utils.jl:4) draws for point i (0-based) of sweep t
 *     are Philox4x32-10(key = seed)(counter = (key, i, t_lo, t_hi)), key = the candidate cluster's label
 *     (1..n), 0 for the new-cluster candidate; u = (top 52 bits + 0.5) * 2^-52  (DESIGN.md "Uniform stream").
 */
#ifndef REDCLUST_HIP_H
#define REDCLUST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_OK 0
#define RC_ERR_ARG (-1)      /* bad argument (null pointer, n < 1, label outside 1..n, r <= 0, p outside (0,1)) */
#define RC_ERR_HIP (-2)      /* HIP runtime error, including "no device" */
#define RC_ERR_OOM (-3)      /* host or device allocation failed */
#define RC_ERR_DOMAIN (-4)   /* D not symmetric / not finite / non-positive off-diagonal entry (log D = -Inf) */
#define RC_ERR_STATE (-5)    /* call sequence error (params or state not set) */
#define RC_ERR_CAPACITY (-6) /* more clusters than the library holds (min(n, 32767)), or than a capacity fixed with RC_KCAP_FIXED */

typedef struct rc_ctx rc_ctx;

/* Fields read by the sweep at src/mcmc.jl:171-178 (δ1 δ2 α β ζ γ repulsion maxK) and by logprior at
 * src/mcmc.jl:65-68 (η σ u v); struct PriorHyperparamsList, src/types.jl:93-108. */
typedef struct rc_params {
    double delta1, delta2, alpha, beta, zeta, gamma;
    double eta, sigma, u, v;
    int64_t maxK;      /* 0 = unbounded */
    uint8_t repulsion; /* Julia Bool */
    uint8_t pad_[7];
} rc_params;

/* Counters of the last rc_gibbs_sweep (diagnostics; no reference counterpart). */
typedef struct rc_sweep_stats {
    int64_t n_changes; /* points whose label changed in the sweep */
    int64_t n_rounds;  /* resolve rounds (tentative scoring passes); between 1 and 1 + n_changes */
    int64_t K;         /* clusters after the sweep (state.K, src/mcmc.jl:254) */
} rc_sweep_stats;

/* MCMCData constructor, src/types.jl:145-157.  Copies the n×n matrix D to HBM once, checks symmetry
 * (types.jl:149-151) and derives logD = log.(D - Diagonal(D) + I) on the device (types.jl:155; diagonal 0,
 * D's own diagonal kept as stored) unless the caller passes its own logD (e.g. MCMCData.logD).
 * With logD_or_null == NULL and 64-bit storage the fixed-point logD is not stored at all: every consumer evaluates it
 * from the stored D with one shared table-based log (DESIGN.md "Derived logD"; results are exact integers either way,
 * the row reduction reads half the bytes).  rc_get_matrix(ctx, 1, ·) returns the values in use.  RC_STORED_LOG=1
 * forces the stored form.
 * storage_bits: 64 (int64 fixed point; the Float64 path) or 32 (int32 fixed point: every entry rounded to
 * 2^-30 of the largest magnitude, half the HBM traffic; all sums stay exact 64-bit integers and scores stay f64
 * — the counterpart of BASELINE config 5's Float32 storage, which the reference itself does not have).
 * kcap: INITIAL slot capacity (clusters the sweep kernel's tables hold).  It grows on demand — rc_set_state with more
 * clusters, a sweep or a split–merge proposal that needs one more slot: the tables are doubled, the sweep is resumed at the
 * point that needed the slot and the sweeps enqueued behind it are replayed; the chain is exactly the one a larger capacity
 * would have produced.  Up to 4096 slots the kernel's tables live in LDS (the fast path).  Beyond — the reference's clustsizes
 * has length n, src/types.jl:131-137, src/mcmc.jl:198-199 — the context becomes WIDE: tables in global memory, one row-sum
 * table corrected in place, the sweep point by point on one workgroup (tens to hundreds of ms per sweep; the same draws), up
 * to min(n, 32767) clusters (slot ids are 16-bit); more is RC_ERR_CAPACITY.  A wide context NARROWS again once its state is down
 * to 1024 clusters (a chain started from all singletons collapses within a sweep or two): rc_set_state, and rc_gibbs_sweep[_async]
 * between two sweeps (also those of rc_run_chain), re-install the labels with a capacity sized by the state — the same chain.
 * 0 = automatic: sized from the first state (twice
 * its cluster count, at least 128, on the fast path while the clusters fit it).  Small capacities are faster (the tables sit
 * beside more row-reduction blocks on a CU); rc_capacity_info reports the current one.
 * device_id: HIP device ordinal. */
int32_t rc_create(int64_t n, const double *D, const double *logD_or_null, int32_t storage_bits,
                  int32_t device_id, int64_t kcap, rc_ctx **out);
/* MCMCData(points) constructor, src/types.jl:159-162: D = pairwise(Euclidean(), makematrix(pnts), dims=2) is
 * computed on the device from the n×dim row-major points (the n×n matrix never exists on the host), then
 * everything proceeds as in rc_create.  SURVEY.md §8f-2. */
int32_t rc_create_from_points(int64_t n, int64_t dim, const double *points, int32_t storage_bits, int32_t device_id,
                              int64_t kcap, rc_ctx **out);

/* ---------------------------------------------------------------------------------------------------------------
 * Metrics from coordinates (DESIGN.md §8 "Metrics from coordinates").  The names are SciPy's and Distances.jl's.  There is no
 * Minkowski-p: pow is not correctly rounded on the device, so it could not be restated bit for bit.
 *
 * The arithmetic of a pair (y, x) is part of the contract: the coordinates k are walked in ascending order, every
 * accumulator starts at +0.0, every operation is one IEEE-754 binary64 operation rounded to nearest even, nothing is fused
 * unless written fma, nothing is reassociated and nothing is split across threads.
 *   EUCLIDEAN    t = y_k − x_k; acc = fma(t, t, acc); d = sqrt(acc)                       (what rc_predict_points always did)
 *   SQEUCLIDEAN  the same chain; d = acc
 *   CITYBLOCK    t = y_k − x_k; acc = acc + |t|; d = acc
 *   CHEBYSHEV    t = y_k − x_k; acc = max(acc, |t|); d = acc
 *   COSINE       per point, once: nn = fma(x_k, x_k, nn); norm = sqrt(nn).  Per pair: dot = fma(y_k, x_k, dot);
 *                s = norm_y·norm_x; c = dot / s; d = max(1 − c, 0)
 *   CORRELATION  COSINE on centred coordinates: per point sum = sum + x_k; mu = sum / (double)dim; x'_k = x_k − mu.
 *                Needs dim >= 2 (RC_ERR_ARG otherwise).
 * Each is symmetric in (y, x) bit for bit.  Note for the two angular metrics: the arithmetic above does not return 0 for
 * every point against itself or against an exact multiple — norm·norm may round an ulp or two off nn, and d is then 2^-53 or
 * 2^-52 instead of 0 (one coincident pair in four on random vectors); it never exceeds 2^-51 there.
 *
 * Bad pairs (where a call refuses them: rc_predict_points_metric; rc_pairwise refuses nothing): EUCLIDEAN keeps its rule on
 * the squared distance; for every other metric a pair is bad when d is 0, subnormal or not finite, and for COSINE /
 * CORRELATION also when s is 0, subnormal or not finite (a zero, or constant, vector) and when d <= 2^-51, the arithmetic's
 * zero by the note above — so that a coincident pair is refused whatever its coordinates.  A context
 * (rc_create_from_points_metric) refuses zero entries of its matrix as rc_create does, no more: two identical training
 * points under an angular metric pass there when their entry comes out 2^-53 or 2^-52. */
#define RC_METRIC_EUCLIDEAN 0
#define RC_METRIC_SQEUCLIDEAN 1
#define RC_METRIC_CITYBLOCK 2
#define RC_METRIC_CHEBYSHEV 3
#define RC_METRIC_COSINE 4
#define RC_METRIC_CORRELATION 5

/* The raw distances as doubles, in the arithmetic above.  new_points_or_null == NULL: out is the symmetric n×n matrix of
 * points (row-major n×dim) with a zero diagonal (q is ignored); one triangle is computed and mirrored, and n² doubles must fit
 * on the device (RC_ERR_OOM otherwise).  Otherwise out is q×n, new point (row of new_points, q×dim) against training point, by
 * the kernel of rc_predict_points_metric, the rows in chunks sized by the workspace (RC_PREDICT_WORKSPACE_KIB shrinks it).
 * Nothing about the values is refused: zero distances are legal here, and a zero vector under COSINE gives what the
 * arithmetic gives.  No context: errors through rc_last_error(NULL).  RC_ERR_ARG: a NULL points or out, n < 1 or n > 2^24,
 * q < 1 with new points, dim outside 1..2^20, an unknown metric, CORRELATION with dim < 2, a device that is not there.
 * RC_ERR_DOMAIN: a coordinate that is not finite.  kernel_ms (may be NULL): the kernels' time by device events. */
int32_t rc_pairwise(int32_t device, int32_t metric, int64_t n, int64_t dim, const double *points /* n×dim row-major */,
                    int64_t q, const double *new_points_or_null /* q×dim row-major */, double *out /* n×n or q×n */,
                    double *kernel_ms);

/* rc_create_from_points with D in the given metric, in the arithmetic above (one triangle computed, mirrored, zero
 * diagonal); everything after D is rc_create_from_points'.  RC_METRIC_EUCLIDEAN here is the direct-difference chain, not
 * rc_create_from_points' |a|² + |b|² − 2a·b: the context's matrix then agrees with the distances of rc_predict_points to the
 * same points.  The points are kept for the k-means entry points as before; k-means clusters the observations themselves
 * and stays Euclidean whatever the metric.  A zero off-diagonal entry fails with rc_create's RC_ERR_DOMAIN text.
 * RC_ERR_ARG besides rc_create_from_points': an unknown metric, CORRELATION with dim < 2. */
int32_t rc_create_from_points_metric(int64_t n, int64_t dim, const double *points, int32_t metric, int32_t storage_bits,
                                     int32_t device_id, int64_t kcap, rc_ctx **out);
/* The matrix the device actually holds (which = 0: D, 1: logD), as doubles: value = q·2^-e exactly. */
int32_t rc_get_matrix(rc_ctx *ctx, int32_t which, double *out_n_by_n);
/* Selected rows (0-based, caller's point order) of the same matrix: out is nrows×n row-major.  For sizes where the
 * n×n doubles of rc_get_matrix do not fit on the host (BASELINE config 5: 8 GiB). */
int32_t rc_get_matrix_rows(rc_ctx *ctx, int32_t which, const int64_t *rows, int64_t nrows, double *out);
int32_t rc_destroy(rc_ctx *ctx);

/* Last error text of ctx (or of the calling thread's last failed rc_create when ctx == NULL). */
const char *rc_last_error(const rc_ctx *ctx);

int32_t rc_set_params(rc_ctx *ctx, const rc_params *params);

/* MCMCState, src/types.jl:131-137: clustsizes and K are derived from the labels (types.jl:135-136). */
int32_t rc_set_state(rc_ctx *ctx, const int64_t *clusts /* n, 1-based */);
/* Any of the three outputs may be NULL.  With clusts == NULL nothing is copied from the device: sizes and K come
 * from the summary the sweep kernel leaves in host-mapped memory (the per-iteration need of sample_r!/sample_p!). */
int32_t rc_get_state(rc_ctx *ctx, int64_t *clusts /* n */, int64_t *clustsizes /* n, by label */, int64_t *K);

/* sample_labels_Gibbs!(data, state, params), src/mcmc.jl:158-256 — one full sequential sweep with the
 * r, p of the current iteration (mcmc.jl:169-170); mutates the device state exactly as the sequential loop
 * would under the uniform stream (seed, sweep_index).  Blocking. */
int32_t rc_gibbs_sweep(rc_ctx *ctx, double r, double p, uint64_t seed, uint64_t sweep_index);
int32_t rc_last_sweep_stats(rc_ctx *ctx, rc_sweep_stats *out);
/* Current slot capacity, its ceiling min(n, 32767) (beyond 4096 slots the context is wide: see rc_create), the number of growths so far and the resolver's batch capacity (each
 * pointer may be NULL).  Diagnostics; no reference counterpart. */
int32_t rc_capacity_info(rc_ctx *ctx, int64_t *kcap, int64_t *kcap_max, int64_t *n_grows, int64_t *batch_capacity);

/* Data flow of the sweep.  RC_MODE_FULL (default) recomputes the row-sum table S[k][i] = Σ_j D[i,j]·[c_j = k] from
 * the matrices in every sweep — what the reference does (src/mcmc.jl:206-214) and what the HBM roofline metric
 * is defined on.  RC_MODE_INCREMENTAL computes it once and then only corrects it for label changes; because the
 * sums are exact integers both modes give bit-identical results, and a sweep that changes no label reads no
 * matrix data at all.  Can be switched at any time. */
#define RC_MODE_FULL 0
#define RC_MODE_INCREMENTAL 1
int32_t rc_set_mode(rc_ctx *ctx, int32_t mode);

/* Non-blocking sweep for the stationary fast path and for benchmarking: enqueues one sweep on the
 * context's stream and returns; label changes are resolved on the device.  rc_synchronize() (or any
 * blocking call) waits for completion. */
int32_t rc_gibbs_sweep_async(rc_ctx *ctx, double r, double p, uint64_t seed, uint64_t sweep_index);
int32_t rc_synchronize(rc_ctx *ctx);

/* loglik(data, state, params), src/mcmc.jl:1-56. */
int32_t rc_loglik(rc_ctx *ctx, double *out);
/* logprior(state, params), src/mcmc.jl:58-78, with the given r, p. */
int32_t rc_logprior(rc_ctx *ctx, double r, double p, double *out);

/* Recording step of runsampler, src/mcmc.jl:546-553: canonical labels = sortlabels(state.clusts)
 * (src/utils.jl:69-74) written to canonical_out (nullable), and counts += adjacencymatrix(clusts)
 * (src/utils.jl:59-63), the running sum behind src/mcmc.jl:560. */
int32_t rc_record_sample(rc_ctx *ctx, int64_t *canonical_out /* n or NULL */);
/* posterior_coclustering = sum(adjacencymatrix.(result.clusts)) ./ numsamples, src/mcmc.jl:560. */
int32_t rc_cocluster(rc_ctx *ctx, double *out_n_by_n, int64_t numsamples);
/* Raw integer counts (exact), e.g. for cross-chain reduction on the host. */
int32_t rc_cocluster_counts(rc_ctx *ctx, uint32_t *out_n_by_n);
/* Device address and leading dimension (elements) of the uint32 count matrix, for a device-side
 * all-reduce across chains (RCCL through torch.distributed); valid until rc_destroy. */
int32_t rc_cocluster_device_buffer(rc_ctx *ctx, void **dev_ptr, int64_t *ld);
int32_t rc_cocluster_reset(rc_ctx *ctx);

/* ---- split–merge step -------------------------------------------------------------------
 * One proposal of the MH loop of sample_labels!, src/mcmc.jl:374-473 (chaperones, launch state, numGibbs
 * restricted scans sample_labels_Gibbs_restricted! src/mcmc.jl:259-354, split or merge bookkeeping, prior /
 * likelihood / proposal ratios, acceptance), restated as written including quirks Q2/Q3.  The
 * scalar scans run on the host on matrices borrowed with rc_attach_host_matrices (MCMCData.D and .logD; logD may
 * be NULL — the library then derives it); both log-likelihoods of mcmc.jl:462-464 come from the device.
 * Uniforms: Philox keyed (seed_lo, seed_hi ^ 0x4D485F52), counter (draw, mh_counter, iter_lo, iter_hi) — DESIGN.md.
 * On acceptance the device state becomes the proposed state.  The reference's `state = finalstate` (mcmc.jl:470)
 * only rebinds a local name (quirk Q1): a host loop that wants the reference's behaviour as written brackets the
 * iteration with rc_state_checkpoint / rc_state_restore and skips the Gibbs sweep after an acceptance. */
int32_t rc_attach_host_matrices(rc_ctx *ctx, const double *D, const double *logD_or_null);
int32_t rc_splitmerge(rc_ctx *ctx, double r, double p, int64_t numGibbs, uint64_t seed, uint64_t iter,
                      uint64_t mh_counter, uint8_t *accept_out, uint8_t *split_out);
int32_t rc_state_checkpoint(rc_ctx *ctx);
int32_t rc_state_restore(rc_ctx *ctx);

/* Introspection used by the parity tests: exact fixed-point row sums Σ_j D[i,j]·[c_j = label] of the
 * current state (the matsum(D,[i],clust_k) of src/mcmc.jl:210-213 before β is added), value = q·2^-e. */
int32_t rc_debug_rowsums(rc_ctx *ctx, int64_t label, int64_t *sumD_q /* n */, int64_t *sumL_q /* n */,
                         int32_t *eD, int32_t *eL);

/* Fixed-point row totals of the matrices as the caller gave them: totD_q[i] = Σ_j Dq[i,j], totL_q[i] = Σ_j Lq[i,j] (value =
 * q·2^-e, exponents from rc_debug_rowsums).  Computed by a plain per-row kernel that shares nothing with the row-reduction
 * kernels: Σ_labels rc_debug_rowsums(label)[i] must equal it (the full matsum(x) of src/utils.jl:18-24 row by row). */
int32_t rc_debug_rowtotals(rc_ctx *ctx, int64_t *totD_q /* n */, int64_t *totL_q /* n */);

/* The logarithms the sweep kernel scores candidates with, evaluated on the device for m caller-supplied arguments: which = 0
 * log(x) (x > 0, normal), 1 log1p(x) (x >= 0), 2 -log(-log(x)) (0 < x < 1: the Gumbel noise of src/utils.jl:4).  The reference
 * calls Julia's log / log1p (src/mcmc.jl:223-241); the kernel uses one table-driven routine of its own (<= 1.5 ulp on these
 * domains) — this entry lets the tests hold it against libm. */
int32_t rc_debug_flog(rc_ctx *ctx, int32_t which, const double *x, int64_t m, double *out /* m */);

/* Timing of the dominant kernel (row-bucket reduction) measured with HIP events on the stream it is launched
 * on: accumulated milliseconds and number of timed launches since the last reset.  enable: 0 = off, 1 = time
 * every launch, N > 1 = time every N-th launch, negative = just read the counters.  The two events of a timed
 * launch ride in its dispatch (hipExtLaunchKernelGGL) and report the kernel's own start and stop on that stream;
 * no marker packets are added around the kernel. */
int32_t rc_kernel_timing(rc_ctx *ctx, int32_t enable, double *bulk_ms_total, int64_t *bulk_launches);
/* What is subtracted from every timed launch: 0 (round 1 recorded marker pairs around the launch and subtracted
 * what such a pair reports around an empty kernel; kept so that the bench line can say so). */
int32_t rc_event_overhead_ms(rc_ctx *ctx, double *out);

/* Which row-reduction kernel the last enqueued sweep used — *which = 0: k_bulk (reads every entry of D and logD, any point
 * order), 1: one of the symmetric kernels (upper triangle only; chosen automatically when the points of a cluster are
 * contiguous in the internal point order, override with rc_set_bulk_kernel or RC_BULK_KERNEL=perm|sym|auto).  Which symmetric
 * kernel that is depends on the storage (and, for measurements, on RC_SYM_VARIANT): k_bulk_syml2 (64-bit storage with logD
 * derived, the default: wave-autonomous units, streams the 48-bit packed copy of D), k_bulk_sym (64-bit, logD stored:
 * block-tiled), k_bulk_sym32 (32-bit storage) —
 * rc_bulk_kernel_name says which.  *algorithmic_bytes = the matrix bytes that kernel has to read per launch (what bench.py's
 * roofline prices): every entry of the matrices it reads for k_bulk, the upper triangle incl. diagonal for the symmetric
 * ones, at 6 bytes per entry for the packed copy. */
int32_t rc_bulk_kernel_info(rc_ctx *ctx, int32_t *which, double *algorithmic_bytes);
/* The kernel's name as a profiler shows it (k_bulk_syml2<true, true>: logD derived, packed copy; k_bulk<long long, false>,
 * k_bulk_sym<false>, k_bulk_sym32 ...). */
const char *rc_bulk_kernel_name(rc_ctx *ctx);
/* k_bulk_syml2 with logD derived exists in two forms under that one name: 1 = this context's launches read the log table with
 * the exponent folded in (its entries span at most four binades and option "fold_log_table" is 1); 0 = they derive the exponent
 * per entry — a profiler shows those as k_bulk_syml2w — or the context does not derive logD.  Same integers either way. */
int32_t rc_log_table_folded(rc_ctx *ctx);
/* Force the kernel family: -1 automatic, 0 k_bulk (full read), 1 the symmetric kernel of this context (tests / measurements;
 * results are identical bit for bit). */
int32_t rc_set_bulk_kernel(rc_ctx *ctx, int32_t which);
/* Run-time options of one context.  Defaults come from the environment once, when the context is created (INTEGRATION.md
 * "Environment switches"); nothing reads the environment per sweep or per chain.
 *   "prune"          -1 automatic (default), 0 never, 1 always: candidates that cannot win skip their Gumbel noise (exact either way)
 *   "lds_point_cache" 1 (default) / 0: the sweep kernel keeps the internal indices and clusters of each workgroup's points in LDS
 *                    (possible while a workgroup owns at most 4 chunks of 32 points, i.e. n <= 128 x #CUs; larger problems and 0 read
 *                    them from global memory in every pass; same results)
 *   "chain_workers"  worker threads of rc_run_chain (0 = automatic: the host's cores shared by the chains of this process)
 *   "chain_depth"    iterations rc_run_chain keeps in flight (0 = automatic: 24)
 *   "chain_pipeline" 1 (default): the pipelined loop; 0: its synchronous form (the same chain bit for bit)
 *   "fold_log_table" 1 (default): a context that derives logD and whose entries span at most four binades runs the row reduction
 *                    that reads the exponent from its log table (k_bulk_syml2); 0: always the one that derives it per entry
 *                    (k_bulk_syml2w; same integers)
 *   "syml2_unit_rows" (tests) 0 (default): k_bulk_syml2's plan chooses the rows per work unit; 8..128, a multiple of 8: fixes
 *                    them and plans the unit lists again (the pipeline is drained first; same integers) — with 8-row units a
 *                    problem of n = 2560 has more units than resident waves, which the plan's own choice reaches from n ~ 14 000
 * No reference counterpart (the reference has no tuning knobs on this path). */
int32_t rc_set_option(rc_ctx *ctx, const char *name, int64_t value);
/* The plan of k_bulk_syml2's fast path (contexts with 64-bit storage): resident waves, fast work units, rows per unit and the
 * most units dealt to one wave.  Any pointer may be NULL.  No reference counterpart. */
int32_t rc_bulk_plan_info(rc_ctx *ctx, int32_t *waves, int32_t *fast_units, int32_t *unit_rows, int32_t *max_units_per_wave);
/* Internal point layout.  rc_set_state stores D and logD with the points of a cluster contiguous (a stable sort of
 * the caller's points by label), so that k_bulk_sym applies whatever order the caller's points come in; the sweep
 * still visits the points in the caller's order and every output is in the caller's order.  Label movement
 * fragments the layout; in automatic kernel mode the library re-lays the points out when the number of label runs
 * in internal order exceeds n/32 and a fresh layout would be below it again (at most once per 32 sweeps up to n/64 clusters, per
 * 128 sweeps — doubling when a layout does not last — up to n/36; the chain is bit-identical either way).  Returns the
 * number of layouts built so far and the current run count.  RC_NO_RELAYOUT=1 keeps the caller's order throughout. */
int32_t rc_layout_info(rc_ctx *ctx, int32_t *n_relayouts, int32_t *label_runs);

/* The within- / between-cluster split of the pairwise dissimilarities under the CURRENT labels, as fitprior forms it
 * for its Gamma fits (src/prior.jl:73-75: A = upper-triangle entries of pairs in one cluster, B = the rest;
 * src/prior.jl:96-110 consume |A|, sum(A), sum(log A) and the same of B).  From the K×K block sums of the row-sum
 * table: no pass over the n×n matrices. */
typedef struct rc_wb_stats {
    int64_t count_within, count_between;
    double sum_within, sumlog_within, sum_between, sumlog_between;
} rc_wb_stats;
int32_t rc_within_between(rc_ctx *ctx, rc_wb_stats *out);

/* kmedoids(D, k; maxiter, tol) of Clustering.jl with k-medoids++ seeding by costs, as fitprior (src/prior.jl:22-128) and
 * runsampler's default start (src/mcmc.jl:516-527) call it, on the context's fixed-point D in the caller's point order
 * (the algorithm as restated, its tie rules and the integer weighted draw).  Sums and comparisons are exact
 * integers, so the result is a pure function of (D, k, seed).  Uniforms: Philox keyed (seed_lo, seed_hi ^ 0x4B4D4544),
 * counter (step, k, 0, 0).  Converged when |totalcost - previous| < tol (units of D).  Works on any context (64- or 32-bit
 * storage, from D or from points, with or without a state) and leaves the chain state, the layout and the co-clustering
 * counts untouched.  RC_ERR_DOMAIN when a group becomes empty (a nonzero diagonal entry) or every seeding weight is zero. */
int32_t rc_kmedoids(rc_ctx *ctx, int64_t k, int64_t maxiter, double tol, uint64_t seed,
                    int64_t *assignments /* n, 1-based */, int64_t *medoids /* k, 1-based */, double *totalcost,
                    int64_t *iterations, uint8_t *converged);
/* rc_kmedoids for every k in kmin..kmax in one batched job (the per-k loop of fitprior, src/prior.jl:63-70): entry k - kmin
 * of each array (length kmax - kmin + 1) equals rc_kmedoids(k) with the same seed, bit for bit. */
int32_t rc_kmedoids_scan(rc_ctx *ctx, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                         double *totalcost, int64_t *iterations, uint8_t *converged);
/* The scan above plus, for every k, the within / between split of its final assignment (fitprior2's A_k and B_k,
 * src/prior.jl:211-217): split[k - kmin] equals what rc_within_between returns after rc_set_state with that assignment, bit
 * for bit, and totalcost / iterations / converged equal the plain scan's.  Exact integer sums over the pairs of every group
 * on the device; the chain state, the layout and the co-clustering counts stay untouched. */
int32_t rc_kmedoids_scan_split(rc_ctx *ctx, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                               double *totalcost, int64_t *iterations, uint8_t *converged,
                               rc_wb_stats *split /* kmax - kmin + 1 */);

/* kmeans(X, k; maxiter, tol) of Clustering.jl with k-means++ seeding, as fitprior / fitprior2 call it with algo = "k-means"
 * (src/prior.jl:64, :197), on the f64 points a context created by rc_create_from_points keeps (a context created from a
 * matrix: RC_ERR_STATE).  DESIGN.md §8 "k-means (built)" restates the algorithm and its fixed orders: squared distances summed
 * over ascending coordinates without fma, centres as ordered member sums and one division, the objective in one fixed tree,
 * integer weighted draws — so a run is a pure function of (points, k, seed | init), reproducible bit for bit on the host.
 * Uniforms: Philox keyed (seed_lo, seed_hi ^ 0x4B4D4E53), counter (draw, k, 0, 0); draw 0 is the uniform first seed, the
 * repicks of empty groups continue the count (from 0 when init is given).  init_or_null: k distinct 1-based point indices
 * whose points are the starting centres (RC_ERR_ARG for an index outside 1..n or a repeated one).  Converged as Clustering.jl:
 * objective change <= tol and (k == 1 or |change| < tol).  maxiter = 0 returns the initial assignment.  Leaves the chain
 * state, the layout and the co-clustering counts untouched.  RC_ERR_DOMAIN: k outside 1..n (kmax < kmin), maxiter outside
 * 0..2^24, tol negative or NaN, or every weight of a draw zero (fewer distinct points than k; Clustering.jl's wsample fails
 * there).  Non-finite points never get this far: rc_create_from_points refuses them. */
int32_t rc_kmeans(rc_ctx *ctx, int64_t k, int64_t maxiter, double tol, uint64_t seed, const int64_t *init_or_null,
                  int64_t *assignments /* n, 1-based */, double *centers /* k×dim row-major */, double *costs /* n */,
                  int64_t *counts /* k */, double *totalcost, int64_t *iterations, uint8_t *converged);
/* rc_kmeans for every k in kmin..kmax in one batched job: entry k - kmin of each array equals rc_kmeans(k) with the same
 * seed, bit for bit.  slots_per_chunk: runs per device pass, 0 = automatic (a workspace of at most 512 MiB; RC_ERR_OOM when
 * one run alone exceeds it); the results do not depend on it. */
int32_t rc_kmeans_scan(rc_ctx *ctx, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                       int64_t slots_per_chunk /* 0 = automatic */, double *totalcost, int64_t *iterations, uint8_t *converged);
/* The scan above plus, for every k, the within / between split of the context's D under that k's final assignment:
 * split[k - kmin] equals rc_set_state(assignments_k) + rc_within_between, bit for bit (as rc_kmedoids_scan_split). */
int32_t rc_kmeans_scan_split(rc_ctx *ctx, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                             int64_t slots_per_chunk /* 0 = automatic */, double *totalcost, int64_t *iterations,
                             uint8_t *converged, rc_wb_stats *split /* kmax - kmin + 1 */);

/* sampleK (src/prior.jl:316-338) for m samples whose r[i] ~ Gamma(eta, 1/sigma) and p[i] ~ Beta(u, v) the caller has
 * drawn: the Gumbel-max draw over the n log-probabilities of every sample on the device.  Uniforms: Philox keyed
 * (seed_lo, seed_hi ^ 0x534D504B), counter (K, i_lo, i_hi, 0); sample i is a pure function of (n, r[i], p[i], seed, i).
 * A sample with no score above -inf (p = 1) returns K = 1.  n in 1..2^30.  K_out: m values in 1..n.  kernel_ms (may be
 * NULL): device time of the launches.  No context: errors are read with a NULL context. */
int32_t rc_sample_k(int32_t device, int64_t n, int64_t m, const double *r, const double *p, uint64_t seed,
                    int64_t *K_out /* m, 1-based */, double *kernel_ms);

/* generatemixture's oracle co-clustering matrix (src/utils.jl:130-143) for the caller's weight draws:
 * out = (1/T)·Σ_t P_t P_tᵀ with P_t[i][j] = softmax_j(log w_tj + radius·x_ij/σ²), j < K (the centres are radius·e_j;
 * every other factor of the pdfs cancels).  f64 MFMA product on the device; every entry is summed in one fixed order
 * (ascending t, then j), so the result does not depend on iters_per_chunk, is the same run to run and is exactly
 * symmetric.  n in 1..2^16 (the device holds the n² sum), K in 1..dim, radius > 0, sigma > 0,
 * numiters >= 1: RC_ERR_ARG otherwise.  RC_ERR_DOMAIN for a non-finite point or radius·x/σ², or a weight row that is
 * not finite, has a negative entry or no positive one (rows need not sum to 1).  iters_per_chunk: iterations per
 * device pass, 0 = automatic (a workspace of about 1 GiB).  kernel_ms (may be NULL): device time.  No context: errors
 * are read with a NULL context. */
int32_t rc_oracle_coclustering(int32_t device, int64_t n, int64_t dim, const double *points /* n×dim row-major */,
                               int64_t K, double radius, double sigma, int64_t numiters,
                               const double *weights /* numiters×K */, int64_t iters_per_chunk /* 0 = automatic */,
                               double *out /* n×n */, double *kernel_ms /* may be NULL */);

/* ---------------------------------------------------------------------------------------------------------------
 * The iteration loop of runsampler (src/mcmc.jl:533-556) as native host code: per iteration sample_r!, sample_p!
 * (src/mcmc.jl:80-155, on the build's counter-based scalar stream — DESIGN.md), sample_labels! (numMH split–merge
 * proposals, then the Gibbs sweep; src/mcmc.jl:356-479) and the recording rule (src/mcmc.jl:546-553).  Recorded
 * samples also enter the device co-clustering counts (read them with rc_cocluster afterwards).
 * ------------------------------------------------------------------------------------------------------------- */
#define RC_SM_AS_WRITTEN 0 /* split–merge exactly as the reference executes it (an accepted
                            * proposal is discarded together with that iteration's Gibbs scan) */
#define RC_SM_INTENDED 1   /* accepted proposals are kept and swept */

typedef struct rc_chain_options {
    int64_t numiters, burnin, thin; /* MCMCOptionsList (src/types.jl:3-43) */
    int64_t numGibbs, numMH;
    int32_t splitmerge_mode;        /* RC_SM_* */
    int32_t pad_;
    uint64_t seed;                  /* keys the label, split–merge and scalar streams */
    uint64_t first_iter;            /* stream index of the first iteration (0 for a fresh chain; continue with numiters) */
    double r0, p0;                  /* MCMCState.r / .p at the start */
    double proposalsd_r;            /* PriorHyperparamsList.proposalsd_r (src/types.jl:102) */
    const double *r_trace, *p_trace;/* both NULL: free-running; else numiters forced values (parity tests) */
    int64_t max_samples;            /* capacity of the per-sample output arrays */
} rc_chain_options;

typedef struct rc_chain_outputs {
    /* per recorded sample (capacity max_samples; each pointer may be NULL) — MCMCResult fields, src/types.jl:193-248 */
    int64_t *clusts;                /* max_samples × n, sortlabels'd (src/mcmc.jl:547) */
    int64_t *K;
    double *r, *p, *loglik, *logposterior;
    /* per iteration (may be NULL) */
    uint8_t *r_acceptances;         /* numiters */
    uint8_t *splitmerge_acceptances, *splitmerge_splits; /* numiters × numMH */
    double *r_all, *p_all;          /* numiters: the r and p every iteration used */
    /* scalars written on return */
    int64_t num_samples;
    double runtime_s;               /* wall time of the loop (MCMCResult.runtime, src/mcmc.jl:586) */
    double r_final, p_final;
} rc_chain_outputs;

int32_t rc_run_chain(rc_ctx *ctx, const rc_chain_options *opt, rc_chain_outputs *out);
/* Counters of the last rc_run_chain on this context (each pointer may be NULL): rollbacks of the speculative split–merge
 * pipeline (an accepted proposal voids the iterations launched behind it), split proposals evaluated off the live state,
 * host worker threads used, capacity growths during the run.  Diagnostics; no reference counterpart. */
int32_t rc_chain_stats(rc_ctx *ctx, int64_t *rollbacks, int64_t *split_evals, int64_t *workers, int64_t *grows);

/* ---------------------------------------------------------------------------------------------------------------
 * Chain-parallel execution: independent chains, one per GPU; the single exchange step is the SUM
 * all-reduce of the n×n uint32 co-clustering counts (and of the numbers of recorded samples) over RCCL.  The reference
 * has no multi-chain driver (runsampler, /root/reference/src/mcmc.jl:501-590, is one chain); the merged estimate is
 * Σ_chains counts / Σ_chains numsamples — what mcmc.jl:560 forms for one chain.
 * ------------------------------------------------------------------------------------------------------------- */
#define RC_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */
typedef struct rc_comm rc_comm;

/* Rank 0 of a multi-process job calls this and sends the bytes to the other processes (MPI, a TCP store, a file ...). */
int32_t rc_comm_unique_id(uint8_t *id_out /* RC_COMM_ID_BYTES */);

/* A communicator over world_size chains; this process owns chains rank_offset .. rank_offset + n_local - 1, one per
 * entry of device_ids (distinct devices: one chain per GPU).  unique_id_or_null == NULL: all chains live in this
 * process (rank_offset = 0, world_size = n_local; ncclCommInitAll).  Collective over all participating processes. */
int32_t rc_comm_create(int32_t n_local, const int32_t *device_ids, int32_t rank_offset, int32_t world_size,
                       const uint8_t *unique_id_or_null, rc_comm **out);
int32_t rc_comm_destroy(rc_comm *comm);

/* In-place SUM all-reduce of the co-clustering counts of the n_local contexts (ctxs[i] on device_ids[i]) over all
 * chains, and of their numbers of recorded samples.  Afterwards every context holds the merged counts:
 * rc_cocluster(ctx, out, *total_samples) is the merged posterior co-clustering matrix.  elapsed_ms may be NULL. */
int32_t rc_comm_allreduce_counts(rc_comm *comm, rc_ctx *const *ctxs, const int64_t *num_samples /* n_local */,
                                 int64_t *total_samples, double *elapsed_ms);

typedef struct rc_chains_input {
    int64_t n;
    const double *D;             /* n×n, or NULL when points are given */
    const double *logD_or_null;  /* as rc_create */
    const double *points;        /* n×dim (rc_create_from_points: Euclidean — the layout is ABI and carries no metric; hand
                                    data in another metric over as D), used when D == NULL */
    int64_t dim;
    int32_t storage_bits;        /* 64 or 32 */
    int32_t pad_;
    int64_t kcap;                /* initial slot capacity as rc_create, 0 = automatic */
    const rc_params *params;
    const int64_t *init_clusts;  /* n labels: every chain starts from them (MCMCState.clusts) */
} rc_chains_input;

/* n_chains chains in this process: one host thread and one context per device runs rc_run_chain with seed
 * opt->seed + chain index (outs[chain] as for rc_run_chain), then the counts are merged over RCCL.
 * posterior_coclustering (n×n, may be NULL): Σ counts / Σ numsamples.  total_samples, allreduce_ms may be NULL. */
int32_t rc_run_chains(int32_t n_chains, const int32_t *device_ids, const rc_chains_input *in, const rc_chain_options *opt,
                      rc_chain_outputs *outs /* n_chains */, double *posterior_coclustering, int64_t *total_samples,
                      double *allreduce_ms);

/* Measured streaming-read ceiling of a device in GB/s (SURVEY.md §8d asks for the roofline fraction against it as well as
 * against the nominal 8 TB/s): `mib` MiB — use far more than the 256 MiB Infinity Cache — read once per launch with the access
 * pattern of the row reductions, best of `reps` launches.  No context needed. */
int32_t rc_measure_read_ceiling(int32_t device, int64_t mib, int32_t reps, double *gbps_out);

/* One sample_r + sample_p pair exactly as rc_run_chain draws them (tests; host only, no GPU needed).  sizes: the K
 * non-empty cluster sizes in ascending label order. */
int32_t rc_scalar_updates(uint64_t seed, uint64_t iter, double r, double p, const int64_t *sizes, int64_t K, int64_t n,
                          double eta, double sigma, double proposalsd_r, double u, double v, double *r_out,
                          double *p_out, uint8_t *accept_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Point estimation — the step after the sampler.  Stand-alone entry points (no rc_ctx): they
 * take host label vectors as MCMCResult.clusts holds them; errors are read with rc_last_error(NULL).
 * ------------------------------------------------------------------------------------------------------------- */

/* loss specifiers of getpointestimate(method = "MPEL") (src/pointestimate.jl:38-47) */
#define RC_LOSS_BINDER 0 /* "binder": randindex(x, y)[3] */
#define RC_LOSS_OMARI 1  /* "omARI":  1 - randindex(x, y)[1] */
#define RC_LOSS_VI 2     /* "VI":     varinfo(x, y) */
#define RC_LOSS_ID 3     /* "ID":     infodist(x, y; normalised = false) */

/* The MPEL search of getpointestimate (src/pointestimate.jl:49-58): lossmatrix[i][j] = loss(clusts[i], clusts[j])
 * for every pair of the m samples (computed for i < j and mirrored, zero diagonal), its column sums and the index
 * (0-based) of the first minimal one.  samples: m×n row-major (sample s = samples[s*n ..]), labels in 1..n.
 * lossmatrix (m×m), colsum (m), argmin and kernel_ms (device time of the pair kernel) may each be NULL. */
int32_t rc_loss_matrix(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t loss,
                       double *lossmatrix, double *colsum, int64_t *argmin, double *kernel_ms);

/* Everything evaluateclustering (src/summaries.jl:12-23), binderloss and infodist (src/pointestimate.jl:68-99)
 * derive from a pair of labelings: Clustering.jl's randindex 4-tuple, mutualinfo (normed = false / true), varinfo,
 * the two entropies and the information distance (plain / normalised by max entropy as infodist does). */
typedef struct rc_pair_measures_t {
    double ari, ri, mirkin, hubert;
    double mi, nmi, vi;
    double ha, hb;
    double id, nid;
} rc_pair_measures_t;
int32_t rc_pair_measures(int32_t device, const int64_t *a, const int64_t *b, int64_t n, rc_pair_measures_t *out);

/* ---------------------------------------------------------------------------------------------------------------
 * Point-estimate search: a greedy search over ALL partitions for the clustering of minimum expected loss under the
 * posterior co-clustering counts — what the reference's docs/src/index.md "Point estimation" sends its users to R's SALSO
 * for; the MPEL search above only looks at the clusterings the chain visited.  DESIGN.md §8 "Point-estimate search".
 *
 * counts: n×n uint32, symmetric, diagonal = m (the number of samples), no entry above m.  Criterion of a labelling c:
 *   RC_PSM_BINDER  num = Σ_{i<j} C_ij + Σ_{i<j, c_i=c_j} (m − 2·C_ij), loss = num / (m·n(n−1)/2) (0 for n = 1): the posterior
 *                  mean of binderloss(c, sample; normalised = true), src/pointestimate.jl:68-76.  Exact integers.
 *   RC_PSM_VILB    Wade & Ghahramani's lower bound of the expected VI without its partition-independent constant:
 *                  f = Σ_i [log n_{c_i} − 2·log T_i], T_i = Σ_{j: c_j=c_i} C_ij (C_ii included), loss = f/n + 2·log m.
 * A run: starting labels (0 = not yet allocated, else 1..n: the slots), a point order (a permutation of 1..n), maxK (0 = no
 * cap) and maxsweeps.  A sweep visits the points in that order: the point is taken out of its cluster, every non-empty
 * cluster and — while the cluster count is below maxK — a new one are scored by the change of the criterion, and the
 * point goes to the minimum.  Equal scores: the point's own slot first (it does not move), then the lowest slot; a new
 * cluster takes the slot the point just emptied, else the lowest free one.  A point counts as moved when the partition
 * changed (an unallocated point always).  The run ends after a sweep without a move (converged) or after maxsweeps.
 * From all-zero labels the first sweep is a sequential allocation, the later ones improve it.
 * One launch, one 1024-thread workgroup per run with its state in LDS: n <= 8192 and m·n < 2^31, RC_ERR_CAPACITY beyond.
 * Binder runs are exact integers; VI sums its log terms in fixed point (2^-40 per term, integer atomics): both are
 * pure functions of their arguments, bit for bit.  labels_out: sortlabels'd (src/utils.jl:69-74).  best: the first run
 * of minimal loss (0-based).  kernel_ms (may be NULL): device time of the search kernel.
 * RC_ERR_ARG: a NULL pointer, m, n or nruns < 1, maxsweeps < 1, maxK < 0, an unknown loss, a label outside 0..n, an
 * order that is not a permutation, counts that are asymmetric, exceed m or whose diagonal is not m, a run that starts
 * with more than a non-zero maxK clusters.
 * ------------------------------------------------------------------------------------------------------------- */
#define RC_PSM_BINDER 0
#define RC_PSM_VILB 1
typedef struct rc_psm_run_t {
    double loss;
    int64_t loss_num; /* Binder numerator, 0 for VI */
    int32_t sweeps, converged;
    int64_t moves;
    int32_t K;
} rc_psm_run_t;

/* counts: host n×n uint32; runs_out: nruns rc_psm_run_t.  Both are untyped so that hosts binding through a plain FFI
 * (julia/RedClustHIP.jl) pass their buffers as they are.  No context: errors are read with a NULL context. */
int32_t rc_psm_search(int32_t device, const void *counts /* uint32_t n×n */, int64_t m, int64_t n, int32_t loss,
                      int32_t nruns, const int64_t *init /* nruns×n, 0 = unallocated */, const int32_t *order /* nruns×n, 1-based */,
                      int32_t maxK, int32_t maxsweeps, int64_t *labels_out /* nruns×n */, void *runs_out /* rc_psm_run_t[nruns] */,
                      int32_t *best, double *kernel_ms);
/* The same search on the context's own device count matrix (what rc_record_sample and rc_run_chain accumulate), read in
 * place: no copy.  Equal to the stand-alone entry on rc_cocluster_counts, bit for bit.  Leaves the chain state, the
 * layout and the counts untouched.  RC_ERR_STATE when no sample has been recorded. */
int32_t rc_psm_search_ctx(rc_ctx *ctx, int64_t numsamples, int32_t loss, int32_t nruns, const int64_t *init,
                          const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                          rc_psm_run_t *runs_out, int32_t *best, double *kernel_ms);

/* Counts from samples that are already there (a stored result, several merged chains, another sampler's draws), built on
 * the device: counts[i][j] = #{s : samples[s][i] == samples[s][j]} — exact, symmetric, diagonal m; what rc_record_sample
 * accumulates for a live chain.  samples: host m×n int64 row-major, labels 1..n.  One kernel computes every count once from
 * zero in registers and stores it once (DESIGN.md §8 "Counts from samples"); kernel_ms (may be NULL) is its device time.
 * rc_samples_counts copies the result into the caller's dense n×n buffer.  Capacity: n <= 32767 (labels are narrowed to 16
 * bits beside two pad values) and m < 2^31, RC_ERR_CAPACITY beyond.  RC_ERR_ARG: a NULL pointer, m < 1, n < 1, a device that
 * is not there, a label outside 1..n (the message names the sample and the position). */
int32_t rc_samples_counts(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n,
                          void *counts_out /* uint32_t n×n */, double *kernel_ms);
/* rc_psm_search on those counts without a host copy of them: they are built in device memory as rc_psm_search stages its
 * copy and searched there; equal to rc_psm_search on rc_samples_counts' matrix, bit for bit.  Arguments, errors and capacity
 * (n <= 8192, m·n < 2^31, checked before any device work) as rc_psm_search; counts_ms (may be NULL): device time of the
 * counts kernel, kernel_ms: of the search kernel. */
int32_t rc_psm_search_samples(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n, int32_t loss,
                              int32_t nruns, const int64_t *init /* nruns×n, 0 = unallocated */, const int32_t *order /* nruns×n, 1-based */,
                              int32_t maxK, int32_t maxsweeps, int64_t *labels_out /* nruns×n */, void *runs_out /* rc_psm_run_t[nruns] */,
                              int32_t *best, double *kernel_ms, double *counts_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * PEAR search: the same greedy search over ALL partitions for the clustering of maximum posterior expected adjusted Rand
 * index in Fritsch & Ickstadt's form (mcclust's pear / maxpear, SALSO's omARI.approx) under the counts — the adjusted Rand
 * index with the sample's pair indicators replaced by their posterior means C_ij/m.  DESIGN.md §8 "PEAR search".
 *
 * With T = n(n−1)/2, P = Σ_{i<j} C_ij and, for a labelling c (0 = unallocated counts as a singleton),
 * X = Σ_{i<j, c_i=c_j≠0} C_ij and A = Σ_k n_k(n_k−1)/2:
 *   PEAR(c) = num/den,  num = 2·(T·X − A·P),  den = T·(m·A + P) − 2·A·P >= 0;  0 (num = 0, den = 1) where den = 0.
 * A run, its arguments, the tie rules (own slot, then the lowest slot; the new cluster with the priority of the slot it
 * would take), maxK, maxsweeps, the moved rule and labels_out are rc_psm_search's; the point goes to the MAXIMUM of the
 * fraction of (X₀ + S_ik, A₀ + n_k) over the clusters k and (X₀, A₀) for a new one, X₀, A₀ the state without the point.
 * Fractions are compared exactly, a/b > c/d ⇔ a·d > c·b in signed 128 bits, so every accepted move raises PEAR strictly
 * and a run is a pure integer function of its arguments.  num and den of a run are recomputed from the matrix at its end.
 * best: the first run of maximal fraction (0-based), by the exact comparison.
 * Capacity (RC_ERR_CAPACITY beyond, before any device work): n <= 8192, m·n < 2^31 and m·T² < 2^62 (m <= 4097 at n = 8192),
 * which keeps |num| and den below 2^63.  RC_ERR_ARG as rc_psm_search, in its order (there is no loss specifier).
 * The _samples and _ctx forms are to this entry what rc_psm_search_samples and rc_psm_search_ctx are to rc_psm_search: equal
 * to it on rc_samples_counts' / rc_cocluster_counts' matrix bit for bit; the context's state, layout and counts stay untouched.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rc_pear_run_t {
    double pear; /* num / den */
    int64_t num, den;
    int32_t sweeps, converged;
    int64_t moves;
    int32_t K;
} rc_pear_run_t;
int32_t rc_pear_search(int32_t device, const void *counts /* uint32_t n×n */, int64_t m, int64_t n, int32_t nruns,
                       const int64_t *init /* nruns×n, 0 = unallocated */, const int32_t *order /* nruns×n, 1-based */, int32_t maxK,
                       int32_t maxsweeps, int64_t *labels_out /* nruns×n */, void *runs_out /* rc_pear_run_t[nruns] */, int32_t *best,
                       double *kernel_ms);
int32_t rc_pear_search_ctx(rc_ctx *ctx, int64_t numsamples, int32_t nruns, const int64_t *init, const int32_t *order, int32_t maxK,
                           int32_t maxsweeps, int64_t *labels_out, rc_pear_run_t *runs_out, int32_t *best, double *kernel_ms);
int32_t rc_pear_search_samples(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n, int32_t nruns,
                               const int64_t *init /* nruns×n, 0 = unallocated */, const int32_t *order /* nruns×n, 1-based */,
                               int32_t maxK, int32_t maxsweeps, int64_t *labels_out /* nruns×n */, void *runs_out /* rc_pear_run_t[nruns] */,
                               int32_t *best, double *kernel_ms, double *counts_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Exact expected-VI search: the same greedy search (one run = starting labels, a point order, maxsweeps; the same scoring
 * of every non-empty cluster and a new one, the same tie rules) for the posterior expected Variation of Information itself
 * — the mean over the m samples of VI(c, sample), SALSO's "VI" — instead of RC_PSM_VILB's lower bound.  It needs the
 * samples, not only their pairwise counts.  DESIGN.md §8 "Exact expected VI search".
 *
 * Fixed point.  phi(x) = x·log x, g(x) = phi(x+1) − phi(x).  rc_vi_gtable writes Gq[x] = llrint(g(x)·2^32), x = 0..n−1
 * (Gq[0] = 0; g(x) = log(x+1) + x·log1p(1/x) for x >= 1); Phiq(x) = Σ_{y<x} Gq[y].  The search minimises the integer
 *   Q(c) = m·Σ_k Phiq(n_k) − 2·Σ_s Σ_{k,l} Phiq(N^s_kl),   N^s_kl = #{j : c_j = k, sample_s[j] = l},
 * and a move of point i into cluster k changes Q by exactly m·Gq[n_k] − 2·Σ_s Gq[N^s[l_s(i)][k]] (0 for a new cluster), so
 * a run is a pure integer function of its arguments.  Per run: loss_num = Q, loss = (Q + Σ_s Σ_l Phiq(n^s_l)) / (2^32·n·m),
 * the expected VI in nats (within 2·2^-32 of the f64 value); sweeps, converged, moves, K as rc_psm_search.
 *
 * Differences from rc_psm_search: the slot cap is always positive — Kcap = maxK, or with maxK = 0 the largest cluster
 * count among the samples — and starting labels are compacted to slots 1..K0 by first appearance before the run.
 * samples: host m×n int64, labels 1..n.  Capacity (RC_ERR_CAPACITY beyond, checked before the samples are read where
 * possible): n <= 8192, m·n <= 2^26, min(Kcap, n) <= 1024, nruns·m·Lmax·Kcap4·2 bytes of contingency tables <= 4 GiB
 * (Lmax = largest cluster count among the samples, Kcap4 = Kcap rounded up to a multiple of 4).
 * RC_ERR_ARG: a NULL pointer, m, n or nruns < 1, maxsweeps < 1, maxK < 0, a sample label outside 1..n, a starting label
 * outside 0..n, an order that is not a permutation, a run that starts with more than Kcap clusters.
 * best: the first run of minimal loss_num (0-based).  runs_out is untyped for the same reason as rc_psm_search's.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_vi_gtable(int64_t n, int64_t *out /* n */);
int32_t rc_vi_search(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n, int32_t nruns,
                     const int64_t *init /* nruns×n, 0 = unallocated */, const int32_t *order /* nruns×n, 1-based */,
                     int32_t maxK, int32_t maxsweeps, int64_t *labels_out /* nruns×n */, void *runs_out /* rc_psm_run_t[nruns] */,
                     int32_t *best, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Exact expected-ID search: rc_vi_search's search — the same runs, slot cap, compaction of the start, tie rules, tables and
 * capacity — for the posterior expected information distance, the mean over the m samples of
 * infodist(c, sample; normalised = false) = max(H(c), H(sample)) − I(c, sample) (src/pointestimate.jl:89-99; the `id` of
 * evaluateclustering, whose `nid` is id / log n, so the same partition minimises both).  DESIGN.md §8 "Exact expected ID search".
 *
 * With rc_vi_gtable's Gq and Phiq:  Aq(c) = Σ_k Phiq(n_k),  Bq_s = Σ_l Phiq(n^s_l), and the search minimises the integer
 *   Q_ID(c) = Σ_s max(Aq(c), Bq_s) − Σ_s Σ_{k,l} Phiq(N^s_kl).
 * With point i out (Aq becomes A0), putting it into a cluster of n_k members changes Q_ID by exactly
 *   F(A0 + Gq[n_k]) − F(A0) − Σ_s Gq[N^s[l_s(i)][k]],   F(x) = Σ_s max(x, Bq_s)   (0 for a new cluster),
 * so a run is a pure integer function of its arguments.  Per run: loss_num = Q_ID, loss = Q_ID / (2^32·n·m), the expected
 * ID in nats (within 2^-32 of the f64 value).  The sorted Bq_s and their prefix sums (16·(m+1) bytes) sit in the workgroup's LDS
 * where they fit beside rc_vi_search's state, else in global memory — the same integers either way; RC_ID_TABLE_GLOBAL=1 in the
 * environment (read at every call) forces the latter, for tests.
 * Arguments, RC_ERR_ARG and RC_ERR_CAPACITY (n <= 8192, m·n <= 2^26, slot cap <= 1024, the table budget) as rc_vi_search.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_id_search(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n, int32_t nruns,
                     const int64_t *init /* nruns×n, 0 = unallocated */, const int32_t *order /* nruns×n, 1-based */,
                     int32_t maxK, int32_t maxsweeps, int64_t *labels_out /* nruns×n */, void *runs_out /* rc_psm_run_t[nruns] */,
                     int32_t *best, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Grouped exact expected-VI search: many rc_vi_search searches over disjoint subsets of one sample set in one launch — the
 * update step of the several-partition summary (DESIGN.md §8 "Several-partition summary").  group[s] in 0..ngroups−1 names the
 * group of sample s, −1 leaves it out; run r searches the group run_group[r].
 *
 * Contract: run r — labels, loss_num, loss, sweeps, converged, moves, K — is bit for bit what rc_vi_search returns for the same
 * init row, order row, maxK and maxsweeps on the sub-array samples[group == run_group[r]] (rows in their order).  So the factor m
 * of the criterion, the constant and the divisor of loss are the group's, and with maxK = 0 a run's slot cap is the largest
 * cluster count among its own group's samples.  Nothing else is defined here.
 * best[g]: the first run of minimal loss_num among the runs of group g (0-based), −1 for a group no run searches.
 *
 * Checked before any device work, in this order.  RC_ERR_ARG: a NULL pointer; m, n or nruns < 1; maxsweeps < 1 or maxK < 0;
 * ngroups < 1.  RC_ERR_CAPACITY: n > 8192; m·n >= 2^31.  RC_ERR_ARG: a group id outside −1..ngroups−1; a run_group outside
 * 0..ngroups−1 or naming a group without samples.  RC_ERR_CAPACITY: a group with m_g·n > 2^26.  RC_ERR_ARG: a sample label
 * outside 1..n (every sample, grouped or not).  RC_ERR_CAPACITY: a searched group's slot cap min(Kcap_g, n) > 1024; the table
 * budget, below.  Then run by run, RC_ERR_ARG: a starting label outside 0..n, a start with more clusters than its group's cap,
 * an order that is not a permutation.
 * Table budget: run r keeps m_g × Lmax_g × Kcap4 cells of 2 bytes (g = run_group[r], Lmax_g the largest cluster count among
 * group g's samples, Kcap4 the LARGEST slot cap of any searched group rounded up to a multiple of 4: the thread geometry is
 * the launch's); the sum over the runs must not exceed rc_vi_search's 4 GiB.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_vi_search_groups(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n,
                            const int32_t *group /* m: 0..ngroups-1, or -1 = in no group */, int32_t ngroups,
                            int32_t nruns, const int32_t *run_group /* nruns: the group each run searches */,
                            const int64_t *init /* nruns×n, 0 = unallocated */, const int32_t *order /* nruns×n, 1-based */,
                            int32_t maxK, int32_t maxsweeps, int64_t *labels_out /* nruns×n */,
                            void *runs_out /* rc_psm_run_t[nruns] */,
                            int32_t *best /* ngroups: first run of minimal loss_num within the group, -1 = no run */,
                            double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Hierarchical point estimates: agglomerative clustering of the co-clustering counts (Medvedovic's method; mcclust's
 * minbinder and mcclust.ext's minVI with method = "avg" / "comp"), the whole dendrogram in one launch, and the expected
 * loss of given labellings on the device.  DESIGN.md §8 "Hierarchical point estimates".
 *
 * counts, m, n, capacity (n <= 8192, m·n < 2^31: RC_ERR_CAPACITY beyond, before any device work) and the checks of the
 * counts (RC_ERR_ARG) as in the point-estimate search above.  Clusters are named by their smallest member (1-based).  Per
 * pair of active clusters a < b: S_ab = Σ_{i∈a, j∈b} C_ij and M_ab = the minimum (complete) or maximum (single) of C_ij over
 * the pair.  Similarity, larger is closer:  average S_ab / (|a|·|b|), compared exactly by cross-multiplication in 128 bits;
 * complete and single M_ab.  A step merges the pair of largest similarity — ties: the smallest a, then the smallest b — b
 * into a: S_ac += S_bc and M_ac = min / max(M_ac, M_bc) for every other active c, |a| += |b|.  n − 1 steps; pairs of
 * similarity 0 merge too, at the end.  No floating point: a run is a pure integer function of (counts, m, linkage).
 * merges_out[t − 1], t = 1..n−1: a, b, the new size of a, S_ab and M_ab (0 for average) of step t.
 * binder_num[t], t = 0..n−1: RC_PSM_BINDER's num of the partition after t merges (K = n − t clusters):
 *   binder_num[0] = Σ_{i<j} C_ij,  binder_num[t] = binder_num[t−1] + |a|·|b|·m − 2·S_ab.
 * vilb (may be NULL with maxcut = 0): vilb[K − 1], K = 1..maxcut <= n, is RC_PSM_VILB's loss of the cut with K clusters,
 * evaluated like the expected-loss entry points below on labellings the host derives from the merges.
 * kernel_ms (may be NULL): device time of the call's kernels.  RC_ERR_ARG also: a NULL pointer, an unknown linkage, maxcut
 * outside 0..n.
 * ------------------------------------------------------------------------------------------------------------- */
#define RC_HCLUST_AVERAGE 0
#define RC_HCLUST_COMPLETE 1
#define RC_HCLUST_SINGLE 2
typedef struct rc_hclust_merge_t {
    int32_t a, b;  /* a < b; b goes into a */
    int32_t size;  /* members of a after the merge */
    uint32_t m_ab; /* 0 for average */
    int64_t s_ab;
} rc_hclust_merge_t;

/* counts: host n×n uint32; merges_out: rc_hclust_merge_t[n − 1] (untyped for plain FFIs, like runs_out above). */
int32_t rc_hclust(int32_t device, const void *counts /* uint32_t n×n */, int64_t m, int64_t n, int32_t linkage,
                  void *merges_out /* rc_hclust_merge_t[n-1] */, int64_t *binder_num /* n */, int32_t maxcut, double *vilb /* maxcut */,
                  double *kernel_ms);
/* On the counts of an m×n label matrix, built on the device where they stay (as rc_psm_search_samples; counts_ms likewise). */
int32_t rc_hclust_samples(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n, int32_t linkage,
                          void *merges_out /* rc_hclust_merge_t[n-1] */, int64_t *binder_num /* n */, int32_t maxcut,
                          double *vilb /* maxcut */, double *kernel_ms, double *counts_ms);
/* On the context's own device counts, read in place: chain state, layout and counts stay untouched.  RC_ERR_STATE when no
 * sample has been recorded. */
int32_t rc_hclust_ctx(rc_ctx *ctx, int64_t numsamples, int32_t linkage, void *merges_out /* rc_hclust_merge_t[n-1] */,
                      int64_t *binder_num /* n */, int32_t maxcut, double *vilb /* maxcut */, double *kernel_ms);
/* Host only: the labelling with K clusters (after the first n − K merges), labels 1..K in sortlabels order — names are
 * smallest members, so ranking the names gives that order.  RC_ERR_ARG: K outside 1..n, n outside 1..8192, merges that are
 * not merges of active clusters a < b. */
int32_t rc_hclust_cut(const void *merges /* rc_hclust_merge_t[n-1] */, int64_t n, int64_t K, int64_t *labels_out /* n */);

/* The expected loss of L given labellings (labels 1..n, L×n row-major, L <= 65536) under the counts: one kernel returns
 * T_i = Σ_{j: c_j=c_i} C_ij (uint32) for every labelling and point, reading each row of the counts once per group of 8
 * labellings; the host finishes from T and the cluster sizes:
 *   RC_PSM_BINDER  num_out = Σ_{i<j} C_ij + m·#{i<j: c_i=c_j} − Σ_i (T_i − m), exact; loss_out = num / (m·n(n−1)/2);
 *   RC_PSM_VILB    loss_out = f/n + 2·log m, f = Σ_i [log n_{c_i} − 2·log T_i] summed in index order in f64; num_out = 0.
 * Errors as rc_hclust; RC_ERR_ARG also for a label outside 1..n and an unknown loss. */
int32_t rc_psm_expected_loss(int32_t device, const void *counts /* uint32_t n×n */, int64_t m, int64_t n, int32_t loss, int64_t L,
                             const int64_t *labels /* L×n */, double *loss_out /* L */, int64_t *num_out /* L */, double *kernel_ms);
int32_t rc_psm_expected_loss_ctx(rc_ctx *ctx, int64_t numsamples, int32_t loss, int64_t L, const int64_t *labels /* L×n */,
                                 double *loss_out /* L */, int64_t *num_out /* L */, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Predict: where do observations go that were not in the fit?  For every posterior sample s and every new point i, the
 * Gibbs full conditional (src/mcmc.jl:192-252) of an (n+1)-th point whose own cluster is empty, and a draw from it.  New
 * points are allocated independently of each other given a sample.  No context: errors through rc_last_error(NULL).
 * DESIGN.md §8 "Predict".
 *
 * Quantisation, per new point: row i of Dnew is q_ij = llrint(ldexp(x_ij, eD_i)), eD_i = 62 − ex_i − ceil(log2 n) where
 * max_j |x_ij| < 2^ex_i (frexp) — the rule of the context's matrices, applied to the row; the log row likewise with eL_i
 * (logDnew_or_null = NULL: the host's libm log of Dnew).  A new point's result is therefore a pure function of its own
 * row, the samples and the offsets, whichever other points share the call.
 * Sums: for sample s with labels z, S_D[k] = Σ_j q_ij·[z_j = k] and S_L[k] likewise — exact int64.
 * Scores: an existing cluster k of size s_k (nothing is removed: the new point is in no cluster)
 *   A[s_k] + (log p_s + log(s_k − 1 + r_s)) + cL·S_L − (α + δ1 s_k)·log1p(S_D/β) + rep·(ζ + δ2 s_k)·log1p(S_D/γ),
 * A and cL as for the sweep, the two log1p by the sweep's own routines; a new cluster
 *   log(K_s + 1) + r_s·log(1 − p_s),  offered iff params->maxK == 0 || K_s < params->maxK.
 * Draw: Gumbel-max.  The uniform of candidate label c (0 = the new cluster) is Philox4x32-10 with key
 * (seed_lo, seed_hi ^ 0x50524544), counter (c, point_offset + i, s_lo, s_hi), s = sample_offset + sample index,
 * u = (top 52 bits + ½)·2^-52.  Ties go to the smaller label, the new cluster last.
 *
 * labels_out[s][i]: the drawn label in sample s's own label names, 0 = a cluster of its own.  map_out (may be NULL): the
 * argmax of the noise-free scores, same tie rule.  scores_out (may be NULL) [s][i][t]: t < K_s the noise-free score of the
 * t-th smallest label of sample s, column Kmax the new cluster (−inf when not offered), NaN between.  sums_out (may be
 * NULL) [s][i][t][0..1]: (S_D, S_L) of the same candidates (0 beyond K_s).  Kmax is read only when one of the two is given
 * and must then be >= every K_s.  eD_out, eL_out (may be NULL): the exponents of every new point.  kernel_ms (may be NULL):
 * device time of the call's kernels.
 *
 * Errors, all before any device work.  RC_ERR_ARG: a NULL required pointer; n, q or m < 1; a label outside 1..n; r <= 0 or
 * not finite; p outside (0, 1); params that rc_set_params would reject; Kmax below a K_s; a device that is not there.
 * RC_ERR_DOMAIN: an entry of Dnew that is not finite or not > 0, a given log that is not finite.  RC_ERR_CAPACITY (checked
 * first, before any array is read): n > 32767 or m·n >= 2^31.  q is unbounded: the host walks the new points, and the
 * samples if need be, in chunks of a device workspace of about 1 GiB.  RC_PREDICT_ROWS_GLOBAL=1 in the environment (read at
 * every call) makes the sums gather from the rows in global memory instead of LDS, as n > 10240 does, and
 * RC_PREDICT_WORKSPACE_KIB=<k> shrinks the workspace so that small calls are chunked — the same results either way; for tests.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_predict(int32_t device, int64_t n, int64_t q,
                   const double *Dnew /* q×n row-major: new point i to training point j */,
                   const double *logDnew_or_null /* q×n; NULL: host libm log() of Dnew */,
                   int64_t m, const int64_t *samples /* m×n, labels 1..n */,
                   const double *r /* m */, const double *p /* m */, const rc_params *params,
                   uint64_t seed, uint64_t sample_offset, uint64_t point_offset,
                   int64_t *labels_out /* m×q */, int64_t *map_out /* m×q or NULL */,
                   int64_t Kmax, double *scores_out /* m×q×(Kmax+1) or NULL */,
                   int64_t *sums_out /* m×q×Kmax×2 or NULL */,
                   int32_t *eD_out /* q or NULL */, int32_t *eL_out /* q or NULL */, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Predict from points: rc_predict for new observations given by their coordinates.  The distances, their logarithms, the
 * quantisation and the per-cluster summary of the draws stay on the device, and the samples are uploaded once per chunk of
 * samples, however many new points there are.  No context: errors through rc_last_error(NULL).  DESIGN.md §8 "Predict from
 * points".
 *
 * Distance: d_ij = sqrt(Σ_k (y_ik − x_jk)²) of new point i (row i of new_points) and training point j (row j of points), the
 * coordinates k in ascending order: acc = +0; per coordinate t = y_ik − x_jk (one subtraction) and acc = fma(t, t, acc) (one
 * explicit fused multiply-add); d_ij = the correctly rounded square root of acc.  Direct differences, so a new point next to
 * a training point does not cancel to zero; the bits are part of the contract (tests/predict_points_ref.py restates them).
 * Logarithm: the resolver's own table-driven one: log_ij is what rc_debug_flog with which = 0 returns for d_ij.
 * Quantisation, per new point, on the device: eD_i = 62 − ex − ceil(log2 n) with max_j d_ij < 2^ex, eL_i likewise from
 * max_j |log_ij| over the whole row (rc_predict's rule when it is given logarithms), q_ij = the round-to-nearest-even integer
 * of ldexp(·, e).
 * Everything after that is rc_predict's: sums, scores, draws, counters, tie rules and the optional outputs scores_out,
 * sums_out (Kmax as there), eD_out, eL_out and kernel_ms.  Defining property: with D = dist_out and L = log_out of a call,
 * rc_predict(D, L, … the same arguments …) returns the same labels, map, scores, sums, eD and eL, bit for bit.
 * dist_out, log_out (may be NULL; host q×n, filled chunk by chunk): the distances and logarithms; for tests and small q.
 *
 * Counts (counts_out for the draws, mapcounts_out for map; uint32 q×(K_p + 1); either may be NULL).  They need maps (the
 * maps_out of rc_relabel for the same samples: maps[s][t] the pivot label that the t-th smallest label of sample s is sent
 * to, 0 unmatched, −1 for t >= K_s; maps_width columns) and pivot_labels (the pivot's K_p labels, ascending).  The label of
 * (sample s, new point i) is 0 or the t-th smallest label of sample s; it counts in column k of row i when maps[s][t] is the
 * k-th pivot label (k = 1..K_p) and in column 0 otherwise (a cluster of its own, or a cluster of the sample without a
 * counterpart).  Every row sums to m.  The counts of the whole call (4·q·(K_p + 1) bytes each) live on the device and
 * accumulate there across chunks of samples.  labels_out and map_out may both be NULL when a counts output is given — then
 * nothing of size m×q crosses the bus; at least one of the four must be given.
 *
 * q is unbounded: the new points go through rc_predict's workspace plan in chunks, a new point costing its coordinates, its
 * f64 distances (and logarithms when log_out is given) beside what it costs there; the sorted orders of a chunk of samples
 * are built and uploaded once for all chunks of points.  RC_PREDICT_WORKSPACE_KIB and RC_PREDICT_ROWS_GLOBAL apply as for
 * rc_predict.  A new point's outputs are a pure function of its own coordinates, the training points, the samples and the
 * offsets.
 *
 * Errors.  RC_ERR_ARG: a NULL required pointer (points, new_points, samples, r, p, params); none of labels_out, map_out,
 * counts_out, mapcounts_out given; n, q or m < 1; dim outside 1..2^20; a counts output without maps or pivot_labels; and,
 * as for rc_predict, a label outside 1..n, r, p, params, Kmax below a K_s, a device that is not there; with a counts output
 * also maps_width below a K_s, pivot_labels not strictly ascending in 1..n, a maps entry that is neither 0, nor −1 at
 * t >= K_s, nor a pivot label.  RC_ERR_CAPACITY (checked before any array is read): n > 32767 or m·n >= 2^31.
 * RC_ERR_DOMAIN: a coordinate that is not finite (checked on the host before any device work); a squared distance that is
 * 0, subnormal or not finite — a new point that coincides with a training point, or coordinates whose scale underflows or
 * overflows the square — found on the device through a flag word, never by a fault: the message names the first such (new
 * point, training point) pair, 1-based, in row-major order; outputs of earlier chunks may have been written by then.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_predict_points(int32_t device, int64_t n, int64_t dim, const double *points /* n×dim row-major */,
                          int64_t q, const double *new_points /* q×dim row-major */,
                          int64_t m, const int64_t *samples /* m×n, labels 1..n */,
                          const double *r /* m */, const double *p /* m */, const rc_params *params,
                          uint64_t seed, uint64_t sample_offset, uint64_t point_offset,
                          int64_t *labels_out /* m×q or NULL */, int64_t *map_out /* m×q or NULL */,
                          const int64_t *maps /* m×maps_width or NULL */, int64_t maps_width,
                          const int64_t *pivot_labels /* Kp, ascending, or NULL */, int64_t Kp,
                          void *counts_out /* uint32_t q×(Kp+1) or NULL */, void *mapcounts_out /* uint32_t q×(Kp+1) or NULL */,
                          int64_t Kmax, double *scores_out /* m×q×(Kmax+1) or NULL */,
                          int64_t *sums_out /* m×q×Kmax×2 or NULL */,
                          double *dist_out /* q×n or NULL */, double *log_out /* q×n or NULL */,
                          int32_t *eD_out /* q or NULL */, int32_t *eL_out /* q or NULL */, double *kernel_ms);
/* rc_predict_points with the distances in the given metric (RC_METRIC_*, "Metrics from coordinates" above);
 * rc_predict_points is this call with RC_METRIC_EUCLIDEAN.  RC_ERR_ARG also for an unknown metric and for CORRELATION with
 * dim < 2.  RC_ERR_DOMAIN for the first bad pair by the rules stated there; the message names the pair, the metric and the
 * cause (coincident points, parallel points, a zero or constant vector, a scale that underflows or overflows). */
int32_t rc_predict_points_metric(int32_t metric, int32_t device, int64_t n, int64_t dim, const double *points /* n×dim row-major */,
                                 int64_t q, const double *new_points /* q×dim row-major */,
                                 int64_t m, const int64_t *samples /* m×n, labels 1..n */,
                                 const double *r /* m */, const double *p /* m */, const rc_params *params,
                                 uint64_t seed, uint64_t sample_offset, uint64_t point_offset,
                                 int64_t *labels_out /* m×q or NULL */, int64_t *map_out /* m×q or NULL */,
                                 const int64_t *maps /* m×maps_width or NULL */, int64_t maps_width,
                                 const int64_t *pivot_labels /* Kp, ascending, or NULL */, int64_t Kp,
                                 void *counts_out /* uint32_t q×(Kp+1) or NULL */, void *mapcounts_out /* uint32_t q×(Kp+1) or NULL */,
                                 int64_t Kmax, double *scores_out /* m×q×(Kmax+1) or NULL */,
                                 int64_t *sums_out /* m×q×Kmax×2 or NULL */,
                                 double *dist_out /* q×n or NULL */, double *log_out /* q×n or NULL */,
                                 int32_t *eD_out /* q or NULL */, int32_t *eL_out /* q or NULL */, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Joint predict: new observations that may form clusters with each other.  One posterior sample (training labels z over n
 * points, r_s, p_s) defines an independent problem whose state is z, which never changes, and the labels y_1..y_q of the q
 * new observations, which start unallocated.  No context: errors through rc_last_error(NULL).  DESIGN.md §8 "Joint predict".
 *
 * A visit of new point i does what src/mcmc.jl:192-252 does for point n+i of the (n+q)-point problem whose other
 * unallocated points do not exist:
 *  1. Remove i.  If it was allocated its cluster shrinks; a cluster made only of new points may die, training clusters cannot.
 *  2. Score every non-empty cluster with rc_predict's score above; S_D and S_L run over the cluster's members (its training
 *     points and the other allocated new points in it), s_k is the cluster's size without i.
 *  3. Offer a new cluster, log(K_i + 1) + r_s·log(1 − p_s), iff params->maxK == 0 || K_i < params->maxK; K_i counts all
 *     non-empty clusters after the removal, those born earlier in the same call included.
 *  4. Draw by Gumbel-max; ties go to the smaller label, the new cluster last.  A new cluster takes the lowest label of 1..n+q
 *     that has no member at that moment (findfirst(clustsizes .== 0), mcmc.jl:199), so a label freed by a death is reused.
 * Passes: pass 0 visits i = 1..q in the caller's order (sequential allocation: y_i sees z and y_1..y_{i−1}); `sweeps` >= 0
 * further passes visit 1..q again with everything else allocated — Gibbs on p(y | z, D, r_s, p_s).
 * Uniforms: Philox4x32-10, key (seed_lo, seed_hi ^ 0x5052444A), counter (candidate label, or 0 for the new cluster; visit
 * index v = pass·q + i, 0-based; s_lo; s_hi), s = sample_offset + sample index, u = (top 52 bits + ½)·2^-52.
 * (sweeps + 1)·q < 2^32 is required.
 * Fixed point: row i is the n entries of Dnew[i] followed by the q entries of Dnn[i]; the diagonal entry is ignored and
 * counts as 0.  The row is quantised with one exponent, eD_i = 62 − ex_i − ceil(log2(n + q)), rc_predict's rule with n + q
 * addends; its logarithms likewise (logDnew / logDnn both NULL: the host's libm log).  Every sum is an exact int64, so a
 * sample's result is a pure function of that sample, the rows, the seed and its own counter: splitting the samples over
 * several calls with sample_offset changes no bit.  The new points of a call always travel together.
 * Size-dependent terms: A[s] for sizes up to n + q; log p_s on the host; log(s − 1 + r_s) on the device by the sweep's
 * logarithm, which takes positive normal arguments: an r below the smallest normal double is RC_ERR_ARG here.
 *
 * labels_out[s][i]: the final label in sample s's own names; new clusters carry the free labels they took, there is no 0.
 * first_out (may be NULL): the labels after pass 0.  K_out[s]: clusters of the extended sample.  moves_out (may be NULL)
 * [s][pass]: the visits of the pass whose draw differs from the point's previous label (pass 0 gives q).  sums_out (may be
 * NULL) [s][i][0..1]: the int64 (S_D, S_L) of the cluster the point joined at its last visit, without the point; (0, 0) for
 * a cluster it opened.  eD_out, eL_out (may be NULL): the exponents of every new point.  kernel_ms (may be NULL): device time.
 *
 * Errors, all before any device work.  rc_predict's own apply (NULL pointers, sizes, labels, r, p, params, the device;
 * RC_ERR_DOMAIN for an entry of Dnew that is not finite or not > 0 or a given log that is not finite; RC_ERR_CAPACITY for
 * n > 32767 or m·n >= 2^31).  RC_ERR_ARG also: Dnn or K_out NULL, one of logDnew / logDnn without the other, sweeps < 0,
 * (sweeps + 1)·q >= 2^32.  RC_ERR_DOMAIN also: Dnn not symmetric, or not finite and > 0 off the diagonal.
 * RC_ERR_CAPACITY also: K_s + q > 4096 for a sample (the message names it) — a sample's slots, its clusters and up to q new
 * ones, live in the workgroup's LDS.  Larger q: call in blocks, each block's extended samples the next block's training set.
 * The host walks the samples in chunks whose base sums (q·16·ΣK_s bytes) fit a workspace of 1 GiB;
 * RC_PREDICT_WORKSPACE_KIB=<k> shrinks it as for rc_predict — the same results either way; for tests.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_predict_joint(int32_t device, int64_t n, int64_t q,
                         const double *Dnew /* q×n row-major */, const double *Dnn /* q×q symmetric, diagonal ignored */,
                         const double *logDnew_or_null /* q×n */, const double *logDnn_or_null /* q×q; both or neither */,
                         int64_t m, const int64_t *samples /* m×n, labels 1..n */,
                         const double *r /* m */, const double *p /* m */, const rc_params *params,
                         int64_t sweeps, uint64_t seed, uint64_t sample_offset,
                         int64_t *labels_out /* m×q */, int64_t *first_out /* m×q or NULL */, int64_t *K_out /* m */,
                         int64_t *moves_out /* m×(sweeps+1) or NULL */, int64_t *sums_out /* m×q×2 or NULL */,
                         int32_t *eD_out /* q or NULL */, int32_t *eL_out /* q or NULL */, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Partition distances: what the Binder loss, the VI and the information distance between each of L labellings and each
 * of m samples are made of, as exact integers — the L×m rectangle behind credible balls and exact expected losses.  No
 * context: errors through rc_last_error(NULL).  DESIGN.md §8 "Partition distances".
 *
 * With N_kl = #{j : labels[l][j] = k, samples[s][j] = l'} the contingency table of labelling l and sample s, and Gq / Phiq
 * the fixed-point table of rc_vi_gtable (Phiq(x) = Σ_{y<x} Gq[y]; the same table, not a second one):
 *   sq_out[l][s]  = P = Σ_kl N_kl²            phi_out[l][s] = T = Σ_kl Phiq(N_kl)
 *   lab_marg[l]   = (A₂, A_q, K) = (Σ_k n_k², Σ_k Phiq(n_k), number of clusters) of labelling l;  smp_marg[s] = (B₂, B_q, K)
 *                   likewise of sample s.
 * The three distances follow in integers:
 *   Binder numerator = (A₂ + B₂ − 2P)/2, the number of pairs of points on which the two partitions disagree — what
 *                      binderloss(normalised = false) returns; divide by n(n−1)/2 for the normalised loss;
 *   VI_q = A_q + B_q − 2T   and   ID_q = max(A_q, B_q) − T,   both in units of 2^-32/n nats: VI = VI_q/(2^32·n).
 *   Σ_s VI_q of a labelling is rc_vi_search's loss_num for it plus that search's constant Σ_s B_q.
 * Every output is a pure function of (labelling, sample) — bit for bit the same whatever L is, however the call is
 * chunked and whichever other labellings share it.  Any of sq_out, phi_out, lab_marg, smp_marg may be NULL (with both
 * sq_out and phi_out NULL no device is touched).  kernel_ms (may be NULL): device time of the call's kernels.
 *
 * Errors, all before any device work.  RC_ERR_ARG: samples or labels NULL; m, n or L < 1; a label outside 1..n (the
 * message names the sample or labelling and the position); a device that is not there.  RC_ERR_CAPACITY (checked before
 * any array is read): n > 32767, m·n >= 2^31 or L > 65536.  L and m are otherwise unbounded in memory terms: the host
 * walks the labellings, and the samples if need be, in chunks of a device workspace of about 1 GiB.  Labellings of more
 * than 1024 clusters keep their histograms in global memory instead of LDS; RC_PARTDIST_HIST_GLOBAL=1 in the environment
 * (read at every call) does that for every labelling, RC_PARTDIST_GQ_GLOBAL=1 reads Gq from global memory where its
 * reachable part would be copied to LDS, and RC_PARTDIST_WORKSPACE_KIB=<k> shrinks the workspace so that small calls are
 * chunked — the same integers either way; for tests.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_partition_distances(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n,
                               int64_t L, const int64_t *labels /* L×n, labels 1..n */,
                               int64_t *sq_out /* L×m or NULL */, int64_t *phi_out /* L×m or NULL */,
                               int64_t *lab_marg /* L×3 or NULL */, int64_t *smp_marg /* m×3 or NULL */, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Relabelling: each of m samples renamed onto a pivot labelling (a point estimate), and per point how often it lands in
 * each of the pivot's clusters — pivot relabelling in exact integers.  No context: errors through rc_last_error(NULL).
 * DESIGN.md §8 "Relabelling".
 *
 * Dense ids are given in ascending label order to the pivot's K_p clusters and to the K_s clusters of sample s;
 * N[k][l] = #{j : pivot[j] has dense id k, samples[s][j] has dense id l}.  The sample's clusters are matched to the
 * pivot's by the injective partial matching of size min(K_p, K_s) that maximises the matched overlap Σ N[σ(l)][l], found
 * by shortest augmenting paths with potentials on cost = −N: rows are the side with fewer clusters (the pivot on a tie),
 * inserted in ascending dense id from zero potentials; every step goes to the unused column of minimum reduced cost, the
 * smallest column id among equals.  The matching, not only its value, is therefore a function of the inputs.
 *   labels_out[s][j]  the label of point j in sample s in the pivot's names; 0 where its cluster is unmatched (K_s > K_p only)
 *   maps_out[s][t]    the pivot label that the t-th smallest label of sample s is sent to; 0 unmatched; −1 for t >= K_s.
 *                     maps_width columns, at least the largest K_s
 *   overlap_out[s]    the matched overlap: n − overlap points disagree with the pivot after renaming
 *   counts_out[j][k]  k = 0..K_p: the samples whose renamed label of point j is the pivot's k-th smallest label; column 0
 *                     counts unmatched.  Every row sums to m.  K_p is passed in so that the caller can size the array; it
 *                     must be the pivot's cluster count.
 * labels_out, maps_out and kernel_ms (device time of the call's kernels) may be NULL.  Every sample's outputs are a pure
 * function of (pivot, sample): the same whatever m is and however the call is chunked.
 *
 * Errors, all before any device work.  RC_ERR_ARG: samples, pivot, overlap_out or counts_out NULL; m or n < 1; a label
 * outside 1..n (the message names the sample and the position); K_p that is not the pivot's cluster count; maps_width
 * below the largest K_s; a device that is not there.  RC_ERR_CAPACITY: n > 32767 (checked before any array is read), a
 * pivot or a sample of more than 1024 clusters.  m is otherwise unbounded in memory terms: the samples go through a device
 * workspace of about 1 GiB in chunks, counts accumulating on the device.  The contingency table of a sample is kept in LDS
 * when it fits 128 KiB beside the assignment's vectors, else in global memory; RC_RELABEL_TABLE_GLOBAL=1 in the
 * environment (read at every call) does the latter for every sample and RC_RELABEL_WORKSPACE_KIB=<k> shrinks the
 * workspace so that small calls are chunked — the same integers either way; for tests.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_relabel(int32_t device, const int64_t *samples /* m×n, labels 1..n */, int64_t m, int64_t n,
                   const int64_t *pivot /* n, labels 1..n */, int64_t Kp,
                   int64_t *labels_out /* m×n or NULL */, int64_t *maps_out /* m×maps_width or NULL */, int64_t maps_width,
                   int64_t *overlap_out /* m */, void *counts_out /* uint32_t n×(Kp+1) */, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Scoring labellings: the log-likelihood (src/mcmc.jl:1-56) and log-prior (src/mcmc.jl:58-78) of each of L given labellings
 * under the model, against the context's fixed-point matrices as they are (64- or 32-bit storage, logD stored or derived,
 * the current internal point order read through its index map).  DESIGN.md §8 "Scoring labellings".
 *
 * For labelling l with its K_l clusters in ascending label order k = 0..K_l−1 and k <= t,
 *   B_D[l][k][t] = Σ_{i in k} Σ_{j in t} Dq[i][j]        B_L[l][k][t] likewise for logD (diagonal 0; D's as stored)
 * — rows in the smaller label, columns in the larger, matsum(D, clust_k, clust_t) of mcmc.jl:48 and what rc_loglik reads.
 * D need not be symmetric.  Every block is an exact integer carried as two halves, value = hi·2^24 + lo, each half the sum
 * of the halves of the per-row sums Σ_{j in t} Dq[i][j] (an int64 each), so n² terms cannot overflow.  Every output is a
 * pure function of (matrices, labelling): bit for bit the same whatever L is, however the call is chunked and whichever
 * other labellings share it.  The matrices are read once per chunk of labellings, never once per labelling.
 *
 * loglik_out[l] equals, bit for bit, rc_set_state(labels[l]) + rc_loglik on the same context with the same parameters
 * (params NULL: the context's, which must then be set; otherwise as after rc_set_params(params)).  logprior_out (may be
 * NULL; needs r and p) is rc_logprior(r[l], p[l]) of that state.  K_out (may be NULL): the K_l.  blocks_out (may be NULL):
 * per labelling in turn its K_l(K_l+1)/2 blocks in row-major (k, t >= k) order, 4 int64 each (D_hi, D_lo, L_hi, L_lo);
 * blocks_len is the caller's count of blocks and must equal Σ_l K_l(K_l+1)/2 (0 with a NULL pointer).  eD_out, eL_out (may
 * be NULL): the context's exponents, Dq = D·2^eD and Lq = logD·2^eL, which rc_loglik_from_blocks takes.  kernel_ms (may be
 * NULL): device time of the call's kernels.
 *
 * The call waits for the context's streams first and leaves the chain state, the layout, the row-sum tables, the
 * co-clustering counts and the choice of kernels untouched; a context with no state set is fine.
 *
 * Errors, all before any device work.  RC_ERR_ARG: ctx, labels or loglik_out NULL; L < 1; a label outside 1..n (the
 * message names the labelling and the position); an r that is <= 0 or not finite; a p outside (0, 1); logprior_out without
 * r and p; params that rc_set_params would reject; a blocks_len that does not match.  RC_ERR_STATE: params NULL on a
 * context without parameters.  RC_ERR_CAPACITY: n > 32767, L·n >= 2^31, a labelling of more than 4096 clusters.  L is
 * otherwise unbounded in memory terms: the rows and the labellings go through a device workspace of about 1 GiB in chunks.
 * RC_SCORE_ROWS_GLOBAL=1 in the environment (read at every call) makes the sums gather from the staged rows in global
 * memory instead of LDS, as n > 10240 does, and RC_SCORE_WORKSPACE_KIB=<k> shrinks the workspace so that small calls are
 * chunked — the same integers either way; for tests.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_score_labellings(rc_ctx *ctx, int64_t L, const int64_t *labels /* L×n, labels 1..n */,
                            const double *r /* L or NULL */, const double *p /* L or NULL */,
                            const rc_params *params /* NULL: the context's */,
                            double *loglik_out /* L */, double *logprior_out /* L or NULL */, int64_t *K_out /* L or NULL */,
                            int64_t *blocks_out /* blocks_len×4 or NULL */, int64_t blocks_len,
                            int32_t *eD_out, int32_t *eL_out, double *kernel_ms);

/* The scalar part of loglik for ONE labelling from its block sums, under any hyperparameters: host only, no device is
 * touched and no context is needed.  sizes: the K cluster sizes in ascending label order (each >= 1, Σ = n); blocks: the
 * K(K+1)/2 × 4 int64 of rc_score_labellings; eD, eL: the exponents it reported.  Long double arithmetic, terms summed in
 * ascending label order — the arithmetic of rc_loglik, so with the parameters of the scoring call the result is its
 * loglik_out bit for bit.  RC_ERR_ARG: a NULL pointer, n or K < 1, K > n, sizes that are not positive or do not sum to n,
 * params that rc_set_params would reject. */
int32_t rc_loglik_from_blocks(int64_t n, int64_t K, const int64_t *sizes /* K */, const int64_t *blocks /* K(K+1)/2 × 4 */,
                              int32_t eD, int32_t eL, const rc_params *params, double *out);

/* ---------------------------------------------------------------------------------------------------------------
 * Cluster profiles: the medoid of every cluster and, for every point, the sum of its distances within its own cluster and
 * its neighbour cluster — the integers the silhouette width (Rousseeuw 1987) is made of — for each of L given labellings,
 * against the context's fixed-point D as it is (64- or 32-bit storage, the current internal point order read through its
 * index map).  logD plays no part: a context that derives it computes no logarithm here.  DESIGN.md §8 "Cluster profiles".
 *
 * Dq is the integer matrix with D = Dq·2^-eD, in the caller's point order (what rc_get_matrix returns).  The diagonal entry
 * Dq[i][i] never counts, whatever the context holds there.  Labelling l has its K_l clusters in ascending label order, slots
 * k = 0..K_l−1 of sizes n_k; A(i) is the slot of point i.
 *   within[l][i]    = Σ_{j in A(i), j != i} Dq[i][j]                          (0 for a singleton)
 *   S_t(i)          = Σ_{j in t} Dq[i][j] for t != A(i).  The neighbour cluster of i is the slot t != A(i) of minimum mean
 *                     S_t(i)/n_t.  Means are compared exactly, S_t·n_u against S_u·n_t in 128 bits; ties go to the lower
 *                     slot, that is the smaller label.
 *   nearest[l][i]   = S_t(i) of the neighbour cluster, neighbour[l][i] = its label, in the caller's names.  With K_l = 1
 *                     both are 0.
 *   medoid of cluster k: its member i of minimum within[l][i]; ties go to the smallest point index.  Reported 1-based, as
 *                     rc_kmedoids reports medoids, with its within.
 * The silhouette width is host arithmetic on these: ā = within/(n_A − 1), b̄ = nearest/n_neighbour, s = (b̄ − ā)/max(ā, b̄),
 * and s = 0 for a singleton, for K_l = 1 and when max(ā, b̄) = 0; the scale 2^-eD cancels.
 * Every output is an exact integer and a pure function of (Dq, labelling): bit for bit the same whatever L is, however the
 * call is chunked, whichever other labellings share it and whatever the context's storage.  The matrix is read once per
 * chunk of labellings, never once per labelling.
 *
 * K_out (may be NULL): the K_l.  medoids_out, medoid_within_out (each may be NULL): per labelling in turn its K_l clusters
 * in ascending label order; medoids_len is the caller's count and must equal Σ_l K_l (0 when both are NULL).  within_out,
 * nearest_out, neighbour_out (each may be NULL): L×n.  eD_out (may be NULL): the context's exponent.  kernel_ms (may be
 * NULL): device time of the call's kernels.
 *
 * The call waits for the context's streams first and leaves the chain state, the layout, the row-sum tables, the
 * co-clustering counts and the choice of kernels untouched; a context with no state and no parameters set is fine.
 *
 * Errors, all before any device work (no output is written).  RC_ERR_ARG: ctx or labels NULL; L < 1; a label outside 1..n
 * (the message names the labelling and the position); a medoids_len that does not match.  RC_ERR_CAPACITY: n > 32767,
 * L·n >= 2^31, a labelling of more than 4096 clusters.  The rows and the labellings go through a device workspace of about
 * 1 GiB in chunks.  RC_PROFILE_ROWS_GLOBAL=1 in the environment (read at every call) makes the sums gather from the staged
 * rows in global memory instead of LDS, as n > 10240 does, and RC_PROFILE_WORKSPACE_KIB=<k> shrinks the workspace so that
 * small calls are chunked — the same integers either way; for tests.
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rc_cluster_profiles(rc_ctx *ctx, int64_t L, const int64_t *labels /* L×n, labels 1..n */,
                            int64_t *K_out /* L or NULL */,
                            int64_t *medoids_out /* medoids_len or NULL, 1-based */,
                            int64_t *medoid_within_out /* medoids_len or NULL */, int64_t medoids_len,
                            int64_t *within_out /* L×n or NULL */, int64_t *nearest_out /* L×n or NULL */,
                            int64_t *neighbour_out /* L×n or NULL */, int32_t *eD_out, double *kernel_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * MAP search: the greedy search of rc_psm_search and rc_vi_search (one run = starting labels, a point order, maxsweeps; the
 * same tie rules) over ALL partitions for the labelling of maximum log-posterior lp(c) = loglik + logprior — what
 * rc_score_labellings computes and mapestimate ranks candidates by — under the context's matrices as they are (64- or 32-bit
 * storage, logD stored or derived, the current internal point order read through its index map).  DESIGN.md §8 "MAP search".
 *
 * Criterion.  With rc_score_labellings' block sums B_D, B_L of the allocated points (D's stored diagonal entry travels with
 * its point into B_D[k][k], logD's diagonal is 0; D is taken as symmetric, which rc_create demands) and P_k = n_k(n_k−1)/2:
 *   within(k)    = (δ1−1)·B_L[k][k]/2 − P_k·lgΓ(δ1) + α·log β − lgΓ(α) + lgΓ(α+δ1·P_k) − (α+δ1·P_k)·log(β + B_D[k][k]/2)
 *   between(k,t) = (δ2−1)·B_L[k][t] − n_k·n_t·lgΓ(δ2) + ζ·log γ − lgΓ(ζ) + lgΓ(ζ+δ2·n_k·n_t) − (ζ+δ2·n_k·n_t)·log(γ + B_D[k][t])
 * (between only with repulsion), evaluated in the regrouped log1p(B/β) form of rc_loglik, and the prior's terms of
 * rc_logprior over the n' allocated points.  One visit takes point i out of its slot a, reduces row i into the exact int64
 * sums s_t = Σ_{j in t, j != i} Dq[i][j] and l_t (logD), and scores
 *   Δ_k   = [within(k ∪ i) − within(k)] + Σ_{t != k} [between(k ∪ i, t) − between(k, t)] + log(n_k+1) − log n_k + log(n_k+r−1) + log p
 *   Δ_new = within({i}) + Σ_t between({i}, t) + log(K+1) + r·log(1−p)            (K: the occupied slots with i out)
 * with B_D[k][k] += 2·s_k + Dq[i][i] and B_D[k][t] += s_t (B_L alike, without a diagonal).  The point goes to the maximum,
 * "stay" included, so every accepted move raises lp.  Equal scores: the own slot first, then the lowest slot; a new cluster
 * takes the slot just emptied, else the lowest free one.
 *
 * What is exact and what is not.  The row sums and the run's K×K block state are exact integers (a block as two halves,
 * value = hi·2^24 + lo, updated by adding and subtracting row sums, never reduced again).  The Δ are f64, with the library's
 * own lgamma (Stirling's series) and log1p (one log, corrected); they decide moves only, and a candidate's sum over its partners has a fixed shape, so a run is a
 * deterministic function of its arguments whatever else shares the call.  Everything reported is recomputed by the exact
 * path: loglik, logprior and logposterior of labels_out, and start_logposterior of a fully allocated start, are
 * rc_score_labellings' values for (labelling, r, p) under the same parameters, bit for bit.  A run's logposterior is never
 * below its start_logposterior up to the f64 error of a Δ.
 *
 * One run is rc_vi_search's: starting labels 0..n (0 = unallocated) compacted to slots by first appearance, the order a
 * permutation of 1..n, at most maxsweeps sweeps, the run ends after a sweep without a move (converged); each run has its own
 * r and p.  The slot cap Kcap is maxK when that is positive, else min(n, 1024); a new cluster is not offered at K = Kcap, and
 * `capped` counts the visits at which only the implicit cap (maxK = 0) withheld the offer.  params->maxK plays no part.
 * labels_out: sortlabels'd (src/utils.jl:69-74).  best: the first run of maximal logposterior (0-based).  blocks_out (may be
 * NULL): per run Kcap×Kcap×4 int64, the kernel's own final cells (D_hi, D_lo, L_hi, L_lo) of the ordered pair of slots
 * (k, t), cell ((k−1)·Kcap + (t−1)); slots_out (may be NULL): nruns×n, the kernel's final slots, 1-based — the two exist so
 * that the incremental state can be checked against rc_score_labellings' blocks (the halves may differ, the values may not).
 * kernel_ms (may be NULL): device time of the search kernel alone — the starting cells and the sweeps; neither the zeroing of
 * the cells nor the copy of blocks_out — summed over its launches (one for the runs whose cells fit 1 GiB, else several).
 *
 * The call waits for the context's streams first and leaves the chain state, the layout, the row-sum tables, the
 * co-clustering counts and the choice of kernels untouched; a context with no state set is fine.
 *
 * Errors, all before any device work, in this order.  RC_ERR_ARG: a NULL ctx or pointer; nruns < 1, maxsweeps < 1, maxK < 0;
 * a starting label outside 0..n; an order that is not a permutation; an r that is <= 0 or not finite; a p outside (0, 1);
 * params that rc_set_params would reject.  RC_ERR_STATE: params NULL on a context without parameters.  RC_ERR_CAPACITY:
 * n > 8192, 2·nruns·n >= 2^31, Kcap > 1024.  RC_ERR_ARG: a run that starts with more than Kcap clusters.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rc_map_run_t {
    double loglik, logprior, logposterior; /* of labels_out: rc_score_labellings' values, bit for bit */
    double start_logposterior;             /* NaN when the start had unallocated points */
    int32_t sweeps, converged, K, capped;
    int64_t moves;
} rc_map_run_t;

int32_t rc_map_search(rc_ctx *ctx, int32_t nruns, const int64_t *init /* nruns×n, 0 = unallocated */,
                      const int32_t *order /* nruns×n, 1-based */, const double *r /* nruns */, const double *p /* nruns */,
                      const rc_params *params /* NULL: the context's */, int32_t maxK, int32_t maxsweeps,
                      int64_t *labels_out /* nruns×n, sortlabels'd */, void *runs_out /* rc_map_run_t[nruns] */,
                      int64_t *blocks_out /* may be NULL: nruns×Kcap×Kcap×4 */, int64_t *slots_out /* may be NULL: nruns×n */,
                      int32_t *best /* first run of maximal logposterior */, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* REDCLUST_HIP_H */
