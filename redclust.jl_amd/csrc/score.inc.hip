// Scoring labellings: the log-likelihood (src/mcmc.jl:1-56) and log-prior (src/mcmc.jl:58-78) of each of L given labellings
// against a context's staged fixed-point matrices, without touching its state.  The sufficient statistics of a labelling are
// its cluster sizes and the K×K block sums of D and logD; for L labellings the matrices are still read once per chunk of
// labellings, not once per labelling.  DESIGN.md §8 "Scoring labellings"; the contract is in include/redclust_hip.h.
// Included at the end of redclust_hip.hip (same translation unit: shares fail(), HIPCHK, View, rc_load_L, rc_bin_add, the
// per-term helpers of loglik and logprior in hostmodel.inc.hpp, sync_and_check, the holders and checks of hostutil.inc.hip and slab.inc.hip).
//
// The block sums come out of the slab driver (slab.inc.hip): the context's rows, in the caller's order, are its rows, with the
// dense slot of every point, rslot[s][i], from its sorted orders; RC_SCORE_WORKSPACE_KIB and RC_SCORE_ROWS_GLOBAL are its
// switches for this entry point.
// k_score_rows (its staging kernel): one workgroup per row of a chunk of rows.  Row i of the caller's order is gathered through
// View.pi from the internal-order matrices, whatever their storage, into interleaved (Dq, Lq) pairs — a derived log is computed
// here, once per entry and chunk of labellings.
// k_score_blocks (its consumer): one workgroup per (labelling, column cluster t).  The slab's column is reduced over the rows,
// grouped by the row's own cluster k <= t, into LDS bins of (hi, lo) halves — k_blocksums' inner step, rc_bin_add — and added
// to the labelling's upper-triangle blocks.  Chunks of rows accumulate there; sums of halves are exact in any grouping, so the
// result does not depend on the chunking.

namespace scr {

constexpr int TPB_ROWS = 256, TPB_BLOCKS = 256;   // (slab::KMAX clusters: 32 B of LDS bins each, 128 KiB)

// rows[b][j] = (Dq, Lq)[row0 + b][j], caller's order.  Grid: one block per row of the chunk.
__global__ __launch_bounds__(TPB_ROWS) void k_score_rows(View V, int row0, ll2 *__restrict__ rows)
{
    const int n = V.n, u = V.pi[row0 + blockIdx.x];
    ll2 *dst = rows + (size_t)blockIdx.x * (size_t)n;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int x = V.pi[j];
        const size_t e = (size_t)u * V.ld + x;
        ll2 v;
        v.x = (V.bits == 64) ? ((const long long *)V.Dq)[e] : (long long)((const int *)V.Dq)[e];
        v.y = rc_load_L(V, u, x, v.x);
        dst[j] = v;
    }
}

struct BlockArgs {
    const ll2 *sums;                 // [np][ktot] the slab of this chunk of rows
    long long ktot;
    int np, row0, n;
    const unsigned short *rslot;     // [ms][n] dense slot of every point
    const int *col_lab;              // [ktot] the labelling (within the chunk) a slab column belongs to
    const long long *koff;           // [ms] first slab column of every labelling
    const long long *boff;           // [ms] first block of every labelling
    const int *K;                    // [ms]
    long long *blocks;               // [btot][4] upper triangles, row-major (k, t >= k); added to
};

// Grid: one block per slab column.  Dynamic LDS: (largest K of the chunk) × 4 words.
__global__ __launch_bounds__(TPB_BLOCKS) void k_score_blocks(const BlockArgs a)
{
    extern __shared__ __align__(16) unsigned char scr_lds[];
    u64 *bins = reinterpret_cast<u64 *>(scr_lds);   // [t + 1][4]
    const long long c = blockIdx.x;
    const int s = a.col_lab[c], t = (int)(c - a.koff[s]);
    const long long K = a.K[s];
    for (int q = threadIdx.x; q < (t + 1) * 4; q += blockDim.x) bins[q] = 0;
    __syncthreads();
    const unsigned short *rs = a.rslot + (size_t)s * (size_t)a.n + a.row0;
    for (int i = threadIdx.x; i < a.np; i += blockDim.x) {
        const int k = rs[i];
        if (k > t) continue;                        // rows in the smaller label, columns in the larger
        const ll2 v = a.sums[(size_t)i * (size_t)a.ktot + c];
        rc_bin_add(bins, k, v.x, v.y);
    }
    __syncthreads();
    long long *out = a.blocks + a.boff[s] * 4;      // this block alone owns column t of its labelling
    for (int q = threadIdx.x; q < (t + 1) * 4; q += blockDim.x) {
        const long long k = q >> 2;
        out[(k * K - k * (k - 1) / 2 + (t - k)) * 4 + (q & 3)] += (long long)bins[q];
    }
}

// The scalar part of loglik for one labelling from its upper-triangle blocks (row-major (k, t >= k), ascending label order):
// loglik_host_c's sum, the same helpers in the same order.
// (the lgamma differences are memoised by the integer pair count as there: labellings of one call — the cuts of a dendrogram,
// consecutive samples of a chain — share most of their cluster sizes; the value is that of evaluating afresh)
struct LgMemo { std::unordered_map<long long, long double> within, between; };
static double loglik_blocks(const rc_params &P, int eD, int eL, int64_t K, const int *sizes, const long long *blocks, LgMemo &memo)
{
    const LLConsts C = ll_consts(P, eD, eL);
    long double L1 = 0, L2 = 0;
    auto at = [&](int64_t k, int64_t t) { return blocks + (k * K - k * (k - 1) / 2 + (t - k)) * 4; };
    for (int64_t k = 0; k < K; ++k) {
        const long double pairs = ll_within_pairs(sizes[k]);
        auto it = memo.within.find((long long)pairs);
        if (it == memo.within.end()) it = memo.within.emplace((long long)pairs, ll_within_lg(C, pairs)).first;
        L1 += ll_within_term(C, pairs, it->second, at(k, k));
    }
    if (P.repulsion)
        for (int64_t k = 0; k < K; ++k)
            for (int64_t t = k + 1; t < K; ++t) {
                const long double pairs = ll_between_pairs(sizes[k], sizes[t]);
                auto it = memo.between.find((long long)pairs);
                if (it == memo.between.end()) it = memo.between.emplace((long long)pairs, ll_between_lg(C, pairs)).first;
                L2 += ll_between_term(C, pairs, it->second, at(k, t));
            }
    if (memo.within.size() > (1u << 20)) memo.within.clear();
    if (memo.between.size() > (1u << 20)) memo.between.clear();
    return (double)(L1 + L2);
}

// what the caller passed, after the checks
struct Call {
    rc_ctx *c;
    int64_t n, L;
    const int64_t *labels;
    const double *r, *p;
    const rc_params *P;
    double *loglik_out, *logprior_out;
    int64_t *blocks_out;
    const int *K;                    // [L]
    const int64_t *boff;             // [L + 1] first block of every labelling in blocks_out
    bool rows_global;
    size_t workspace;
    LgMemo *memo;
};

// labellings s0 .. s0 + ms - 1 against every row, the rows in chunks of at most qc.  ms_acc: device milliseconds, added to.
static int32_t run_labellings(const char *who, const Call &a, int64_t s0, int64_t ms, int64_t qc, double &ms_acc)
{
    rc_ctx *c = a.c;
    const int64_t n = a.n, btot = a.boff[s0 + ms] - a.boff[s0];
    const int Kmax = *std::max_element(a.K + s0, a.K + s0 + ms);
    prd::Orders O;
    std::vector<int> sizes, col_lab;
    std::vector<long long> boff, h_blocks;
    bool ok = true;
    try {
        boff.resize((size_t)ms); h_blocks.resize((size_t)btot * 4);
        for (int64_t s = 0; s < ms; ++s) boff[(size_t)s] = a.boff[s0 + s] - a.boff[s0];
        long long kt = 0;
        for (int64_t s = 0; s < ms; ++s) kt += a.K[s0 + s];
        sizes.resize((size_t)kt); col_lab.resize((size_t)kt);
    } catch (const std::bad_alloc &) { ok = false; }
    ok = ok && O.build(a.labels, n, a.K, s0, ms, true, [&](int64_t s, long long at, int64_t, int sz) { sizes[(size_t)at] = sz; col_lab[(size_t)at] = (int)s; });
    if (!ok) return fail(c, RC_ERR_OOM, "%s: no host memory for the sorted orders of %lld labellings", who, (long long)ms);

    DeviceBuffers B;
    int *d_col_lab; long long *d_boff, *d_blocks;
    HIPCHK(c, O.upload(B));
    HIPCHK(c, B.alloc(d_col_lab, col_lab.size()));
    HIPCHK(c, B.alloc(d_boff, (size_t)ms));
    HIPCHK(c, B.alloc(d_blocks, (size_t)btot * 4));
    HIPCHK(c, hipMemcpy(d_col_lab, col_lab.data(), col_lab.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_boff, boff.data(), (size_t)ms * sizeof(long long), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(d_blocks, 0, (size_t)btot * 4 * sizeof(long long)));

    const size_t lds_bins = (size_t)Kmax * 4 * sizeof(u64);
    HIPCHK(c, set_dynamic_lds(k_score_blocks, lds_bins));
    const int32_t rc = slab::run_rows(c, O, B, qc, a.rows_global, k_score_rows, TPB_ROWS, [&](const ll2 *d_sums, int64_t i0, int64_t np) {
        BlockArgs b{};
        b.sums = d_sums; b.ktot = O.ktot; b.np = (int)np; b.row0 = (int)i0; b.n = (int)n; b.rslot = O.d_rslot; b.col_lab = d_col_lab;
        b.koff = O.d_koff; b.boff = d_boff; b.K = O.d_K; b.blocks = d_blocks;
        k_score_blocks<<<(unsigned)O.ktot, TPB_BLOCKS, lds_bins, 0>>>(b);
    }, ms_acc);
    if (rc != RC_OK) return rc;
    HIPCHK(c, hipMemcpy(h_blocks.data(), d_blocks, h_blocks.size() * sizeof(long long), hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < ms; ++s) {
        const int K = O.Ks[(size_t)s];
        const int *sz = sizes.data() + O.koff[(size_t)s];
        const long long *blk = h_blocks.data() + boff[(size_t)s] * 4;
        a.loglik_out[s0 + s] = loglik_blocks(*a.P, c->eD, c->eL, K, sz, blk, *a.memo);
        if (a.logprior_out) {
            const double r = a.r[s0 + s], p = a.p[s0 + s];
            double lp = logprior_head(*a.P, (double)n, (double)K, r, p);
            for (int t = 0; t < K; ++t) lp += logprior_cluster(sz[t], r);
            a.logprior_out[s0 + s] = lp;
        }
        if (a.blocks_out) memcpy(a.blocks_out + a.boff[s0 + s] * 4, blk, (size_t)K * (K + 1) / 2 * 4 * sizeof(int64_t));
    }
    return RC_OK;
}

// rc_score_labellings behind its argument checks — L labellings of labels in 1..n, r and p valid or null, P checked — for the
// entry points that score labellings of their own through the same path (rc_map_search): the capacity in clusters, the
// blocks_len, the wait for the context's streams, the chunks of the slab driver and the outputs.
static int32_t score_valid(rc_ctx *c, const char *who, int64_t L, const int64_t *labels, const double *r, const double *p, const rc_params &P,
                           double *loglik_out, double *logprior_out, int64_t *K_out, int64_t *blocks_out, int64_t blocks_len,
                           double *kernel_ms, int32_t *eD_out = nullptr, int32_t *eL_out = nullptr)
{
    const int64_t n = c->n;
    int32_t rc;
    std::vector<int> K, seen;
    std::vector<int64_t> boff;
    try { K.assign((size_t)L, 0); seen.assign((size_t)n + 1, -1); boff.assign((size_t)L + 1, 0); }
    catch (const std::bad_alloc &) { return fail(c, RC_ERR_OOM, "%s: no host memory", who); }
    const int64_t over = count_clusters(labels, L, n, slab::KMAX, seen, K.data());
    if (over < L) return fail(c, RC_ERR_CAPACITY, "%s: labelling %lld has %d clusters, more than the %lld whose bins fit the workgroup's LDS", who, (long long)over + 1, K[(size_t)over], (long long)slab::KMAX);
    for (int64_t s = 0; s < L; ++s) boff[(size_t)s + 1] = boff[(size_t)s] + (int64_t)K[(size_t)s] * (K[(size_t)s] + 1) / 2;
    if (blocks_len != (blocks_out ? boff[(size_t)L] : 0))
        return fail(c, RC_ERR_ARG, "%s: blocks_len = %lld, the labellings have %lld blocks%s", who, (long long)blocks_len, (long long)boff[(size_t)L],
                    blocks_out ? "" : " (and blocks_out is NULL: pass 0)");
    HIPCHK(c, hipSetDevice(c->dev));
    rc = sync_and_check(c, true);
    if (rc != RC_OK) return rc;
    if (c->sC) HIPCHK(c, hipStreamSynchronize(c->sC));
    LgMemo memo;
    Call a{c, n, L, labels, r, p, &P, loglik_out, logprior_out, blocks_out, K.data(), boff.data(),
           env_flag("RC_SCORE_ROWS_GLOBAL"),                                  // tests: gather from the rows in global memory at small n
           env_workspace_kib("RC_SCORE_WORKSPACE_KIB", slab::WORKSPACE), &memo};
    // Chunks.  Device bytes per row for a run of labellings: the staged row and its slots' sums.  Labellings are taken while 512
    // rows (or all n) of them fit the workspace, their sorted orders fit theirs and their blocks a quarter of the workspace; the
    // rows then go in chunks of what fits.
    const int64_t ms_cap = slab_ms_cap(slab::PERM_BYTES, 4, n);
    double ms_acc = 0.0;
    for (int64_t s0 = 0; s0 < L;) {
        const SlabChunk ch = slab_plan(s0, K.data(), L, ms_cap, 16 * (size_t)n, 0, n, std::min<int64_t>(n, 512), a.workspace,
                                       [](size_t k) { return 32 * (k * (k + 1) / 2); }, a.workspace / 4);
        rc = run_labellings(who, a, s0, ch.ms, ch.qc, ms_acc);
        if (rc != RC_OK) return rc;
        s0 += ch.ms;
    }
    if (K_out) for (int64_t s = 0; s < L; ++s) K_out[s] = K[(size_t)s];
    if (eD_out) *eD_out = c->eD;
    if (eL_out) *eL_out = c->eL;
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

}  // namespace scr

extern "C" int32_t rc_score_labellings(rc_ctx *c, int64_t L, const int64_t *labels, const double *r, const double *p,
                                       const rc_params *params, double *loglik_out, double *logprior_out, int64_t *K_out,
                                       int64_t *blocks_out, int64_t blocks_len, int32_t *eD_out, int32_t *eL_out, double *kernel_ms)
{
    const char *who = "rc_score_labellings";
    int32_t rc = clu::check_ctx(c, who);
    if (rc != RC_OK) return rc;
    if (!labels || !loglik_out) return fail(c, RC_ERR_ARG, "%s: NULL argument", who);
    if (L < 1) return fail(c, RC_ERR_ARG, "%s: need L >= 1 (got %lld)", who, (long long)L);
    if (logprior_out && (!r || !p)) return fail(c, RC_ERR_ARG, "%s: the log-prior needs r and p", who);
    const int64_t n = c->n;
    rc = check_label_shape(c, who, n, "points", L, "L");
    if (rc != RC_OK) return rc;
    if (!params && !c->have_params) return fail(c, RC_ERR_STATE, "%s: params is NULL and the context has no parameters set", who);
    const rc_params P = params ? *params : c->P;
    rc = check_params(c, who, &P);
    if (rc != RC_OK) return rc;
    rc = check_r_p(c, who, "labelling", L, r, p);
    if (rc != RC_OK) return rc;
    rc = check_label_rows(c, who, "labelling", labels, L, n);
    if (rc != RC_OK) return rc;
    return scr::score_valid(c, who, L, labels, r, p, P, loglik_out, logprior_out, K_out, blocks_out, blocks_len, kernel_ms, eD_out, eL_out);
}

extern "C" int32_t rc_loglik_from_blocks(int64_t n, int64_t K, const int64_t *sizes, const int64_t *blocks, int32_t eD, int32_t eL,
                                         const rc_params *params, double *out)
{
    const char *who = "rc_loglik_from_blocks";
    if (!sizes || !blocks || !params || !out) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (n < 1 || K < 1 || K > n) return fail(nullptr, RC_ERR_ARG, "%s: need n >= 1 and 1 <= K <= n (got n=%lld K=%lld)", who, (long long)n, (long long)K);
    const int32_t rc = check_params(nullptr, who, params);
    if (rc != RC_OK) return rc;
    int64_t tot = 0;
    for (int64_t k = 0; k < K; ++k) {
        if (sizes[k] < 1 || sizes[k] > n) return fail(nullptr, RC_ERR_ARG, "%s: size %lld of cluster %lld outside 1..n", who, (long long)sizes[k], (long long)k + 1);
        tot += sizes[k];
    }
    if (tot != n) return fail(nullptr, RC_ERR_ARG, "%s: the sizes sum to %lld, not n = %lld", who, (long long)tot, (long long)n);
    std::vector<int> sz;
    try { sz.assign(sizes, sizes + K); } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory", who); }
    scr::LgMemo memo;
    *out = scr::loglik_blocks(*params, eD, eL, K, sz.data(), (const long long *)blocks, memo);
    return RC_OK;
}
