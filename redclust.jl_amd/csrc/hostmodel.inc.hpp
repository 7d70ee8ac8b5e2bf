// The host statistics of the model: the log-likelihood from exact block sums, the log-prior, and the whole split–merge proposal
// (restricted Gibbs scans, prior and proposal ratios, the merge decided from additive block sums, the MH decision).  Plain C++17:
// no HIP, no globals, no environment reads, no context — every function reads a HostModel, the view of what the context holds for
// them, so the chain loop can run them on worker threads and a CPU program can run them without a device.  redclust_hip.hip
// includes it ahead of its context struct (which keeps one LLCache) and builds the view with host_model(c) at each call; chain.inc.hip
// and score.inc.hip use it from there.  tests/hostmodel_host.cpp includes it on its own, with __host__, __device__ and
// __forceinline__ defined away for philox.inc.hpp; tests/test_hostmodel_cpu.py builds that program under ASan / UBSan and holds
// what it prints against the C oracle, proposal by proposal.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/redclust_hip.h"
#include "philox.inc.hpp"

#define RC_LO_BITS 24             // a block sum is kept as two int64 halves, sum of (x >> RC_LO_BITS) and sum of the low RC_LO_BITS bits (rc_bin_add,
                                  // k_blocksums), so that n² terms cannot overflow 64 bits
#define RC_MAX_KCAP 4096          // slot capacity up to which the resolver's per-slot tables live in LDS (the fast path) — and up to which
                                  // loglik_host_c keeps its per-pair memo

// What the host model reads of a context: the parameters, the size, the fixed-point exponents of D and logD, the slot capacity and
// the host matrices borrowed from the caller (rc_attach_host_matrices; only the proposal's scans read them).  Built per call, never
// kept: kcap grows and rc_set_params changes P.
struct HostModel {
    rc_params P;
    int64_t n;
    int eD, eL, kcap;
    const double *D, *L;
};

// lgammal(alpha + delta1*pairs) - lgammal(alpha) and the zeta analogue, memoised by the integer pair count: between
// consecutive rc_loglik calls cluster sizes rarely change, so nearly all of the K + K(K-1)/2 evaluations hit
struct LLTerm { long long e[4] = {0, 0, 0, 0}; int sk = -1, st = -1; long double term = 0; };
struct LLCache {                     // memo of loglik_host: one per thread that evaluates log-likelihoods
    std::unordered_map<long long, long double> lg_memo1, lg_memo2;
    std::vector<LLTerm> ll_cache;    // loglik terms per slot pair ([t][k], ll_dim × ll_dim), see loglik_host
    int ll_dim = 0;
};

// The per-term arithmetic of loglik (mcmc.jl:26-54), shared by loglik_host_c below — rc_loglik and the chain loop — and by the
// scoring entries of score.inc.hip: the constants of one parameter set, a block sum as a long double, and the term of one
// cluster (within) or one pair of clusters (between) from its pair count, its memoisable lgamma difference and its block.
struct LLConsts { long double d1, d2, al, be, ze, ga, lga, lgz, lgd1, lgd2, lb, lg, scD, scL; };
static LLConsts ll_consts(const rc_params &P, int eD, int eL)
{
    LLConsts C;
    C.d1 = P.delta1; C.d2 = P.delta2; C.al = P.alpha; C.be = P.beta; C.ze = P.zeta; C.ga = P.gamma;
    C.lga = lgammal(C.al); C.lgz = lgammal(C.ze); C.lgd1 = lgammal(C.d1); C.lgd2 = lgammal(C.d2);
    C.lb = logl(C.be); C.lg = logl(C.ga);
    C.scD = ldexpl(1.0L, -eD); C.scL = ldexpl(1.0L, -eL);
    return C;
}
static inline long double ll_block(const LLConsts &C, const long long *e, int which)
{
    return ((long double)e[which ? 2 : 0] * (long double)(1ll << RC_LO_BITS) + (long double)e[which ? 3 : 1]) * (which ? C.scL : C.scD);
}
static inline long double ll_within_pairs(int size)
{
    const long double sz = size;
    return sz * (sz - 1) / 2;  // binomial(sz_k, 2)
}
static inline long double ll_within_lg(const LLConsts &C, long double pairs) { return lgammal(C.al + C.d1 * pairs) - C.lga; }
static inline long double ll_within_term(const LLConsts &C, long double pairs, long double lgdiff, const long long *e)
{
    const long double a = C.al + C.d1 * pairs;
    const long double bd = ll_block(C, e, 0) / 2, bl = ll_block(C, e, 1) / 2;
    return (C.d1 - 1) * bl - pairs * C.lgd1 + lgdiff - C.d1 * pairs * C.lb - a * log1pl(bd / C.be);
}
static inline long double ll_between_pairs(int sk, int st) { return (long double)sk * (long double)st; }
static inline long double ll_between_lg(const LLConsts &C, long double pairs) { return lgammal(C.ze + C.d2 * pairs) - C.lgz; }
static inline long double ll_between_term(const LLConsts &C, long double pairs, long double lgdiff, const long long *e)
{
    const long double z = C.ze + C.d2 * pairs;
    const long double bd = ll_block(C, e, 0), bl = ll_block(C, e, 1);
    return (C.d2 - 1) * bl - pairs * C.lgd2 + lgdiff - C.d2 * pairs * C.lg - z * log1pl(bd / C.ga);
}

// Scalar part of loglik (mcmc.jl:26-54) in long double, regrouped as in the oracle's "stable" mode, from the exact
// fixed-point block sums B[t][k] (hi × hi × 4: D hi/lo, logD hi/lo) and the slot sizes.  A term depends only on its
// two cluster sizes and its block sums, and most of them do not change from one recorded sample to the next, so the
// terms are cached per slot pair and re-evaluated only when their (integer) inputs differ: the value — and the order
// of the summation — is exactly that of evaluating every term afresh.
// The terms are summed in ascending LABEL order (slabel: the label of every slot), the order of the reference's loops over
// findall(clustsizes .> 0) (mcmc.jl:13-53) — not in slot order: slot numbers depend on the history of births and deaths (and
// differ between the speculative and the synchronous chain loop after a rollback), labels do not, so the value is a function of
// the partition alone, bit for bit.
static double loglik_host_c(const HostModel &M, LLCache &cache, int hi, const int *ssize, const long long *B, const int *slabel)
{
    const rc_params &P = M.P;
    const LLConsts C = ll_consts(P, M.eD, M.eL);
    // (the per-pair memo is 64 B per slot pair: kept up to the fast path's capacity; a wide context evaluates every term afresh)
    const bool memo = hi <= RC_MAX_KCAP;
    if (memo && hi > cache.ll_dim) {
        cache.ll_dim = std::max(hi, std::min(std::min(M.kcap, RC_MAX_KCAP), 2 * hi));
        cache.ll_cache.assign((size_t)cache.ll_dim * cache.ll_dim, LLTerm{});
    }
    LLTerm scratch_term;
    std::vector<int> act;
    for (int k = 0; k < hi; ++k)
        if (ssize[k] > 0) act.push_back(k);
    std::sort(act.begin(), act.end(), [&](int x, int y) { return slabel[x] < slabel[y]; });
    long double L1 = 0, L2 = 0;
    for (int k : act) {
        const long long *e = &B[((size_t)k * hi + k) * 4];
        if (!memo) scratch_term = LLTerm{};
        LLTerm &T = memo ? cache.ll_cache[(size_t)k * cache.ll_dim + k] : scratch_term;
        if (!(T.sk == ssize[k] && T.e[0] == e[0] && T.e[1] == e[1] && T.e[2] == e[2] && T.e[3] == e[3])) {
            const long double pairs = ll_within_pairs(ssize[k]);
            const long long pk = (long long)pairs;
            auto it = cache.lg_memo1.find(pk);
            if (it == cache.lg_memo1.end()) it = cache.lg_memo1.emplace(pk, ll_within_lg(C, pairs)).first;
            T.term = ll_within_term(C, pairs, it->second, e);
            T.sk = ssize[k]; T.st = ssize[k];
            std::memcpy(T.e, e, sizeof(T.e));
        }
        L1 += T.term;
    }
    if (cache.lg_memo1.size() > (1u << 20)) cache.lg_memo1.clear();
    if (cache.lg_memo2.size() > (1u << 20)) cache.lg_memo2.clear();
    if (P.repulsion)
        for (size_t x = 0; x < act.size(); ++x)
            for (size_t y = x + 1; y < act.size(); ++y) {
                const int k = act[x], t = act[y];
                const long long *e = &B[((size_t)t * hi + k) * 4];
                if (!memo) scratch_term = LLTerm{};
                LLTerm &T = memo ? cache.ll_cache[(size_t)t * cache.ll_dim + k] : scratch_term;
                if (!(T.sk == ssize[k] && T.st == ssize[t] && T.e[0] == e[0] && T.e[1] == e[1] && T.e[2] == e[2] && T.e[3] == e[3])) {
                    const long double pairs = ll_between_pairs(ssize[k], ssize[t]);
                    const long long pk = (long long)pairs;
                    auto it = cache.lg_memo2.find(pk);
                    if (it == cache.lg_memo2.end()) it = cache.lg_memo2.emplace(pk, ll_between_lg(C, pairs)).first;
                    T.term = ll_between_term(C, pairs, it->second, e);
                    T.sk = ssize[k]; T.st = ssize[t];
                    std::memcpy(T.e, e, sizeof(T.e));
                }
                L2 += T.term;
            }
    return (double)(L1 + L2);
}

// The terms of logprior (mcmc.jl:58-78), shared with score.inc.hip: everything but the clusters' own terms, from n, K, r and p;
// and the term of one cluster of a given size, to be added in ascending label order.
static double logprior_head(const rc_params &P, double n, double K, double r, double p)
{
    // logpdf(Gamma(η, 1/σ), r) + logpdf(Beta(u, v), p)   (mcmc.jl:73)
    const double lgam = P.eta * std::log(P.sigma) - std::lgamma(P.eta) + (P.eta - 1) * std::log(r) - P.sigma * r;
    const double lbet = std::lgamma(P.u + P.v) - std::lgamma(P.u) - std::lgamma(P.v) + (P.u - 1) * std::log(p) + (P.v - 1) * std::log(1 - p);
    return std::lgamma(K + 1) + (n - K) * std::log(p) + (r * K) * std::log(1 - p) - K * std::lgamma(r) + lgam + lbet;
}
static inline double logprior_cluster(int size, double r) { return std::log((double)size) + std::lgamma((double)size + r - 1); }

// logprior (mcmc.jl:58-78) from slot sizes / labels
// (nslots: length of ssize / slabel — the capacity at the time the tables were taken, which the context's may have outgrown since)
static double logprior_host(const HostModel &M, const int *ssize, const int *slabel, double r, double p, int nslots = -1)
{
    if (nslots < 0) nslots = M.kcap;
    double K = 0;
    for (int k = 0; k < nslots; ++k) K += ssize[k] > 0;
    double L = logprior_head(M.P, (double)M.n, K, r, p);
    // Σ_j log n_j + lgΓ(n_j + r − 1) over non-empty clusters in ascending label order (mcmc.jl:74-76)
    std::vector<std::pair<int, int>> bylabel;
    for (int k = 0; k < nslots; ++k)
        if (ssize[k] > 0) bylabel.push_back({slabel[k], ssize[k]});
    std::sort(bylabel.begin(), bylabel.end());
    for (auto &e : bylabel) L += logprior_cluster(e.second, r);
    return L;
}

// ===================================================================================================
// Split–merge step (src/mcmc.jl:356-479) — SURVEY.md §8f-1.
// The proposal is a short sequential scalar computation over the |S| members of two clusters (restricted Gibbs
// scans, src/mcmc.jl:259-354): it runs on the host, as it does in the reference, on host matrices borrowed from
// the caller (MCMCData.D / .logD), in the reference's literal arithmetic including its quirks Q1–Q3 (SURVEY.md
// §3.2).  The device supplies what is data-parallel: both log-likelihoods of the acceptance ratio (mcmc.jl:462-464)
// from the exact S table — the proposed state is applied with k_apply_moves and, unless accepted, reverted
// bit-exactly (integer corrections).
// ===================================================================================================
static double rc_uniform_mh(uint64_t seed, uint64_t iter, uint64_t mh, uint64_t draw)
{
    return rc_unit52(rc_philox((uint32_t)draw, (uint32_t)mh, (uint32_t)iter, (uint32_t)(iter >> 32), (uint32_t)seed,
                               (uint32_t)(seed >> 32) ^ RC_MH_TAG));
}

// out = log.(D - Diagonal(D) + I) (types.jl:155) with libm's log of the caller's doubles — what the split–merge scans read (they are
// pinned in the reference's literal arithmetic on log(D), golden_mh.npz).  Rows dealt to the host's cores: a serial loop is 0.5 s at
// n = 8192 and 10 s at n = 32768.
static void host_log_matrix(const double *D, int64_t n, double *out)
{
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::thread::hardware_concurrency(), (int64_t)64, n / 64 + 1}));
    auto rows = [&](int t) {
        for (int64_t i = t; i < n; i += nt)
            for (int64_t j = 0; j < n; ++j) out[(size_t)(i * n + j)] = (i == j) ? 0.0 : std::log(D[(size_t)(i * n + j)]);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) {
        try { th.emplace_back(rows, t); }
        catch (const std::system_error &) { for (int u = t; u < nt; ++u) rows(u); break; }   // (no more threads: the rest here)
    }
    rows(0);
    for (auto &t : th) t.join();
}

namespace {
// literal arithmetic of sample_labels_Gibbs_restricted! on the host matrices
struct Restricted {
    const HostModel *c;
    const double *D, *L;
    int64_t n;
    double r, p;
    uint64_t seed, iter, mh;
    double abratio, zgratio, lg_d1, lg_d2, logp;
    const std::vector<int64_t> *U;  // sorted indices of i, j and S: every member of the two candidate clusters
    std::vector<std::vector<int64_t>> fixed_members;  // members of C[1] / C[2] when they are not candidates
    int64_t fixed_label[2] = {-1, -1};

    // Row sums of item x over the members of the two candidate clusters, in ONE pass over U (ascending index, so
    // each cluster's sum is accumulated in ascending member order exactly as findall + matsum do, mcmc.jl:308-311,
    // utils.jl:9-17).  out[0..1] = D sums, out[2..3] = logD sums.
    // The members are kept as two sorted index lists (rebuilt from U at the start of a scan, updated as items move), so
    // the four sums are four independent add chains without a label test per element.
    std::vector<int64_t> mem[2];
    void cand_sums(int64_t x, double out[4]) const
    {
        double d0 = 0, d1 = 0, l0 = 0, l1 = 0;
        const double *Dx = D + (size_t)x * (size_t)n, *Lx = L + (size_t)x * (size_t)n;
        const std::vector<int64_t> &A = mem[0], &B = mem[1];
        const size_t na = A.size(), nb = B.size(), both = na < nb ? na : nb;
        size_t q = 0;
        for (; q < both; ++q) {
            const int64_t ya = A[q], yb = B[q];
            d0 += Dx[ya]; l0 += Lx[ya];
            d1 += Dx[yb]; l1 += Lx[yb];
        }
        for (size_t t = q; t < na; ++t) { d0 += Dx[A[t]]; l0 += Lx[A[t]]; }
        for (size_t t = q; t < nb; ++t) { d1 += Dx[B[t]]; l1 += Lx[B[t]]; }
        out[0] = d0; out[1] = d1; out[2] = l0; out[3] = l1;
    }
    static double list_sum(const double *M, int64_t x, int64_t n, const std::vector<int64_t> &mem)
    {
        double s = 0;
        for (int64_t y : mem) s += M[(size_t)x * (size_t)n + (size_t)y];
        return s;
    }
    // sums over the (static) members of C[1] / C[2] when they are not candidates: computed once per item and proposal
    std::vector<double> fixedD[2], fixedL[2];
    std::vector<char> fixed_have[2];
    // lgamma(α + δ1·sz) and lgamma(ζ + δ2·sz) depend on the integer size only: memoised (same values, fewer calls)
    std::vector<double> lgA, lgZ;
    double lg_alpha_i(double sz) { const size_t k = (size_t)sz; if (lgA.size() <= k) lgA.resize(k + 64, NAN); if (lgA[k] != lgA[k]) lgA[k] = std::lgamma(c->P.alpha + c->P.delta1 * sz); return lgA[k]; }
    double lg_zeta_i(double sz) { const size_t k = (size_t)sz; if (lgZ.size() <= k) lgZ.resize(k + 64, NAN); if (lgZ[k] != lgZ[k]) lgZ[k] = std::lgamma(c->P.zeta + c->P.delta2 * sz); return lgZ[k]; }
    // the prior-ratio term log(sz+1) + log p + log(sz−1+r) − log(sz) (mcmc.jl:312-313) also depends on the size only
    std::vector<double> lprM;
    double lpr_i(double sz)
    {
        const size_t k = (size_t)sz;
        if (lprM.size() <= k) lprM.resize(k + 64, NAN);
        if (lprM[k] != lprM[k] && sz > 0) lprM[k] = std::log(sz + 1) + logp + std::log(sz - 1 + r) - std::log(sz);
        return sz > 0 ? lprM[k] : std::log(sz + 1) + logp + std::log(sz - 1 + r) - std::log(sz);
    }
    // the L2 term of a non-candidate first cluster is the same in every scan of the proposal
    std::vector<double> fixedTerm[2];

    // one scan (mcmc.jl:302-352); returns log_transition_prob
    double scan(std::vector<int64_t> &clusts, std::vector<int64_t> &sizes, const std::vector<int64_t> &items,
                const int64_t cand[2], const std::vector<int64_t> *final_clusts, int64_t scan_index)
    {
        const rc_params &P = c->P;
        const double d1 = P.delta1, d2 = P.delta2, al = P.alpha, be = P.beta, ze = P.zeta, ga = P.gamma;
        // C = findall(clustsizes .> 0), frozen at entry (mcmc.jl:273); only C[1], C[2] are ever read (Q3)
        int64_t firsts[2] = {0, 0};
        for (int64_t k = 0, f = 0; k < n && f < 2; ++k)
            if (sizes[(size_t)k] > 0) firsts[f++] = k + 1;
        if (fixed_label[0] != firsts[0] || fixed_label[1] != firsts[1] || fixed_members.size() != 2) {
            fixed_members.assign(2, {});
            for (int t = 0; t < 2; ++t) {
                fixed_label[t] = firsts[t];
                fixedD[t].assign((size_t)n, 0.0); fixedL[t].assign((size_t)n, 0.0); fixed_have[t].assign((size_t)n, 0);
                fixedTerm[t].assign((size_t)n, 0.0);
                if (firsts[t] != 0 && firsts[t] != cand[0] && firsts[t] != cand[1])
                    for (int64_t y = 0; y < n; ++y)
                        if (clusts[(size_t)y] == firsts[t]) fixed_members[(size_t)t].push_back(y);
            }
        }
        const int64_t m = (int64_t)items.size();
        double ltp = 0;
        mem[0].clear(); mem[1].clear();
        for (int64_t y : *U) {
            if (clusts[(size_t)y] == cand[0]) mem[0].push_back(y);
            else if (clusts[(size_t)y] == cand[1]) mem[1].push_back(y);
        }
        for (int64_t q = 0; q < m; ++q) {
            const int64_t x = items[(size_t)q];
            {
                std::vector<int64_t> &from = mem[clusts[(size_t)x] == cand[0] ? 0 : 1];
                from.erase(std::lower_bound(from.begin(), from.end(), x));
            }
            sizes[(size_t)clusts[(size_t)x] - 1] -= 1;                                   // mcmc.jl:303
            clusts[(size_t)x] = -1;                                                      // mcmc.jl:304
            double L1[2], lpr[2], L2p_c[2], logprobs[2], cs[4];
            cand_sums(x, cs);
            for (int k = 0; k < 2; ++k) {                                                // mcmc.jl:307-326
                const double sz = (double)sizes[(size_t)cand[k] - 1];
                const double sD = cs[k];
                const double sL = cs[2 + k];
                const double a_i = al + d1 * sz, b_i = be + sD, z_i = ze + d2 * sz, g_i = ga + sD;
                L1[k] = lg_alpha_i(sz) + abratio - a_i * std::log(b_i) + (d1 - 1) * sL - sz * lg_d1;
                lpr[k] = lpr_i(sz);
                L2p_c[k] = lg_zeta_i(sz) - z_i * std::log(g_i) + zgratio + (d2 - 1) * sL - sz * lg_d2;
            }
            double L2p_first[2];
            for (int t = 0; t < 2; ++t) {                                                // mcmc.jl:327-331
                if (firsts[t] == 0) { L2p_first[t] = 0; continue; }
                if (firsts[t] == cand[0]) { L2p_first[t] = L2p_c[0]; continue; }
                if (firsts[t] == cand[1]) { L2p_first[t] = L2p_c[1]; continue; }
                const double sz = (double)sizes[(size_t)firsts[t] - 1];
                if (!fixed_have[t][(size_t)x]) {  // members of a non-candidate cluster do not change during the proposal
                    fixedD[t][(size_t)x] = list_sum(D, x, n, fixed_members[(size_t)t]);
                    fixedL[t][(size_t)x] = list_sum(L, x, n, fixed_members[(size_t)t]);
                    fixed_have[t][(size_t)x] = 1;
                    const double sD = fixedD[t][(size_t)x], sL = fixedL[t][(size_t)x];
                    const double z_i = ze + d2 * sz, g_i = ga + sD;
                    fixedTerm[t][(size_t)x] = lg_zeta_i(sz) - z_i * std::log(g_i) + zgratio + (d2 - 1) * sL - sz * lg_d2;
                }
                L2p_first[t] = fixedTerm[t][(size_t)x];
            }
            const double L2_i = L2p_first[0] + L2p_first[1];                             // Q3
            for (int k = 0; k < 2; ++k)
                logprobs[k] = lpr[k] + (L1[k] + (P.repulsion ? (L2_i - L2p_c[k]) : 0.0)); // mcmc.jl:333-335
            int k;
            if (!final_clusts) {                                                         // mcmc.jl:336-338
                const double mn = logprobs[0] < logprobs[1] ? logprobs[0] : logprobs[1];
                logprobs[0] -= mn; logprobs[1] -= mn;                                    // utils.jl:3 mutates its argument
                const uint64_t base = 4 + (uint64_t)m + 2 * (uint64_t)m * (uint64_t)scan_index + 2 * (uint64_t)q;
                const double g0 = -std::log(-std::log(rc_uniform_mh(seed, iter, mh, base))) + logprobs[0];
                const double g1 = -std::log(-std::log(rc_uniform_mh(seed, iter, mh, base + 1))) + logprobs[1];
                k = (g1 > g0) ? 1 : 0;
            } else {
                k = ((*final_clusts)[(size_t)x] == cand[0]) ? 0 : 1;                     // mcmc.jl:340-341
            }
            clusts[(size_t)x] = cand[k];                                                 // mcmc.jl:344-345
            sizes[(size_t)cand[k] - 1] += 1;
            mem[k].insert(std::lower_bound(mem[k].begin(), mem[k].end(), x), x);
            double mn = logprobs[0] < logprobs[1] ? logprobs[0] : logprobs[1];           // mcmc.jl:348 (Q2)
            if (logprobs[0] != logprobs[0] || logprobs[1] != logprobs[1]) mn = NAN;      // minimum() propagates NaN
            const double p0 = std::exp(logprobs[0] + mn), p1 = std::exp(logprobs[1] + mn);
            ltp += std::log((k ? p1 : p0) / (p0 + p1));                                  // mcmc.jl:349-351
        }
        return ltp;
    }
};
}  // namespace

// The host part of one proposal of the MH loop of sample_labels! (src/mcmc.jl:374-473), as a pure function of a SNAPSHOT
// of the state: labels, sizes by label, K, and the exact block sums B[t][k] of that state with the slot tables they are
// indexed by.  Touches neither the device nor the context (only the HostModel: parameters and the borrowed host matrices), so the
// chain loop can run it on worker threads for several iterations at once (chain.inc.hip).  A merge is decided here
// completely — block sums are additive: B'(m, l) = B(ci, l) + B(cj, l), B'(m, m) = B(ci,ci) + B(cj,cj) + 2 B(ci,cj), so the
// merged state's log-likelihood follows from the snapshot's integers, the same ones k_blocksums would produce after
// applying the merge.  A split needs the row sums of the two new clusters: needs_device is set and the caller applies
// cfinal on the device, takes its log-likelihood and finishes the decision (finish_decision).
struct ProposalSnapshot {
    const int64_t *clusts, *sizes;   // n labels, n sizes by label
    int64_t K;
    int hi;                          // block sums: hi × hi × 4 int64, slot sizes and labels [hi]
    const int *ssize, *slabel;
    const long long *B;
};
struct ProposalResult {
    bool accept = false, split = false, skipped = false, needs_device = false;
    double log_prior_ratio = 0, log_proposal_ratio = 0, ll_cur = 0, ll_fin = 0;
    std::vector<int64_t> cfinal;     // proposed labels (filled for splits and for accepted merges)
    int32_t err = RC_OK;
    const char *errmsg = nullptr;
};

static bool finish_decision(ProposalResult &R, uint64_t seed, uint64_t iter, uint64_t mh_counter)
{
    const double x = R.log_prior_ratio + (R.ll_fin - R.ll_cur) - R.log_proposal_ratio;
    const double lar = (x != x) ? NAN : (x < 0 ? x : 0.0);                                // minimum([0, x]) propagates NaN
    const double lu = std::log(rc_uniform_mh(seed, iter, mh_counter, 2));
    R.accept = lu < lar;                                                                 // mcmc.jl:469-472
    return R.accept;
}

// lap(k): called as phase k of the proposal ends (rc_splitmerge's wall-time profile; everyone else passes a no-op)
template <class Lap>
static void proposal_core(const HostModel &M, LLCache &cache, const ProposalSnapshot &S0, double r, double p, int64_t numGibbs,
                          uint64_t seed, uint64_t iter, uint64_t mh_counter, ProposalResult &out, Lap &&lap)
{
    const int64_t n = M.n;
    const int64_t *clusts = S0.clusts, *sizes = S0.sizes;
    const int64_t K = S0.K;
    // chaperones (mcmc.jl:379)
    int64_t i = (int64_t)std::floor(rc_uniform_mh(seed, iter, mh_counter, 0) * (double)n);
    int64_t j = (int64_t)std::floor(rc_uniform_mh(seed, iter, mh_counter, 1) * (double)(n - 1));
    if (i >= n) i = n - 1;
    if (j >= n - 1) j = n - 2;
    if (j >= i) j += 1;
    const int64_t ci = clusts[(size_t)i], cj = clusts[(size_t)j];
    if (M.P.maxK > 0 && ci == cj && K >= M.P.maxK) { out.skipped = true; return; }      // mcmc.jl:384-386
    std::vector<int64_t> S, U;
    for (int64_t k = 0; k < n; ++k)
        if (clusts[(size_t)k] == ci || clusts[(size_t)k] == cj) {
            U.push_back(k);
            if (k != i && k != j) S.push_back(k);                                        // mcmc.jl:389-390
        }
    if ((uint64_t)S.size() * (uint64_t)(2 * numGibbs + 4) + 8 > 0xFFFFFFFFull) {
        out.err = RC_ERR_ARG; out.errmsg = "rc_splitmerge: uniform counter overflow (|S| * numGibbs too large)"; return;
    }
    std::vector<int64_t> claunch(clusts, clusts + n), szlaunch(sizes, sizes + n);
    if (ci == cj) {                                                                      // mcmc.jl:396-401
        int64_t e = 0;
        while (e < n && sizes[(size_t)e] != 0) ++e;
        if (e >= n) { out.err = RC_ERR_STATE; out.errmsg = "rc_splitmerge: no empty label for a split"; return; }
        claunch[(size_t)i] = e + 1;
        szlaunch[(size_t)ci - 1] -= 1;
        szlaunch[(size_t)e] += 1;
    }
    const int64_t cand[2] = {claunch[(size_t)i], claunch[(size_t)j]};                    // mcmc.jl:402
    for (size_t q = 0; q < S.size(); ++q) {                                              // mcmc.jl:403-407
        const int64_t k = S[q];
        claunch[(size_t)k] = cand[rc_uniform_mh(seed, iter, mh_counter, 4 + (uint64_t)q) < 0.5 ? 0 : 1];
        szlaunch[(size_t)clusts[(size_t)k] - 1] -= 1;
        szlaunch[(size_t)claunch[(size_t)k] - 1] += 1;
    }
    const rc_params &P = M.P;
    Restricted R;
    R.c = &M; R.D = M.D; R.L = M.L; R.n = n; R.r = r; R.p = p; R.seed = seed; R.iter = iter; R.mh = mh_counter;
    R.abratio = P.alpha * std::log(P.beta) - std::lgamma(P.alpha);                       // mcmc.jl:293-297
    R.zgratio = P.zeta * std::log(P.gamma) - std::lgamma(P.zeta);
    R.lg_d1 = std::lgamma(P.delta1); R.lg_d2 = std::lgamma(P.delta2); R.logp = std::log(p);
    R.U = &U;
    lap(1);
    for (int64_t s = 0; s < numGibbs; ++s) R.scan(claunch, szlaunch, S, cand, nullptr, s);  // mcmc.jl:411-414
    std::vector<int64_t> clusts_v;   // the merge's forced final scan wants the original labels as a vector
    if (ci == cj) {                                                                      // split, mcmc.jl:416-434
        out.split = true;
        const double ltp = R.scan(claunch, szlaunch, S, cand, nullptr, numGibbs);
        out.cfinal = claunch;
        const double sfi = (double)szlaunch[(size_t)claunch[(size_t)i] - 1], sfj = (double)szlaunch[(size_t)claunch[(size_t)j] - 1];
        const double sci = (double)sizes[(size_t)ci - 1];
        out.log_prior_ratio = std::log((double)(K + 1)) + r * std::log(1 - p) - std::log(p) - std::lgamma(r) +
                              std::lgamma(sfi - 1 + r) + std::lgamma(sfj - 1 + r) + std::log(sfi) + std::log(sfj) +
                              -(std::lgamma(sci - 1 + r) + std::log(sci));
        out.log_proposal_ratio = ltp;
    } else {                                                                             // merge, mcmc.jl:435-459
        std::vector<int64_t> szfinal = szlaunch;
        out.cfinal = claunch;
        int64_t sz_clust_i = 0;
        for (int64_t k : U)
            if (out.cfinal[(size_t)k] == ci) { out.cfinal[(size_t)k] = cj; ++sz_clust_i; }
        szfinal[(size_t)ci - 1] = 0;
        szfinal[(size_t)cj - 1] += sz_clust_i;
        const double sfj = (double)szfinal[(size_t)cj - 1], sci = (double)sizes[(size_t)ci - 1], scj = (double)sizes[(size_t)cj - 1];
        out.log_prior_ratio = -(std::log((double)K) + r * std::log(1 - p) - std::log(p) - std::lgamma(r)) +
                              std::lgamma(sfj - 1 + r) + std::log(sfj) +
                              -(std::lgamma(sci - 1 + r) + std::lgamma(scj - 1 + r) + std::log(sci) + std::log(scj));
        clusts_v.assign(clusts, clusts + n);
        const double ltp = R.scan(claunch, szlaunch, S, cand, &clusts_v, numGibbs);
        out.log_proposal_ratio = -ltp;
    }
    lap(2);
    // likelihood ratio (mcmc.jl:462-464) from the exact block sums of the snapshot
    out.ll_cur = loglik_host_c(M, cache, S0.hi, S0.ssize, S0.B, S0.slabel);
    lap(3);
    if (ci == cj) { out.needs_device = true; return; }
    const int hi = S0.hi;
    int si = -1, sj = -1;
    for (int k = 0; k < hi; ++k) {
        if (S0.ssize[k] > 0 && S0.slabel[k] == ci) si = k;
        if (S0.ssize[k] > 0 && S0.slabel[k] == cj) sj = k;
    }
    if (si < 0 || sj < 0) { out.err = RC_ERR_STATE; out.errmsg = "rc_splitmerge: internal: slots of the merged clusters not found"; return; }
    std::vector<long long> Bm(S0.B, S0.B + (size_t)hi * hi * 4);
    std::vector<int> szm(S0.ssize, S0.ssize + hi);
    for (int k = 0; k < hi; ++k)
        for (int w = 0; w < 4; ++w) Bm[((size_t)sj * hi + k) * 4 + w] += Bm[((size_t)si * hi + k) * 4 + w];
    for (int t = 0; t < hi; ++t)
        for (int w = 0; w < 4; ++w) Bm[((size_t)t * hi + sj) * 4 + w] += Bm[((size_t)t * hi + si) * 4 + w];
    szm[(size_t)sj] += szm[(size_t)si];
    szm[(size_t)si] = 0;
    out.ll_fin = loglik_host_c(M, cache, hi, szm.data(), Bm.data(), S0.slabel);   // the merged cluster keeps cj's slot and label
    lap(5);
    finish_decision(out, seed, iter, mh_counter);
    if (!out.accept) out.cfinal.clear();
}
