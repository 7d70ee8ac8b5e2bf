// Stand-alone run of csrc/hostmodel.inc.hpp — the model's host statistics as the library ships them — without a device
// (tests/test_hostmodel_cpu.py builds it with the host compiler, under the sanitizers where they exist, runs it on a case file
// it wrote and holds every printed line against the C oracle).
//
// The case file is flat binary: int64 n, numGibbs, seed, iterations, proposals per iteration, eD, eL; double r, p; the bytes of
// rc_params; D and logD (n×n doubles); their fixed-point copies Dq and Lq (n×n int64, exponents eD / eL); the start labels
// (n int64, 1-based).  The program walks the proposals in "intended" semantics, as rc_splitmerge does: a snapshot of its own
// state with the block sums k_blocksums would give — formed here by brute force from Dq / Lq — goes to proposal_core; a split's
// proposed state gets its block sums the same way, loglik_host_c for ll_fin, and finish_decision; an accepted proposal replaces
// the state.  One line per proposal: "p accept split skipped log_prior_ratio log_proposal_ratio ll_cur logprior K labels…",
// ll_cur being the log-likelihood of the state before the proposal, logprior, K and the labels those of the state after it.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#define __host__
#define __device__
#define __forceinline__
#include "../redclust.jl_amd/csrc/hostmodel.inc.hpp"

// labels (1-based, by point) with the slot tables a context would hold for them: a cluster keeps its slot while it lives, a new
// one takes the lowest free slot, hi is the high-water mark
struct State {
    std::vector<int64_t> clusts, sizes;
    int64_t K = 0;
    int hi = 0;
    std::vector<int> ssize, slabel;      // [kcap]
    std::vector<long long> B;            // hi × hi × 4
};

static void set_labels(State &S, const std::vector<int64_t> &z, int kcap)
{
    const size_t n = z.size();
    S.clusts = z;
    S.sizes.assign(n, 0);
    for (int64_t l : z) S.sizes[(size_t)l - 1] += 1;
    S.ssize.resize((size_t)kcap, 0); S.slabel.resize((size_t)kcap, 0);
    for (int k = 0; k < kcap; ++k) {     // deaths free their slot
        if (S.slabel[(size_t)k] > 0 && S.sizes[(size_t)S.slabel[(size_t)k] - 1] == 0) S.slabel[(size_t)k] = 0;
        S.ssize[(size_t)k] = 0;
    }
    S.K = 0;
    for (size_t l = 1; l <= n; ++l) {
        if (S.sizes[l - 1] == 0) continue;
        ++S.K;
        int k = 0;
        while (k < kcap && S.slabel[(size_t)k] != (int)l) ++k;
        if (k == kcap) {
            k = 0;
            while (k < kcap && S.slabel[(size_t)k] != 0) ++k;
            if (k == kcap) { std::printf("FAILED: more clusters than slots\n"); std::exit(1); }
            S.slabel[(size_t)k] = (int)l;
        }
        S.ssize[(size_t)k] = (int)S.sizes[l - 1];
        S.hi = std::max(S.hi, k + 1);
    }
}

// k_blocksums by brute force: B[(t·hi + k)·4 + {0, 1, 2, 3}] = Σ_{i in slot k} of the (hi, lo) halves of the row sums
// Σ_{j in slot t} Dq[i][j] and Σ_{j in slot t} Lq[i][j] — j = i included, each row sum split at RC_LO_BITS on its own
static void block_sums(State &S, const std::vector<int64_t> &Dq, const std::vector<int64_t> &Lq)
{
    const size_t n = S.clusts.size();
    const int hi = S.hi;
    std::vector<int> slot_of_label(n + 1, -1), slot(n);
    for (int k = 0; k < hi; ++k)
        if (S.slabel[(size_t)k] > 0) slot_of_label[(size_t)S.slabel[(size_t)k]] = k;
    for (size_t i = 0; i < n; ++i) slot[i] = slot_of_label[(size_t)S.clusts[i]];
    S.B.assign((size_t)hi * hi * 4, 0);
    const long long mask = ((long long)1 << RC_LO_BITS) - 1;
    std::vector<long long> sd((size_t)hi), sl((size_t)hi);
    for (size_t i = 0; i < n; ++i) {
        std::fill(sd.begin(), sd.end(), 0); std::fill(sl.begin(), sl.end(), 0);
        for (size_t j = 0; j < n; ++j) { sd[(size_t)slot[j]] += Dq[i * n + j]; sl[(size_t)slot[j]] += Lq[i * n + j]; }
        for (int t = 0; t < hi; ++t) {
            long long *e = &S.B[((size_t)t * hi + slot[i]) * 4];
            e[0] += sd[(size_t)t] >> RC_LO_BITS; e[1] += sd[(size_t)t] & mask;
            e[2] += sl[(size_t)t] >> RC_LO_BITS; e[3] += sl[(size_t)t] & mask;
        }
    }
}

template <class T>
static std::vector<T> take(std::FILE *f, size_t count)
{
    std::vector<T> v(count);
    if (std::fread(v.data(), sizeof(T), count, f) != count) { std::printf("FAILED: case file too short\n"); std::exit(1); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: hostmodel_host <case file>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("FAILED: cannot open %s\n", argv[1]); return 1; }
    const std::vector<int64_t> head = take<int64_t>(f, 7);
    const int64_t n = head[0], numGibbs = head[1], iters = head[3], nmh = head[4];
    const uint64_t seed = (uint64_t)head[2];
    const std::vector<double> rp = take<double>(f, 2);
    const double r = rp[0], p = rp[1];
    const std::vector<rc_params> P = take<rc_params>(f, 1);
    const size_t nn = (size_t)n * (size_t)n;
    const std::vector<double> D = take<double>(f, nn), logD = take<double>(f, nn);
    const std::vector<int64_t> Dq = take<int64_t>(f, nn), Lq = take<int64_t>(f, nn), init = take<int64_t>(f, (size_t)n);
    std::fclose(f);

    // the scans read the library's own log matrix (rc_attach_host_matrices without a logD), which has to be the caller's bit for bit
    std::vector<double> ownL(nn);
    host_log_matrix(D.data(), n, ownL.data());
    if (std::memcmp(ownL.data(), logD.data(), nn * sizeof(double)) != 0) { std::printf("FAILED: host_log_matrix differs from the case's logD\n"); return 1; }

    const int kcap = (int)std::min<int64_t>(n, 128);   // (a context's first capacity)
    const HostModel M{P[0], n, (int)head[5], (int)head[6], kcap, D.data(), ownL.data()};
    LLCache cache;
    State S;
    set_labels(S, init, kcap);
    block_sums(S, Dq, Lq);
    for (int64_t it = 0; it < iters; ++it)
        for (int64_t mh = 0; mh < nmh; ++mh) {
            const ProposalSnapshot S0{S.clusts.data(), S.sizes.data(), S.K, S.hi, S.ssize.data(), S.slabel.data(), S.B.data()};
            ProposalResult R;
            proposal_core(M, cache, S0, r, p, numGibbs, seed, (uint64_t)it, (uint64_t)mh, R, [](int) {});
            if (R.err != RC_OK) { std::printf("FAILED: %s\n", R.errmsg); return 1; }
            // (a skipped proposal returns before its likelihoods: the line still carries the state's)
            if (R.skipped) R.ll_cur = loglik_host_c(M, cache, S.hi, S.ssize.data(), S.B.data(), S.slabel.data());
            if (R.needs_device) {                                // split: what the device would be asked for
                State T = S;
                set_labels(T, R.cfinal, kcap);
                block_sums(T, Dq, Lq);
                R.ll_fin = loglik_host_c(M, cache, T.hi, T.ssize.data(), T.B.data(), T.slabel.data());
                if (finish_decision(R, seed, (uint64_t)it, (uint64_t)mh)) S = std::move(T);
            } else if (R.accept) {                               // merge: decided by proposal_core from the snapshot's sums
                set_labels(S, R.cfinal, kcap);
                block_sums(S, Dq, Lq);
            }
            std::printf("p %d %d %d %.17g %.17g %.17g %.17g %" PRId64, (int)R.accept, (int)R.split, (int)R.skipped, R.log_prior_ratio,
                        R.log_proposal_ratio, R.ll_cur, logprior_host(M, S.ssize.data(), S.slabel.data(), r, p), S.K);
            for (int64_t l : S.clusts) std::printf(" %" PRId64, l);
            std::printf("\n");
        }
    std::printf("ok %" PRId64 "\n", iters * nmh);
    return 0;
}
