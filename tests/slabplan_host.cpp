// Stand-alone check of csrc/slabplan.inc.hpp (tests/test_slabplan_cpu.py builds it with the host compiler, under the sanitizers
// where they exist, and runs it).  For every case the chunks are planned the way the four entry points call the planner and
// checked by brute force — every labelling in exactly one chunk, no chunk above its caps unless it is a single labelling, no
// chunk that the next labelling would still have fitted, the rows of a chunk within the workspace — and printed as
// "plan <key> <ms:qc*repeats,...>" for the test to hold against tests/golden/slab_plans.json.  Ends with "ok <cases>" and
// returns 0, or prints the first failure and returns 1.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../redclust.jl_amd/csrc/slabplan.inc.hpp"

#define REQUIRE(cond)                                                                                    \
    do {                                                                                                 \
        if (!(cond)) { std::printf("FAILED %s (line %d, %s, chunk at %lld)\n", #cond, __LINE__, key.c_str(), (long long)s0); return false; } \
    } while (0)

constexpr size_t PERM_BYTES = (size_t)1 << 29;

// what an entry point passes for its chunks; side(K) and side_cap as in the header
struct Entry {
    int64_t ms_cap, rows, qt;
    size_t fixed, per_labelling, side_cap;
    size_t (*side)(size_t K, size_t n);   // null: none (the planner's short form)
};

static bool check_case(const std::string &key, const Entry &e, const std::vector<int> &K, size_t n, size_t workspace)
{
    const int64_t L = (int64_t)K.size();
    std::string rle;
    int64_t last_ms = -1, last_qc = -1, repeats = 0;
    const auto flush = [&] { if (repeats) rle += (rle.empty() ? "" : ",") + std::to_string(last_ms) + ":" + std::to_string(last_qc) + "*" + std::to_string(repeats); };
    for (int64_t s0 = 0; s0 < L;) {
        const auto side_of = [&](size_t k) { return e.side ? e.side(k, n) : (size_t)0; };
        const SlabChunk c = e.side ? slab_plan(s0, K.data(), L, e.ms_cap, e.fixed, e.per_labelling, e.rows, e.qt, workspace, side_of, e.side_cap)
                                   : slab_plan(s0, K.data(), L, e.ms_cap, e.fixed, e.per_labelling, e.rows, e.qt, workspace);
        REQUIRE(c.ms >= 1 && c.ms <= e.ms_cap && s0 + c.ms <= L);
        REQUIRE(c.qc >= 1 && c.qc <= e.rows);
        size_t bytes = e.fixed, side = 0;
        for (int64_t s = s0; s < s0 + c.ms; ++s) { bytes += 16 * (size_t)K[s] + e.per_labelling; side += side_of((size_t)K[s]); }
        REQUIRE(c.ms == 1 || (bytes * (size_t)e.qt <= workspace && side <= e.side_cap));
        REQUIRE(c.qc == 1 || bytes * (size_t)c.qc <= workspace);
        REQUIRE(c.qc == e.rows || bytes * (size_t)(c.qc + 1) > workspace);
        if (s0 + c.ms < L && c.ms < e.ms_cap) {                           // the next labelling did not fit
            const size_t k = (size_t)K[s0 + c.ms];
            REQUIRE((bytes + 16 * k + e.per_labelling) * (size_t)e.qt > workspace || side + side_of(k) > e.side_cap);
        }
        if (c.ms != last_ms || c.qc != last_qc) { flush(); last_ms = c.ms; last_qc = c.qc; repeats = 0; }
        ++repeats;
        s0 += c.ms;
    }
    flush();
    std::printf("plan %s %s\n", key.c_str(), rle.c_str());
    return true;
}

int main()
{
    int cases = 0;
    for (int64_t n : {1, 65, 257, 8192})
        for (int64_t L : {1, 3, 65, 1025})
            for (int pattern = 0; pattern < 3; ++pattern) {                // all 1; all min(n, 4096); alternating 1 / sqrt(n)
                std::vector<int> K((size_t)L);
                int Kmax = 1;
                for (int64_t s = 0; s < L; ++s) {
                    K[(size_t)s] = pattern == 0 ? 1 : pattern == 1 ? (int)std::min<int64_t>(n, 4096) : (s % 2 ? (int)std::sqrt((double)n) : 1);
                    Kmax = std::max(Kmax, K[(size_t)s]);
                }
                for (size_t kib : {4, 64, 1024, 1024 * 1024}) {
                    const size_t w = kib << 10, N = (size_t)n;
                    const std::string tail = std::to_string(n) + "," + std::to_string(L) + "," + std::to_string(pattern) + "," + std::to_string(kib);
                    const int64_t qt = std::min<int64_t>(n, 512);
                    // rc_score_labellings: a labelling's blocks within a quarter of the workspace
                    const Entry score{slab_ms_cap(PERM_BYTES, 4, n), n, qt, 16 * N, 0, w / 4, [](size_t k, size_t) { return 32 * (k * (k + 1) / 2); }};
                    // rc_cluster_profiles: a labelling's per-point results and medoids within half of it
                    const Entry profiles{slab_ms_cap(PERM_BYTES, 4, n), n, qt, 16 * N, 0, w / 2, [](size_t k, size_t n_) { return 24 * n_ + 16 * k; }};
                    if (!check_case("score," + tail, score, K, N, w) || !check_case("profiles," + tail, profiles, K, N, w)) return 1;
                    cases += 2;
                    for (int64_t q : {1, 3, 600}) {
                        // rc_predict, without and with the scores_out and sums_out columns at Kmax = max K
                        for (int tab = 0; tab < 2; ++tab) {
                            const size_t per = 16 + (tab ? 8 * ((size_t)Kmax + 1) + 16 * (size_t)Kmax : 0);
                            const Entry predict{slab_ms_cap(PERM_BYTES, 2, n), q, std::min<int64_t>(q, 512), 16 * N, per, 0, nullptr};
                            if (!check_case("predict," + tail + "," + std::to_string(q) + "," + std::to_string(tab), predict, K, N, w)) return 1;
                        }
                        // rc_predict_joint: all q points together, their base sums within the workspace
                        const Entry joint{slab_ms_cap(PERM_BYTES, 2, n), q, q, 0, 0, 0, nullptr};
                        if (!check_case("joint," + tail + "," + std::to_string(q), joint, K, N, w)) return 1;
                        cases += 3;
                    }
                }
            }
    std::printf("ok %d\n", cases);
    return 0;
}
