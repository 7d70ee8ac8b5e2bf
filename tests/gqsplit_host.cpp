// csrc/gqsplit.inc.hpp on the host alone (tests/test_visearch_large_resources.py builds this under ASan / UBSan): hi(x) as the
// kernel evaluates it against Gq[x] >> 32 at every x of rc_vi_gtable's table (visearch.inc.hip gtable), and the refusals.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../redclust.jl_amd/csrc/gqsplit.inc.hpp"

using namespace visearch;

#define REQUIRE(c) do { if (!(c)) { std::printf("failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    const int64_t N = GQ_SPLIT_NMAX;
    std::vector<int64_t> G((size_t)N, 0);
    for (int64_t x = 1; x < N; ++x) {
        const double d = (double)x;
        G[(size_t)x] = (int64_t)std::llrint(std::ldexp(std::log(d + 1.0) + d * std::log1p(1.0 / d), 32));
    }
    GqSplit s;
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)4, (int64_t)8, (int64_t)8192, (int64_t)22027, (int64_t)22028, N}) {
        REQUIRE(build_gq_split(G.data(), n, s) == GQ_SPLIT_OK);
        for (int64_t x = 0; x < n; ++x) REQUIRE((int64_t)split_hi(s, (unsigned)x) == (G[(size_t)x] >> 32));
    }
    REQUIRE(s.count == GQ_THR_MAX);
    std::printf("thresholds");
    for (int t = 1; t <= s.count; ++t) std::printf(" %d", (int)s.thr[t]);
    std::printf("\n");
    REQUIRE(build_gq_split(G.data(), 0, s) == GQ_SPLIT_SIZE && build_gq_split(G.data(), N + 1, s) == GQ_SPLIT_SIZE);
    std::vector<int64_t> B(G.begin(), G.begin() + 100);
    B[50] = B[49] - 1;
    REQUIRE(build_gq_split(B.data(), 100, s) == GQ_SPLIT_ORDER);
    B[50] = G[50]; B[99] = (int64_t)12 << 32;
    REQUIRE(build_gq_split(B.data(), 100, s) == GQ_SPLIT_RANGE);
    B[99] = G[99];
    for (int x = 3; x < 7; ++x) B[(size_t)x] = (int64_t)3 << 32;     // still non-decreasing; the thresholds of 2·2^32 and 3·2^32 are both x = 3
    REQUIRE(build_gq_split(B.data(), 100, s) == GQ_SPLIT_OCTAVE);
    return 0;
}
