// Stand-alone check of csrc/s2plan.inc.hpp (tests/test_s2plan_cpu.py builds it with the host compiler, under the sanitizers where
// they exist, and runs it).  Every plan is checked by brute force — each row of each column block of the upper triangle in exactly
// one unit, fast units on 8-row boundaries, slow units short, the wave offsets monotone — and its 64-bit FNV-1a hash is printed as
// "plan <n> <cap_blocks> <sw_coarse> <hash>", for the test to hold against tests/golden/s2_plans.json.  Ends with "ok <cases>" and
// returns 0, or prints the first failure and returns 1.
#include <cstdint>
#include <cstdio>

#include "../redclust.jl_amd/csrc/s2plan.inc.hpp"

#define REQUIRE(cond)                                                                                                     \
    do {                                                                                                                  \
        if (!(cond)) { std::printf("FAILED %s (line %d, n = %d, cap_blocks = %d, sw_coarse = %d)\n", #cond, __LINE__, n, cap, sw); return false; } \
    } while (0)

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void add(int v) { for (int b = 0; b < 4; ++b) { h ^= ((uint32_t)v >> (8 * b)) & 0xffu; h *= 0x100000001b3ull; } }   // little-endian bytes
    void add(const std::vector<S2Unit> &u) { add((int)u.size()); for (const S2Unit &q : u) { add(q.x); add(q.y); add(q.z); add(q.w); } }
    void add(const std::vector<int> &v) { add((int)v.size()); for (int q : v) add(q); }
};

static bool offsets_ok(const std::vector<int> &w, size_t nwaves, size_t total)
{
    if (w.size() != nwaves + 1 || w.front() != 0 || (size_t)w.back() != total) return false;
    for (size_t q = 0; q + 1 < w.size(); ++q) if (w[q] > w[q + 1]) return false;
    return true;
}

static bool check_case(int n, int cap, int sw)
{
    const S2Plan p = s2_plan(n, cap, sw, 3);
    const int ncb = (n + S2_COLS - 1) / S2_COLS;
    const auto rows_of = [&](int J) { return std::min(S2_COLS * J + S2_COLS, n); };
    std::vector<std::vector<int>> seen((size_t)ncb);
    for (int J = 0; J < ncb; ++J) seen[(size_t)J].assign((size_t)rows_of(J), 0);
    const auto mark = [&](const S2Unit &u) {
        if (u.x < 0 || u.x % S2_COLS != 0 || u.x / S2_COLS >= ncb || u.w != 0) return false;
        const int J = u.x / S2_COLS;
        if (!(0 <= u.y && u.y < u.z && u.z <= rows_of(J))) return false;
        for (int r = u.y; r < u.z; ++r) seen[(size_t)J][(size_t)r]++;
        return true;
    };
    REQUIRE(p.g > 0 && p.g % 8 == 0);
    for (const S2Unit &u : p.fast) {
        REQUIRE(mark(u));
        REQUIRE(u.y % 8 == 0 && u.z % 8 == 0 && u.z <= (rows_of(u.x / S2_COLS) & ~7) && u.z - u.y <= p.g);
    }
    for (const S2Unit &u : p.slow) {
        REQUIRE(mark(u));
        REQUIRE(u.z - u.y <= RC_S2_SLOW_ROWS);
    }
    for (int J = 0; J < ncb; ++J)
        for (int r = 0; r < rows_of(J); ++r) REQUIRE(seen[(size_t)J][(size_t)r] == 1);
    REQUIRE(offsets_ok(p.wfast, 4 * (size_t)cap, p.fast.size()));
    REQUIRE(offsets_ok(p.wslow, 4 * (size_t)cap, p.slow.size()));
    Fnv f;
    f.add(p.g); f.add(p.fast); f.add(p.slow); f.add(p.wfast); f.add(p.wslow);
    std::printf("plan %d %d %d %016llx\n", n, cap, sw, (unsigned long long)f.h);
    return true;
}

int main()
{
    int cases = 0;
    for (int n : {1, 7, 8, 127, 128, 129, 135, 1000, 2561, 8192})
        for (int cap : {4, 2 * 256, 3 * 256})
            for (int sw : {0, 24}) {
                if (!check_case(n, cap, sw)) return 1;
                ++cases;
            }
    std::printf("ok %d\n", cases);
    return 0;
}
