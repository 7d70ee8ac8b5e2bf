// Host-only planning of k_bulk_syml2's unit lists.  Plain C++17: no HIP, no globals, no environment reads — redclust_hip.hip
// includes it ahead of build_syml2_lists, which copies a plan to the device, and tests/s2plan_host.cpp includes it on its own.
//
// Column block J (S2_COLS columns) holds the rows 0 .. S2_COLS J + S2_COLS - 1 of the upper triangle.  Its first rows & ~7 rows
// are FAST units of g rows (a multiple of 8; the rest of a block is a shorter unit) — the diagonal block and the padding columns
// included: the fast path masks them.  What is left of a ragged last column block is SLOW: the round-2 unit code with its
// triangle masks, ~3x the cost per 4-row tile, so it is cut fine (RC_S2_SLOW_ROWS rows per unit).  The launch lasts as long as
// its slowest wave, so the units are dealt to the waves by cost — longest first, each to the least loaded wave — and a wave
// reads its share as a contiguous range of each list.  g is chosen for the shortest makespan.
#include <algorithm>
#include <utility>
#include <vector>

#ifndef RC_S2_SLOW_ROWS
#define RC_S2_SLOW_ROWS 16
#endif
constexpr int S2_COLS = 128;

struct S2Unit { int x, y, z, w; };   // (first column of the block, first row, end row, 0): the int4 the kernels read

struct S2Plan {
    std::vector<S2Unit> fast, slow;  // grouped by wave (stable: heavy column blocks first inside a wave)
    std::vector<int> wfast, wslow;   // [4 cap_blocks + 1] offsets of each wave's units in the two lists
    int g = 0;                       // rows per fast unit
    long long makespan = 0;          // load of the busiest wave, in tile costs
};

// The plan for n points and cap_blocks resident 4-wave blocks.  sw_coarse > 0 fixes g (rounded up to a multiple of 8) instead of
// searching 16..256; slow_factor is the cost of a slow 4-row tile in fast ones.
static inline S2Plan s2_plan(int n, int cap_blocks, int sw_coarse, int slow_factor)
{
    const int ncb = (n + S2_COLS - 1) / S2_COLS, nwaves = 4 * cap_blocks;
    struct Unit { S2Unit u; int cost; bool fast; };
    auto make_units = [&](int g, std::vector<Unit> &out) {
        out.clear();
        for (int J = ncb - 1; J >= 0; --J) {
            const int c0 = J * S2_COLS, rows = std::min(c0 + S2_COLS, n);
            const int fast_rows = rows & ~7;
            for (int a0 = 0; a0 < fast_rows; a0 += g) {
                const int a1 = std::min(a0 + g, fast_rows);
                out.push_back({{c0, a0, a1, 0}, (a1 - a0) / 4 + 2, true});
            }
            for (int a0 = fast_rows; a0 < rows; a0 += RC_S2_SLOW_ROWS) {
                const int a1 = std::min(a0 + RC_S2_SLOW_ROWS, rows);
                out.push_back({{c0, a0, a1, 0}, slow_factor * ((a1 - a0 + 3) / 4) + 3, false});
            }
        }
    };
    auto schedule = [&](const std::vector<Unit> &units, std::vector<int> &owner) -> long long {   // longest first, to the least loaded wave
        std::vector<int> order(units.size());
        for (size_t q = 0; q < order.size(); ++q) order[q] = (int)q;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return units[(size_t)x].cost > units[(size_t)y].cost; });
        std::vector<std::pair<long long, int>> heap;                   // (load, wave), min-heap
        heap.reserve((size_t)nwaves);
        for (int w = 0; w < nwaves; ++w) heap.push_back({0, w});
        auto cmp = [](const std::pair<long long, int> &x, const std::pair<long long, int> &y) { return x > y; };
        std::make_heap(heap.begin(), heap.end(), cmp);
        owner.assign(units.size(), 0);
        long long makespan = 0;
        for (int q : order) {
            std::pop_heap(heap.begin(), heap.end(), cmp);
            auto &top = heap.back();
            owner[(size_t)q] = top.second;
            top.first += units[(size_t)q].cost;
            makespan = std::max(makespan, top.first);
            std::push_heap(heap.begin(), heap.end(), cmp);
        }
        return makespan;
    };
    std::vector<Unit> units, best_units;
    std::vector<int> owner, best_owner;
    S2Plan p;
    p.makespan = -1;
    p.g = 64;
    const int g_lo = sw_coarse > 0 ? (sw_coarse + 7) / 8 * 8 : 16, g_hi = sw_coarse > 0 ? g_lo : 256;
    for (int g = g_lo; g <= g_hi; g += 8) {
        make_units(g, units);
        const long long mk = schedule(units, owner);
        if (p.makespan < 0 || mk < p.makespan || (mk == p.makespan && g > p.g)) { p.makespan = mk; p.g = g; best_units = units; best_owner = owner; }
    }
    // group by wave, fast and slow lists apart
    p.wfast.assign((size_t)nwaves + 1, 0); p.wslow.assign((size_t)nwaves + 1, 0);
    for (size_t q = 0; q < best_units.size(); ++q) (best_units[q].fast ? p.wfast : p.wslow)[(size_t)best_owner[q] + 1]++;
    for (int w = 0; w < nwaves; ++w) { p.wfast[(size_t)w + 1] += p.wfast[(size_t)w]; p.wslow[(size_t)w + 1] += p.wslow[(size_t)w]; }
    p.fast.resize((size_t)p.wfast[(size_t)nwaves]); p.slow.resize((size_t)p.wslow[(size_t)nwaves]);
    std::vector<int> pf(p.wfast.begin(), p.wfast.end() - 1), ps(p.wslow.begin(), p.wslow.end() - 1);
    for (size_t q = 0; q < best_units.size(); ++q) {
        const int w = best_owner[q];
        if (best_units[q].fast) p.fast[(size_t)pf[(size_t)w]++] = best_units[q].u; else p.slow[(size_t)ps[(size_t)w]++] = best_units[q].u;
    }
    return p;
}
