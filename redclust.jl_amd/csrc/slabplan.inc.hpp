// Host-only planning of the chunks of labellings of the slab driver (slab.inc.hip).  Plain C++17: no HIP, no globals, no
// environment reads, no allocation — redclust_hip.hip includes it ahead of slab.inc.hip, and tests/slabplan_host.cpp includes it
// on its own.
//
// A chunk is a run of labellings (posterior samples, for predict) whose sorted orders are built and uploaded together, and a
// number of rows (context rows, or new points) that then go through k_predict_sums at once.  Per row a chunk costs `fixed`
// device bytes plus, per labelling, its K slots' sums (16 bytes each) and `per_labelling` more; labellings are taken while qt
// rows of them fit the workspace, while there are fewer than ms_cap of them, and while what the chunk keeps beside the rows
// — side(K) bytes per labelling — stays within side_cap.  The first labelling of a chunk always goes.
#include <algorithm>
#include <cstddef>
#include <cstdint>

struct SlabChunk { int64_t ms, qc; };   // labellings s0 .. s0 + ms - 1; their rows in chunks of at most qc

// the most labellings whose sorted orders, entry_bytes per point and labelling padded to 64 labellings, fit perm_bytes (>= 64)
static inline int64_t slab_ms_cap(size_t perm_bytes, size_t entry_bytes, int64_t n)
{
    return std::max<int64_t>(64, (int64_t)(perm_bytes / entry_bytes / (size_t)n) / 64 * 64);
}

// The chunk that starts at labelling s0 of `count`, K their cluster counts; rows: all the rows there are (qc never exceeds it).
template <typename Side>
static inline SlabChunk slab_plan(int64_t s0, const int *K, int64_t count, int64_t ms_cap, size_t fixed, size_t per_labelling,
                                  int64_t rows, int64_t qt, size_t workspace, Side side, size_t side_cap)
{
    size_t bytes = fixed, side_bytes = 0;
    int64_t ms = 0;
    while (s0 + ms < count && ms < ms_cap) {
        const size_t k = (size_t)K[s0 + ms], add = 16 * k + per_labelling, sd = side(k);
        if (ms > 0 && ((bytes + add) * (size_t)qt > workspace || side_bytes + sd > side_cap)) break;
        bytes += add; side_bytes += sd; ++ms;
    }
    return {ms, std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t)(workspace / bytes)))};
}

// ... of a caller that keeps nothing beside the rows
static inline SlabChunk slab_plan(int64_t s0, const int *K, int64_t count, int64_t ms_cap, size_t fixed, size_t per_labelling,
                                  int64_t rows, int64_t qt, size_t workspace)
{
    return slab_plan(s0, K, count, ms_cap, fixed, per_labelling, rows, qt, workspace, [](size_t) { return (size_t)0; }, 0);
}
