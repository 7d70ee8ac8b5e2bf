// The split of the exact searches' fixed-point table for the large-n kernels (visearch_large.inc.hip; DESIGN.md §8 "Exact expected
// VI search, large n").  Plain C++17: no HIP, no globals — tests/gqsplit_host.cpp includes it on its own and runs it under ASan /
// UBSan.  The device reads octave_entry through the same text (VIS_HD is __host__ __device__ under hipcc).
//
// For x <= 32767 Gq[x] < 12·2^32 and Gq is non-decreasing, so Gq[x] = lo[x] + 2^32·hi(x) with lo the low word and
//   hi(x) = Gq[x] >> 32 = #{t >= 1 : x >= thr[t]},   thr[t] = the smallest x with Gq[x] >= t·2^32.
// Proof: Gq non-decreasing makes {x : Gq[x] >= t·2^32} an up-set [thr[t], ∞), and Gq[x] >> 32 counts the t >= 1 with
// t·2^32 <= Gq[x].  The thresholds are read off the table itself, so the identity holds for whatever llrint and libm gave.
// Since Gq[x] ≈ (log x + 1)·2^32 rises by log 2 < 1 units of 2^32 per doubling of x, at most one threshold has any given bit
// length; the builder checks that too, and then with b = the bit length of x
//   hi(x) = base[b] + (x >= cut[b]),   base[b] = #{t : bitlength(thr[t]) < b},  cut[b] = the threshold of bit length b (none: 0xFFFF),
// which is what the kernel evaluates per table cell: one count-leading-zeros, one 16-entry LDS word, one compare.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define VIS_HD __host__ __device__
#else
#define VIS_HD
#endif

namespace visearch {

constexpr int GQ_THR_MAX = 11;        // Gq[32767] < 12·2^32
constexpr int64_t GQ_SPLIT_NMAX = 32768;   // table entries: x <= 32767 has a bit length of at most 15

struct GqSplit {
    int count;                                 // thresholds in use: thr[1..count], ascending
    unsigned short thr[GQ_THR_MAX + 1];        // thr[0] unused
};

VIS_HD inline int bit_length(unsigned x)
{
    int b = 0;
    while (x) { ++b; x >>= 1; }
    return b;
}

// (cut << 4) | base of bit length b (0..15), see above
VIS_HD inline unsigned octave_entry(const GqSplit &s, int b)
{
    unsigned base = 0, cut = 0xFFFFu;
#pragma unroll
    for (int t = 1; t <= GQ_THR_MAX; ++t) {          // (a fixed trip count: the device indexes thr[] with constants)
        const int bt = bit_length(s.thr[t]);
        if (t <= s.count && bt < b) ++base;
        else if (t <= s.count && bt == b) cut = s.thr[t];
    }
    return (cut << 4) | base;
}

// hi(x) as the kernel evaluates it
VIS_HD inline unsigned split_hi(const GqSplit &s, unsigned x)
{
    const unsigned e = octave_entry(s, bit_length(x));
    return (e & 15u) + (x >= (e >> 4) ? 1u : 0u);
}

enum GqSplitError { GQ_SPLIT_OK = 0, GQ_SPLIT_SIZE, GQ_SPLIT_ORDER, GQ_SPLIT_RANGE, GQ_SPLIT_OCTAVE };

// The thresholds of Gq[0..n-1].  Refused: n outside 1..32768; a negative or decreasing entry; an entry of 12·2^32 or more;
// two thresholds of one bit length (a step of two units at one x included)
inline GqSplitError build_gq_split(const int64_t *Gq, int64_t n, GqSplit &out)
{
    out = GqSplit{};
    if (n < 1 || n > GQ_SPLIT_NMAX) return GQ_SPLIT_SIZE;
    int64_t prev = 0;
    for (int64_t x = 0; x < n; ++x) {
        const int64_t g = Gq[x];
        if (g < prev) return GQ_SPLIT_ORDER;
        prev = g;
        const int64_t hi = g >> 32;
        if (hi > GQ_THR_MAX) return GQ_SPLIT_RANGE;
        while (out.count < hi) out.thr[++out.count] = (unsigned short)x;
    }
    for (int t = 2; t <= out.count; ++t)
        if (bit_length(out.thr[t]) == bit_length(out.thr[t - 1])) return GQ_SPLIT_OCTAVE;
    return GQ_SPLIT_OK;
}

}  // namespace visearch
