// The exact fraction of the PEAR search where its numerator and denominator pass 64 bits (pointsearch_large.inc.hip, k_pear_large;
// DESIGN.md §8 "PEAR search, large n").  Plain C++17 with the compiler's 128-bit integers: no HIP, no globals, no floating
// point — tests/widefrac_host.cpp includes it on its own and runs it under ASan / UBSan against Python's fractions; the device
// evaluates the same text (WF_HD is __host__ __device__ under hipcc).
//
// With T = n(n−1)/2, P = Σ_{i<j} C_ij, and X, A of a labelling (include/redclust_hip.h):
//   num = 2·(T·X − A·P),   den = T·(m·A + P) − 2·A·P = T·P + (T·m − 2·P)·A.
// Bounds under the entries' capacity n <= 32767, m·n < 2^31:
//   T = n(n−1)/2 < 2^29;  0 <= A <= T;  0 <= X, P <= m·T = (m·n)·(n−1)/2 < 2^31·2^14 = 2^45;
//   T·X, A·P <= T·m·T < 2^74, so |num| < 2^75;
//   |T·m − 2·P| <= T·m < 2^45 (0 <= P <= m·T), T·P < 2^74, so den < 2^74 + 2^74 = 2^75; and den >= 0: with A <= T and P <= m·T,
//   den = T·m·A − A·P + P·(T − A) = A·(m·T − P) + P·(T − A), a sum of two products of non-negative factors;
//   a cross product |num₁|·den₂ < 2^150: three 64-bit limbs hold it with room to spare.
// A fraction whose den is 0 stands for 0/1 (n = 1, or P = 0 or P = m·T with a labelling to match), as in greedy::fraction.
// Per run T, m and P are fixed (Step), so a candidate is the pair (X, A) — 96 bits — and num, den are rebuilt from it where two
// candidates are compared.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define WF_HD __host__ __device__
#else
#define WF_HD
#endif

namespace widefrac {

using i128 = __int128;
using u128 = unsigned __int128;

// what a run's fractions share: T, P, T·m − 2·P and T·P
struct Step {
    long long T, P, coef;
    u128 TP;
};

WF_HD inline Step make_step(long long T, long long m, long long P) { return Step{T, P, T * m - 2 * P, (u128)T * (u128)P}; }

struct Frac {
    i128 num;
    u128 den;   // > 0
};

WF_HD inline Frac fraction(const Step &s, unsigned long long X, unsigned A)
{
    const i128 den = (i128)s.TP + (i128)s.coef * (i128)A;
    if (den == 0) return Frac{0, 1};
    return Frac{2 * ((i128)s.T * (i128)X - (i128)s.P * (i128)A), (u128)den};
}

struct U192 {
    unsigned long long lo, mid, hi;   // (named limbs, not an array: the device keeps them in registers)
};

// a·b for a, b < 2^96 whose product is below 2^192 (here: below 2^150)
WF_HD inline U192 mul(u128 a, u128 b)
{
    const unsigned long long a0 = (unsigned long long)a, a1 = (unsigned long long)(a >> 64);
    const unsigned long long b0 = (unsigned long long)b, b1 = (unsigned long long)(b >> 64);
    const u128 low = (u128)a0 * b0;
    const u128 mid = (u128)a1 * b0 + (u128)a0 * b1 + (low >> 64);   // three terms below 2^96 each
    return U192{(unsigned long long)low, (unsigned long long)mid, (unsigned long long)(mid >> 64) + a1 * b1};
}

// −1, 0, 1: x below, equal to, above y — x.num·y.den against y.num·x.den by sign and magnitude
WF_HD inline int compare(const Frac &x, const Frac &y)
{
    const bool nx = x.num < 0, ny = y.num < 0;
    if (nx != ny) return nx ? -1 : 1;
    const U192 l = mul((u128)(nx ? -x.num : x.num), y.den), r = mul((u128)(ny ? -y.num : y.num), x.den);
    const int c = l.hi != r.hi ? (l.hi < r.hi ? -1 : 1) : l.mid != r.mid ? (l.mid < r.mid ? -1 : 1) : l.lo != r.lo ? (l.lo < r.lo ? -1 : 1) : 0;
    return nx ? -c : c;
}

}  // namespace widefrac
