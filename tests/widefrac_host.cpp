// csrc/widefrac.inc.hpp on the host, on its own: reads lines "T m P X1 A1 X2 A2" and prints, per line, num and den of the two
// candidates as limbs (hi as a signed, lo as an unsigned 64-bit integer) and the comparison's verdict.  tests/test_widefrac_cpu.py
// builds it with g++ (under ASan / UBSan where they link) and holds every line to fractions.Fraction.
#include <cstdio>

#include "../redclust.jl_amd/csrc/widefrac.inc.hpp"

int main()
{
    long long T, m, P;
    unsigned long long X[2];
    unsigned A[2];
    while (std::scanf("%lld %lld %lld %llu %u %llu %u", &T, &m, &P, &X[0], &A[0], &X[1], &A[1]) == 7) {
        const widefrac::Step s = widefrac::make_step(T, m, P);
        widefrac::Frac f[2];
        for (int k = 0; k < 2; ++k) {
            f[k] = widefrac::fraction(s, X[k], A[k]);
            std::printf("%lld %llu %lld %llu ", (long long)(f[k].num >> 64), (unsigned long long)f[k].num, (long long)(f[k].den >> 64),
                        (unsigned long long)f[k].den);
        }
        std::printf("%d\n", widefrac::compare(f[0], f[1]));
    }
    return 0;
}
