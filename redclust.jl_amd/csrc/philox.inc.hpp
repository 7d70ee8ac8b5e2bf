// Philox4x32-10 and the domain tags of the library's random streams, host and device: included by redclust_hip.hip where the
// generator has always stood (ahead of the sweep's rc_uniform) and by hostmodel.inc.hpp, and through it, with __host__,
// __device__ and __forceinline__ defined away, by the CPU program of the host model (tests/hostmodel_host.cpp, built and run by
// tests/test_hostmodel_cpu.py).  Nothing but integer arithmetic.
#pragma once

typedef unsigned long long u64;   // (the translation unit's own typedef, repeated for a consumer that has nothing else of it)

// ---------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., Random123): the one generator behind every stream of the library, host and device.  A
// stream is a counter layout plus a domain tag XORed into the high key word (seed_hi); the sweep's stream (rc_uniform:
// counter (pos, i, sweep_lo, sweep_hi), key = seed; include/redclust_hip.h) has none.
// ---------------------------------------------------------------------------------------------------
#define RC_MH_TAG 0x4D485F52u     // "MH_R": split–merge proposals (rc_uniform_mh, host), counter (draw, mh, iter_lo, iter_hi)
#define RC_RP_TAG 0x52505F5Fu     // "RP__": scalar r / p updates (chain::Stream, host), counter (draw, kind, iter_lo, iter_hi)
#define RC_KMED_TAG 0x4B4D4544u   // "KMED": k-medoids++ seeding, counter (step, k, 0, 0)
#define RC_KMN_TAG 0x4B4D4E53u    // "KMNS": k-means draws, counter (draw, k, 0, 0)
#define RC_SK_TAG 0x534D504Bu     // "SMPK": sampleK's Gumbel noise, counter (K, i_lo, i_hi, 0)

struct Philox4 { unsigned w0, w1, w2, w3; };

__host__ __device__ __forceinline__ constexpr Philox4 rc_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                                unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * (u64)c0, p1 = (u64)0xCD9E8D57u * (u64)c2;   // (one 32 x 32 -> 64 multiply each)
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}
// the top 53 bits of (w0, w1) as an integer; the top 52 as a double in (0, 1): (bits + 0.5)·2^-52
__host__ __device__ __forceinline__ constexpr u64 rc_bits53(Philox4 x) { return (((u64)x.w0 << 32) | x.w1) >> 11; }
__host__ __device__ __forceinline__ constexpr double rc_unit52(Philox4 x) { return ((double)((((u64)x.w0 << 32) | x.w1) >> 12) + 0.5) * 0x1p-52; }

constexpr bool rc_philox_is(Philox4 x, unsigned a, unsigned b, unsigned c, unsigned d) { return x.w0 == a && x.w1 == b && x.w2 == c && x.w3 == d; }
static_assert(rc_philox_is(rc_philox(0, 0, 0, 0, 0, 0), 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u), "Random123 known answer");
static_assert(rc_philox_is(rc_philox(~0u, ~0u, ~0u, ~0u, ~0u, ~0u), 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu), "Random123 known answer");
static_assert(rc_philox_is(rc_philox(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u), 0xd16cfe09u, 0x94fdccebu,
                           0x5001e420u, 0x24126ea1u), "Random123 known answer");
