"""NumPy restatement of sampleK's device draw (csrc/samplek.inc.hip, rc_sample_k; src/prior.jl:316-338 and the Gumbel-max
draw of src/utils.jl:2-6), written from DESIGN.md §8 (TEST INFRASTRUCTURE):

    lp[K] = (r·K)·log(1-p) + (n-K)·log(p) - log(n-K) - logbeta(r·K, n-K)   for K < n,   lp[n] = r·n·log(1-p),
    logbeta(a, b) = gammaln(a) + gammaln(b) - gammaln(a + b),
    K_i = first argmax_K (-log(-log u_K) + lp[K]);  K = 1 when no score exceeds -inf,

u_K from Philox4x32-10 keyed (seed_lo, seed_hi ^ "SMPK"), counter (K, i_lo, i_hi, 0), u = (52 bits + 0.5)·2^-52."""
from __future__ import annotations

import numpy as np
from scipy.special import gammaln

M32 = np.uint64(0xFFFFFFFF)
SMPK = 0x534D504B


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (32-bit words held in uint64), one key."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2   # 32 x 32 -> 64 bits: no wrap
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def uniforms(seed: int, K, i: int):
    """u of candidates K (1-based, array) of sample i."""
    K = np.asarray(K, dtype=np.uint64)
    z = np.zeros_like(K)
    c = philox4x32_10(K, z + np.uint64(i & 0xFFFFFFFF), z + np.uint64((i >> 32) & 0xFFFFFFFF), z,
                      seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ SMPK)
    bits = ((c[0] << np.uint64(32)) | c[1]) >> np.uint64(12)
    return (bits.astype(np.float64) + 0.5) * 2.0 ** -52


def logprobs(n: int, r: float, p: float):
    """lp[K - 1] for K = 1..n, in the reference's order of operations."""
    K = np.arange(1, n + 1, dtype=np.float64)
    a = r * K
    with np.errstate(divide="ignore", invalid="ignore"):
        l1p, lgp = np.log(1.0 - p), np.log(p)
        b = n - K[:-1]
        lb = (gammaln(a[:-1]) + gammaln(b)) - gammaln(a[:-1] + b)
        lp = np.empty(n)
        lp[:-1] = ((a[:-1] * l1p + b * lgp) - np.log(b)) - lb
        lp[-1] = a[-1] * l1p
    return lp


def draw(n: int, r: float, p: float, seed: int, i: int):
    """(K, gap): sample i's K and the gap between its two largest scores (inf when n = 1 or fewer than two are finite)."""
    with np.errstate(invalid="ignore"):
        sc = -np.log(-np.log(uniforms(seed, np.arange(1, n + 1), i))) + logprobs(n, r, p)
    ok = sc > -np.inf
    if not ok.any():
        return 1, np.inf
    v = np.where(ok, sc, -np.inf)
    K = int(np.argmax(v)) + 1
    top = np.sort(v[ok])[::-1]
    return K, (top[0] - top[1]) if len(top) > 1 else np.inf
