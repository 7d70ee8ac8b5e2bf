"""NumPy restatement of rc_predict's contract (include/redclust_hip.h, DESIGN.md §8 "Predict") — TEST INFRASTRUCTURE.

Per new point: its row of D and of logD quantised by the oracle's own rule (orc_quant_exponent / orc_quantize on the row);
per sample: exact integer sums by np.add.at, the stable score with math.log / math.log1p in the order of the oracle's
stable_score, the oracle's uniforms (orc_uniform with the "PRED" tag in the seed's high word) and a first-index argmax over
the candidates in ascending label order with the new cluster last.  Also the fixed inputs of the GPU tests, so that the
CPU suite can check the reference's decision gaps on exactly those."""
from __future__ import annotations

import functools
import math

import numpy as np

import oracle_lib as O

TAG = 0x50524544 << 32
M64 = 0xFFFFFFFFFFFFFFFF


def quantise_rows(Dnew, logDnew, n):
    """(Dq, Lq, eD, eL): per-row exponents 62 - ex - ceil(log2 n) and q = llrint(ldexp(x, e))."""
    L = O.lib()
    Dnew = np.ascontiguousarray(Dnew, dtype=np.float64)
    logDnew = np.ascontiguousarray(logDnew, dtype=np.float64)
    q = Dnew.shape[0]
    Dq, Lq = np.empty((q, n), np.int64), np.empty((q, n), np.int64)
    eD, eL = np.empty(q, np.int32), np.empty(q, np.int32)
    for i in range(q):
        eD[i] = L.orc_quant_exponent(n, Dnew[i], n)
        eL[i] = L.orc_quant_exponent(n, logDnew[i], n)
        L.orc_quantize(Dnew[i], n, int(eD[i]), Dq[i])
        L.orc_quantize(logDnew[i], n, int(eL[i]), Lq[i])
    return Dq, Lq, eD, eL


def score_point(Dq_i, Lq_i, eD, eL, z, r, p, P, A):
    """One (sample, new point): candidate labels ascending (+ 0 when a new cluster is offered), the integer sums (K×2), the
    noise-free scores and T, the sum of the absolute values of every score's terms."""
    n = len(z)
    sD, sL = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    np.add.at(sD, z, Dq_i)
    np.add.at(sL, z, Lq_i)
    sizes = np.bincount(z, minlength=n + 1)
    labs = np.flatnonzero(sizes)
    K = len(labs)
    scD, scL = math.ldexp(1.0, -int(eD)), math.ldexp(1.0, -int(eL))
    rep = bool(P.get("repulsion", True))
    cL = (P["delta1"] - 1) - ((P["delta2"] - 1) if rep else 0.0)
    logp = math.log(p)
    scores, T = [], []
    for k in labs:
        s = int(sizes[k])
        SD, SL = float(int(sD[k])) * scD, float(int(sL[k])) * scL
        lsr = math.log(float(s) - 1 + r)
        base = A[s] + (logp + lsr)
        t1 = (P["alpha"] + P["delta1"] * float(s)) * math.log1p(SD / P["beta"])
        lik = cL * SL - t1
        t2 = 0.0
        if rep:
            t2 = (P["zeta"] + P["delta2"] * float(s)) * math.log1p(SD / P["gamma"])
            lik += t2
        scores.append(base + lik)
        T.append(abs(A[s]) + abs(logp) + abs(lsr) + abs(cL * SL) + abs(t1) + abs(t2))
    cands = [int(k) for k in labs]
    maxK = int(P.get("maxK", 0))
    if maxK == 0 or K < maxK:
        a, b = math.log(float(K + 1)), r * math.log(1 - p)
        scores.append(a + b)
        T.append(abs(a) + abs(b))
        cands.append(0)
    return np.array(cands, np.int64), np.stack([sD[labs], sL[labs]], axis=1), np.array(scores), np.array(T)


def _first_argmax(v):
    best = 0
    for t in range(1, len(v)):
        if v[t] > v[best]:
            best = t
    return best


def _gap(v):
    if len(v) < 2:
        return math.inf
    w = np.sort(np.asarray(v))
    return float(w[-1] - w[-2])


def draw(cands, scores, seed, s, i):
    """(drawn label, MAP label, gap of the two best noisy scores, gap of the two best noise-free scores); s and i are the
    counters: sample_offset + sample index, point_offset + point index."""
    L = O.lib()
    noisy = []
    for c, v in zip(cands, scores):
        u = L.orc_uniform((int(seed) ^ TAG) & M64, int(s) & M64, int(i) & M64, int(c))
        noisy.append(v + (-math.log(-math.log(u))))
    return int(cands[_first_argmax(noisy)]), int(cands[_first_argmax(scores)]), _gap(noisy), _gap(scores)


def predict_ref(Dnew, logDnew, samples, r, p, P, seed, sample_offset=0, point_offset=0):
    """The whole call.  labels, map (m×q); eD, eL (q); K (m); sums (m×q×Kmax×2, zero beyond K_s); scores and T
    (m×q×(Kmax+1): NaN beyond K_s, column Kmax the new cluster, -inf when not offered); min_gap_noisy, min_gap_map."""
    samples = np.ascontiguousarray(samples, dtype=np.int64)
    m, n = samples.shape
    q = len(Dnew)
    Dq, Lq, eD, eL = quantise_rows(Dnew, logDnew, n)
    A = O.size_table(P, n)
    K = np.array([len(np.unique(z)) for z in samples])
    Kmax = int(K.max())
    labels, mp = np.zeros((m, q), np.int64), np.zeros((m, q), np.int64)
    sums = np.zeros((m, q, Kmax, 2), np.int64)
    scores = np.full((m, q, Kmax + 1), np.nan)
    T = np.zeros((m, q, Kmax + 1))
    gn, gm = math.inf, math.inf
    for s in range(m):
        for i in range(q):
            c, sm, sc, tt = score_point(Dq[i], Lq[i], eD[i], eL[i], samples[s], float(r[s]), float(p[s]), P, A)
            k = int(K[s])
            sums[s, i, :k] = sm
            scores[s, i, :k] = sc[:k]
            T[s, i, :k] = tt[:k]
            scores[s, i, Kmax] = sc[k] if len(sc) > k else -math.inf
            T[s, i, Kmax] = tt[k] if len(tt) > k else 0.0
            labels[s, i], mp[s, i], a, b = draw(c, sc, seed, sample_offset + s, point_offset + i)
            gn, gm = min(gn, a), min(gm, b)
    return dict(labels=labels, map=mp, eD=eD, eL=eL, K=K, Kmax=Kmax, sums=sums, scores=scores, T=T, min_gap_noisy=gn, min_gap_map=gm)


# ---------------------------------------------------------------------------------------------------------------
# The fixed inputs of the GPU tests (tests/test_gpu_predict.py); tests/test_predict_cpu.py checks the reference's gaps on them.
# ---------------------------------------------------------------------------------------------------------------
PARAMS = dict(delta1=2.0, delta2=3.0, alpha=9.0, beta=4.0, zeta=12.0, gamma=30.0, eta=1.0, sigma=1.0, u=1.0, v=1.0, repulsion=True,
              maxK=0)
EDGE_SHAPES = [(1, 1, 1), (63, 3, 2), (64, 2, 65), (65, 2, 63), (257, 3, 1025)]


def random_case(n, q, m, seed, maxK=0, sample_offset=0, point_offset=0, last_scale=1.0, **params):
    """q×n distances (the last new point's scaled by last_scale), m labellings of n points (sample 0: all singletons; sample 1:
    one cluster, named n; the rest 1..12 random label names), r, p; params override PARAMS."""
    rng = np.random.default_rng(seed)
    Dnew = rng.gamma(2.0, 1.0, size=(q, n)) + 0.05
    Dnew[q - 1] *= last_scale
    S = np.empty((m, n), np.int64)
    for s in range(m):
        if s == 0:
            S[s] = rng.permutation(n) + 1
        elif s == 1:
            S[s] = n
        else:
            kk = int(rng.integers(1, min(n, 12) + 1))
            names = rng.choice(n, size=kk, replace=False) + 1
            S[s] = names[rng.integers(0, kk, size=n)]
    P = dict(PARAMS, maxK=maxK, **params)
    return dict(Dnew=Dnew, logDnew=np.log(Dnew), samples=S, r=rng.uniform(0.5, 3.0, m), p=rng.uniform(0.1, 0.9, m), P=P,
                seed=1000 + seed, sample_offset=sample_offset, point_offset=point_offset)


@functools.lru_cache(maxsize=None)
def edge_case(n, q, m):
    """maxK = 4 except where noted: among the random samples some have fewer clusters (a new one is offered), some exactly 4
    (maxK reached) and some more; (1, 1, 1) and (64, 2, 65) run with maxK = 0.  With PARAMS and these distances no draw opens a
    cluster, so (64, 2, 65) swaps the deltas and moves its last point far away (it opens one in most samples) and (65, 2, 63)
    runs without repulsion with its last point close by (it opens one in about half of those that offer it); (65, 2, 63)
    also starts its sample counter just below 2^32, so the counter's high word changes inside the call."""
    if (n, q, m) == (64, 2, 65):
        return random_case(n, q, m, seed=n * 7 + m, maxK=0, last_scale=40.0, delta1=3.0, delta2=2.0)
    if (n, q, m) == (65, 2, 63):
        return random_case(n, q, m, seed=n * 7 + m, maxK=4, last_scale=0.02, repulsion=False, sample_offset=(1 << 32) - 3, point_offset=7)
    return random_case(n, q, m, seed=n * 7 + m, maxK=0 if n == 1 else 4)


@functools.lru_cache(maxsize=None)
def independence_case():
    return random_case(100, 5, 70, seed=5070, maxK=0)


def _ref_of(c):
    return predict_ref(c["Dnew"], c["logDnew"], c["samples"], c["r"], c["p"], c["P"], c["seed"], c["sample_offset"], c["point_offset"])


@functools.lru_cache(maxsize=None)
def edge_ref(n, q, m):
    return _ref_of(edge_case(n, q, m))


@functools.lru_cache(maxsize=None)
def independence_ref():
    return _ref_of(independence_case())


@functools.lru_cache(maxsize=None)
def frequency_case():
    """One new point, one sample of three clusters of four: its scores, the softmax, and the reference's 20 000 draws."""
    lab = np.repeat(np.arange(1, 4), 4).astype(np.int64)
    X = np.eye(3)[lab - 1] + 0.45 * np.random.default_rng(3).standard_normal((12, 3))
    y = np.array([0.4, 0.35, 0.25])
    Dnew = np.sqrt(((y[None, :] - X) ** 2).sum(axis=1))[None, :]
    return dict(Dnew=Dnew, logDnew=np.log(Dnew), labels=lab, r=1.5, p=0.3, P=dict(PARAMS), seed=99, m=20000)


@functools.lru_cache(maxsize=None)
def frequency_ref():
    """(candidate labels, softmax of the scores, the reference's drawn counts per candidate, smallest noisy gap)"""
    c = frequency_case()
    Dq, Lq, eD, eL = quantise_rows(c["Dnew"], c["logDnew"], 12)
    cands, _, sc, _ = score_point(Dq[0], Lq[0], eD[0], eL[0], c["labels"], c["r"], c["p"], c["P"], O.size_table(c["P"], 12))
    w = np.exp(sc - sc.max())
    counts = np.zeros(len(cands), np.int64)
    gap = math.inf
    for s in range(c["m"]):
        lab, _, g, _ = draw(cands, sc, c["seed"], s, 0)
        counts[list(cands).index(lab)] += 1
        gap = min(gap, g)
    return cands, w / w.sum(), counts, gap


def within_4_sigma(counts, prob, m):
    """every candidate with expected count >= 100 lies within 4 sigma of it"""
    ok = True
    for c, pr in zip(counts, prob):
        if m * pr >= 100:
            ok = ok and abs(c - m * pr) <= 4 * math.sqrt(m * pr * (1 - pr))
    return ok


@functools.lru_cache(maxsize=None)
def holdout_case():
    """Planted: N = 150 in K = 3 groups around the unit vectors (sigma 0.2); the last 30 observations are held out and one far
    point (3, 3, 3) is added; the samples are the true training labels twice."""
    import np_transcription as T
    rng = np.random.default_rng(11)
    N, K = 150, 3
    truth = rng.integers(0, K, size=N)
    X = np.eye(3)[truth] + 0.2 * rng.standard_normal((N, 3))
    tr, new = X[:120], np.vstack([X[120:], [[3.0, 3.0, 3.0]]])
    lab = (truth[:120] + 1).astype(np.int64)
    Dtr = np.sqrt(((tr[:, None, :] - tr[None, :, :]) ** 2).sum(axis=2))
    P = T.likelihood_hyperparams(Dtr, lab)
    Dnew = np.sqrt(((new[:, None, :] - tr[None, :, :]) ** 2).sum(axis=2))
    return dict(points=tr, new_points=new, truth_new=(truth[120:] + 1).astype(np.int64), samples=np.stack([lab, lab]),
                r=np.array([1.5, 2.0]), p=np.array([0.3, 0.5]), P=P, seed=0, Dnew=Dnew, logDnew=np.log(Dnew))


@functools.lru_cache(maxsize=None)
def holdout_ref():
    c = holdout_case()
    return predict_ref(c["Dnew"], c["logDnew"], c["samples"], c["r"], c["p"], c["P"], c["seed"])
