"""NumPy restatement of rc_predict_joint's contract (include/redclust_hip.h, DESIGN.md §8 "Joint predict") — TEST INFRASTRUCTURE.

Per new point: its extended row (Dnew[i] followed by Dnn[i], the diagonal entry 0) and the row of its logarithms quantised by the
oracle's own rule (orc_quant_exponent / orc_quantize with n + q addends); per visit: exact integer sums by np.add.at over the
training points and the other allocated new points, the stable score with math.log / math.log1p in the order of the oracle's
stable_score, the oracle's uniforms (orc_uniform with the "PRDJ" tag in the seed's high word, the visit index where the sweep has
the point) and a first-index argmax over the candidates in ascending label order with the new cluster last.  Also the fixed
inputs of the GPU tests, so that the CPU suite can check the reference's decision gaps and what the inputs claim to cover."""
from __future__ import annotations

import functools
import math

import numpy as np

import oracle_lib as O
import predict_ref as R

TAG = 0x5052444A << 32
M64 = 0xFFFFFFFFFFFFFFFF
PARAMS = R.PARAMS


def quantise_rows(Dnew, Dnn, logDnew, logDnn):
    """(Dq, Lq, eD, eL): q×(n+q) int64 rows, column n+i of row i zero, and the exponents 62 - ex - ceil(log2(n+q)) per row.
    The leading rows of the blocks alone may be given (k×n and k×q): a row is quantised by itself."""
    L = O.lib()
    Dnew, Dnn = np.asarray(Dnew, dtype=np.float64), np.asarray(Dnn, dtype=np.float64)
    q, n = Dnew.shape
    N = n + Dnn.shape[1]
    rows = np.ascontiguousarray(np.concatenate([Dnew, Dnn], axis=1))
    lrows = np.ascontiguousarray(np.concatenate([np.asarray(logDnew, dtype=np.float64), np.asarray(logDnn, dtype=np.float64)], axis=1))
    for i in range(q):
        rows[i, n + i] = 0.0
        lrows[i, n + i] = 0.0
    Dq, Lq = np.empty((q, N), np.int64), np.empty((q, N), np.int64)
    eD, eL = np.empty(q, np.int32), np.empty(q, np.int32)
    for i in range(q):
        eD[i] = L.orc_quant_exponent(N, rows[i], N)
        eL[i] = L.orc_quant_exponent(N, lrows[i], N)
        L.orc_quantize(rows[i], N, int(eD[i]), Dq[i])
        L.orc_quantize(lrows[i], N, int(eL[i]), Lq[i])
    return Dq, Lq, eD, eL


def log_blocks(Dnew, Dnn):
    """NumPy's logarithms of both blocks, the diagonal of the second 0"""
    Dn = np.array(Dnn, dtype=np.float64)
    np.fill_diagonal(Dn, 1.0)
    return np.log(Dnew), np.log(Dn)


def visit_scores(i, z, y, Dq_i, Lq_i, eD, eL, r, p, P, A):
    """One visit of new point i under training labels z (n) and the new points' labels y (q, 0 = unallocated; y[i] is removed
    first): candidate labels ascending (+ 0 when a new cluster is offered), the label a new cluster would take, the integer
    sums (K_i×2) and the noise-free scores."""
    n, q = len(z), len(y)
    N = n + q
    others = np.flatnonzero(y > 0)
    others = others[others != i]
    sD, sL = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)
    np.add.at(sD, z, Dq_i[:n])
    np.add.at(sL, z, Lq_i[:n])
    np.add.at(sD, y[others], Dq_i[n + others])
    np.add.at(sL, y[others], Lq_i[n + others])
    sizes = np.bincount(z, minlength=N + 1) + np.bincount(y[others], minlength=N + 1)
    labs = np.flatnonzero(sizes)
    K = len(labs)
    scD, scL = math.ldexp(1.0, -int(eD)), math.ldexp(1.0, -int(eL))
    rep = bool(P.get("repulsion", True))
    cL = (P["delta1"] - 1) - ((P["delta2"] - 1) if rep else 0.0)
    logp = math.log(p)
    scores = []
    for k in labs:
        s = int(sizes[k])
        SD, SL = float(int(sD[k])) * scD, float(int(sL[k])) * scL
        base = A[s] + (logp + math.log(float(s) - 1 + r))
        lik = cL * SL - (P["alpha"] + P["delta1"] * float(s)) * math.log1p(SD / P["beta"])
        if rep:
            lik += (P["zeta"] + P["delta2"] * float(s)) * math.log1p(SD / P["gamma"])
        scores.append(base + lik)
    cands = [int(k) for k in labs]
    maxK = int(P.get("maxK", 0))
    newlab = int(np.flatnonzero(sizes[1:] == 0)[0]) + 1                # findfirst(clustsizes .== 0)
    if maxK == 0 or K < maxK:
        scores.append(math.log(float(K + 1)) + r * math.log(1 - p))
        cands.append(0)
    return np.array(cands, np.int64), newlab, np.stack([sD[labs], sL[labs]], axis=1), np.array(scores)


def draw(cands, scores, seed, sc, v):
    """(index of the drawn candidate, gap of the two best noisy scores); sc: the sample counter, v: the visit index"""
    L = O.lib()
    noisy = [x + (-math.log(-math.log(L.orc_uniform((int(seed) ^ TAG) & M64, int(sc) & M64, int(v), int(c))))) for c, x in zip(cands, scores)]
    best = 0
    for t in range(1, len(noisy)):
        if noisy[t] > noisy[best]:
            best = t
    gap = math.inf
    if len(noisy) > 1:
        w = np.sort(np.asarray(noisy))
        gap = float(w[-1] - w[-2])
    return best, gap


def predict_joint_ref(Dnew, Dnn, logDnew, logDnn, samples, r, p, P, sweeps, seed, sample_offset=0):
    """The whole call: labels, first (m×q), K (m), moves (m×(sweeps+1)), sums (m×q×2), eD, eL (q), min_gap_noisy — and what
    happened on the way, per sample: closed_midway (a pass in which the new cluster was offered at one visit and, maxK reached,
    not at a later one), reused (a Gibbs pass in which a cluster of new points alone died and a point that was elsewhere
    opened a cluster under the freed label), new_only (a cluster without a training point exists at the end)."""
    samples = np.ascontiguousarray(samples, dtype=np.int64)
    m, n = samples.shape
    q = len(Dnew)
    Dq, Lq, eD, eL = quantise_rows(Dnew, Dnn, logDnew, logDnn)
    A = O.size_table(P, n + q)
    labels, first = np.zeros((m, q), np.int64), np.zeros((m, q), np.int64)
    K = np.zeros(m, np.int64)
    moves = np.zeros((m, sweeps + 1), np.int64)
    sums = np.zeros((m, q, 2), np.int64)
    closed, reused, new_only = np.zeros(m, bool), np.zeros(m, bool), np.zeros(m, bool)
    gap = math.inf
    for s in range(m):
        z = samples[s]
        y = np.zeros(q, np.int64)
        for ps in range(sweeps + 1):
            offered_before, died = False, set()
            for i in range(q):
                old = int(y[i])
                if old and not np.any(z == old) and np.count_nonzero(y == old) == 1:
                    died.add(old)
                cands, newlab, sm, sc = visit_scores(i, z, y, Dq[i], Lq[i], eD[i], eL[i], float(r[s]), float(p[s]), P, A)
                offered = cands[-1] == 0
                closed[s] |= offered_before and not offered
                offered_before |= offered
                t, g = draw(cands, sc, seed, sample_offset + s, ps * q + i)
                gap = min(gap, g)
                new = int(cands[t]) if cands[t] != 0 else newlab
                sums[s, i] = sm[t] if cands[t] != 0 else 0
                if new != old:
                    moves[s, ps] += 1
                    if ps > 0 and cands[t] == 0 and new in died:
                        reused[s] = True
                y[i] = new
            if ps == 0:
                first[s] = y
        labels[s] = y
        K[s] = len(np.unique(np.concatenate([z, y])))
        new_only[s] = bool(np.any(~np.isin(y, z)))
    return dict(labels=labels, first=first, K=K, moves=moves, sums=sums, eD=eD, eL=eL, min_gap_noisy=gap, closed_midway=closed,
                reused=reused, new_only=new_only)


# ---------------------------------------------------------------------------------------------------------------
# The fixed inputs of the GPU tests (tests/test_gpu_predict_joint.py); tests/test_predict_joint_cpu.py checks the reference's
# gaps on them and that they contain what they claim.
# ---------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(1, 1, 1, 0), (1, 2, 2, 2), (63, 3, 2, 1), (64, 64, 3, 2), (65, 65, 5, 2), (40, 257, 2, 1), (257, 3, 1025, 2)]


def random_case(n, q, m, sweeps, seed, maxK=0, sample_offset=0, far=1.0, among=1.0, **params):
    """q×n distances of the new points to the training points (scaled by far), q×q symmetric distances among them (scaled by
    among), m labellings of n points (sample 0: all singletons; sample 1: one cluster, named n; the rest 1..12 random label
    names), r, p; params override PARAMS."""
    rng = np.random.default_rng(seed)
    Dnew = (rng.gamma(2.0, 1.0, size=(q, n)) + 0.05) * far
    U = (rng.gamma(2.0, 1.0, size=(q, q)) + 0.05) * among
    Dnn = np.triu(U, 1) + np.triu(U, 1).T
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
    logDnew, logDnn = log_blocks(Dnew, Dnn)
    return dict(Dnew=Dnew, Dnn=Dnn, logDnew=logDnew, logDnn=logDnn, samples=S, r=rng.uniform(0.5, 3.0, m), p=rng.uniform(0.1, 0.9, m),
                P=P, sweeps=sweeps, seed=2000 + seed, sample_offset=sample_offset)


@functools.lru_cache(maxsize=None)
def edge_case(n, q, m, sweeps):
    """Where new points lie far from the training points and at moderate distances from each other (far, among) and the
    deltas are swapped, new points open clusters, join each other's, and leave them again in the Gibbs passes.
    (64, 64, 3, 2): maxK = 0, such points; (65, 65, 5, 2): the same without repulsion, maxK = 9, so that clusters born in the
    call close the offer, and a sample counter that starts just below 2^32; (40, 257, 2, 1): more new points than a workgroup
    has threads, plain PARAMS; (257, 3, 1025, 2): maxK = 4 around the samples' own cluster counts."""
    sd = n * 7 + q * 3 + m
    if (n, q) == (64, 64):
        return random_case(n, q, m, sweeps, seed=sd, maxK=0, far=40.0, among=4.0, delta1=3.0, delta2=2.0)
    if (n, q) == (65, 65):
        return random_case(n, q, m, sweeps, seed=sd, maxK=9, far=40.0, among=4.0, delta1=3.0, delta2=2.0, repulsion=False,
                           sample_offset=(1 << 32) - 3)
    if (n, q) == (40, 257):
        return random_case(n, q, m, sweeps, seed=sd, maxK=0)
    if (n, q) == (257, 3):
        return random_case(n, q, m, sweeps, seed=sd, maxK=4, far=6.0, among=2.0)
    return random_case(n, q, m, sweeps, seed=sd, maxK=0, far=8.0 if n == 1 else 1.0)


def _ref_of(c):
    return predict_joint_ref(c["Dnew"], c["Dnn"], c["logDnew"], c["logDnn"], c["samples"], c["r"], c["p"], c["P"], c["sweeps"], c["seed"],
                             c["sample_offset"])


@functools.lru_cache(maxsize=None)
def edge_ref(n, q, m, sweeps):
    return _ref_of(edge_case(n, q, m, sweeps))


@functools.lru_cache(maxsize=None)
def split_case():
    """70 samples, run whole, as 64 + 6, and one per launch"""
    return random_case(100, 5, 70, 2, seed=5070, maxK=0, far=20.0, among=3.0, delta1=3.0, delta2=2.0)


@functools.lru_cache(maxsize=None)
def split_ref():
    return _ref_of(split_case())


@functools.lru_cache(maxsize=None)
def frequency_case():
    """predict_ref.frequency_case's sample (three clusters of four) and two new points close to each other and away from the
    rest; sweeps = 0; 20 000 sample counters."""
    lab = np.repeat(np.arange(1, 4), 4).astype(np.int64)
    X = np.eye(3)[lab - 1] + 0.45 * np.random.default_rng(3).standard_normal((12, 3))
    Y = np.array([[1.5, 1.5, 1.5], [1.6, 1.45, 1.5]])
    Dnew = np.sqrt(((Y[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    Dnn = np.sqrt(((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2))
    logDnew, logDnn = log_blocks(Dnew, Dnn)
    return dict(Dnew=Dnew, Dnn=Dnn, logDnew=logDnew, logDnn=logDnn, labels=lab, r=1.5, p=0.3, P=dict(PARAMS), seed=99, m=20000)


@functools.lru_cache(maxsize=None)
def frequency_ref():
    """(outcomes (y_1, y_2) as label pairs, their exact probabilities p(y_1 | z)·p(y_2 | z, y_1) from the reference's own
    scores, the reference's counts over the m sample counters, smallest noisy gap)"""
    c = frequency_case()
    z, P = c["labels"], c["P"]
    Dq, Lq, eD, eL = quantise_rows(c["Dnew"], c["Dnn"], c["logDnew"], c["logDnn"])
    A = O.size_table(P, 14)

    def visit(i, y):
        cands, newlab, _, sc = visit_scores(i, z, np.array(y, np.int64), Dq[i], Lq[i], eD[i], eL[i], c["r"], c["p"], P, A)
        w = np.exp(sc - sc.max())
        return cands, [int(k) if k else newlab for k in cands], sc, w / w.sum()

    c1, l1, s1, p1 = visit(0, [0, 0])
    second = {a: visit(1, [a, 0]) for a in l1}
    outcomes, prob = [], []
    for a, pa in zip(l1, p1):
        for b, pb in zip(second[a][1], second[a][3]):
            outcomes.append((a, b))
            prob.append(pa * pb)
    counts = {o: 0 for o in outcomes}
    gap = math.inf
    for s in range(c["m"]):
        t, g1 = draw(c1, s1, c["seed"], s, 0)
        c2, l2, s2, _ = second[l1[t]]
        u, g2 = draw(c2, s2, c["seed"], s, 1)
        counts[(l1[t], l2[u])] += 1
        gap = min(gap, g1, g2)
    return outcomes, np.array(prob), np.array([counts[o] for o in outcomes]), gap


@functools.lru_cache(maxsize=None)
def holdout_case():
    """Planted: 120 training points in three groups around the unit vectors (sigma 0.2) and 30 new points in random order, 18
    from those groups and 12 from a fourth group around (1.2, 1.2, 1.2) that the training data do not contain; the samples are
    the true training labels, five times."""
    import np_transcription as T
    rng = np.random.default_rng(21)
    truth = rng.integers(0, 3, size=120)
    tr = np.eye(3)[truth] + 0.2 * rng.standard_normal((120, 3))
    tnew = np.r_[rng.integers(0, 3, size=18), np.full(12, 3)]
    tnew = tnew[rng.permutation(30)]
    centres = np.vstack([np.eye(3), [[1.2, 1.2, 1.2]]])
    new = centres[tnew] + 0.2 * rng.standard_normal((30, 3))
    lab = (truth + 1).astype(np.int64)
    Dtr = np.sqrt(((tr[:, None, :] - tr[None, :, :]) ** 2).sum(axis=2))
    P = T.likelihood_hyperparams(Dtr, lab)
    Dnew = np.sqrt(((new[:, None, :] - tr[None, :, :]) ** 2).sum(axis=2))
    Dnn = np.sqrt(((new[:, None, :] - new[None, :, :]) ** 2).sum(axis=2))
    logDnew, logDnn = log_blocks(Dnew, Dnn)
    m = 5
    return dict(points=tr, new_points=new, truth_new=(tnew + 1).astype(np.int64), unseen=tnew == 3, samples=np.stack([lab] * m),
                r=np.full(m, 1.5), p=np.full(m, 0.3), P=P, sweeps=2, seed=0, sample_offset=0, Dnew=Dnew, Dnn=Dnn, logDnew=logDnew,
                logDnn=logDnn)


@functools.lru_cache(maxsize=None)
def holdout_ref():
    return _ref_of(holdout_case())
