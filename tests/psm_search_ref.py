"""NumPy restatement of the point-estimate search (DESIGN.md §8 "Point-estimate search", include/redclust_hip.h
rc_psm_search): a plain loop, test infrastructure only.  Binder runs are exact integers, so the device has to reproduce
them bit for bit; VI runs decide on host logarithms and pin properties, not trajectories."""
import numpy as np

import greedy_search_ref
from greedy_search_ref import sortlabels  # noqa: F401  (the tests take it from here)

BINDER, VILB = 0, 1


def planted_counts(n, m, K, noise, seed):
    """m samples: a planted partition with K clusters, a `noise` share of the points relabelled at random per sample.
    Returns (samples m×n int64 in 1..K, counts n×n uint32 = Σ_s adjacency(sample_s))."""
    rng = np.random.default_rng(seed)
    truth = rng.integers(1, K + 1, size=n)
    samples = np.tile(truth, (m, 1)).astype(np.int64)
    for s in range(m):
        flip = rng.random(n) < noise
        samples[s, flip] = rng.integers(1, K + 1, size=int(flip.sum()))
    counts = np.zeros((n, n), np.uint32)
    for s in range(m):
        counts += (samples[s][:, None] == samples[s][None, :]).astype(np.uint32)
    return samples, counts


def binder_num(c, C, m):
    """Σ_{i<j} C_ij + Σ_{i<j, c_i=c_j} (m − 2·C_ij) as a Python int"""
    c = np.asarray(c)
    Ci = np.asarray(C).astype(np.int64)
    iu = np.triu_indices(len(c), 1)
    same = (c[:, None] == c[None, :])[iu]
    return int(Ci[iu].sum()) + int((int(m) - 2 * Ci[iu][same]).sum())


def vi_f(c, C):
    """f(c) = Σ_i [log n_{c_i} − 2·log T_i], T_i = Σ_{j: c_j=c_i} C_ij, by the direct O(n²) evaluation"""
    c = np.asarray(c)
    same = c[:, None] == c[None, :]
    T = (np.asarray(C).astype(np.float64) * same).sum(axis=1)
    return float(np.sum(np.log(same.sum(axis=1)) - 2.0 * np.log(T)))


class _Counts:
    """The two scores on the counts: S_ik = Σ_{j∈k} C_ij by a bincount; VI also keeps T_j = Σ_{j' in j's slot} C_jj'"""

    def __init__(self, C, m, loss, init):
        n = len(init)
        self.C, self.m, self.loss = C, m, loss
        self.new_score = 0 if loss == BINDER else -2.0 * np.log(m)
        self.lab = np.asarray(init, np.int64).copy()
        self.sz = np.bincount(self.lab, minlength=n + 2)
        self.sz[0] = 0
        self.T = np.zeros(n, np.int64)
        for j in range(n):
            if self.lab[j]:
                self.T[j] = C[j, self.lab == self.lab[j]].sum()

    def take_out(self, i, a):
        mem = self.lab == a
        self.T[mem] -= self.C[i][mem]

    def scores(self, i, occ):
        lab, T, row, n = self.lab, self.T, self.C[i], len(self.lab)
        # every occupied slot at once (bincount of integers below 2^53 in float64 is exact; slot 0 collects the unallocated)
        S = np.bincount(lab, weights=row.astype(np.float64), minlength=n + 2).astype(np.int64)
        nk = self.sz[occ]
        if self.loss == BINDER:
            d = self.m * nk - 2 * S[occ]
        else:
            alloc = lab != 0
            terms = np.zeros(n)
            terms[alloc] = np.log((T[alloc] + row[alloc]) / T[alloc])
            Ls = np.bincount(lab, weights=terms, minlength=n + 2)
            d = (nk + 1) * np.log(nk + 1) - nk * np.log(nk) - 2.0 * Ls[occ] - 2.0 * np.log(S[occ] + self.m)
        return d.tolist(), S[occ].tolist()

    def put_in(self, i, w, S):
        mem = self.lab == w
        self.T[mem] += self.C[i][mem]
        self.T[i] = S + self.m


def psm_search_ref(C, m, loss, init, order, maxK=0, maxsweeps=100):
    """One run.  init: n labels, 0 = unallocated; order: a permutation of 1..n.  Returns a dict with the raw and the
    sortlabels'd labels, loss, loss_num, sweeps, converged, moves, K."""
    C = np.asarray(C).astype(np.int64)
    n, m = len(init), int(m)
    out = greedy_search_ref.greedy_search(_Counts(C, m, loss, init), order, maxK if maxK else n + 1, maxsweeps)
    if loss == BINDER:
        num = binder_num(out["raw"], C, m)
        pairs = n * (n - 1) // 2
        out.update(loss_num=num, loss=(num / (m * pairs)) if pairs else 0.0)
    else:
        out.update(loss_num=0, loss=vi_f(out["raw"], C) / n + 2.0 * np.log(m))
    return out


def vi_best_move_gain(c, C, m):
    """The largest decrease of f any single-point move achieves (existing clusters and a new one, no cap), in O(n²):
    with point i taken out, staying and every target differ from that state by the step's Δ (redclust_hip.h), so the
    gain of the best move of i is Δ_stay − min Δ."""
    c = sortlabels(c) - 1
    C = np.asarray(C).astype(np.float64)
    n, K = len(c), int(c.max()) + 1
    same = c[:, None] == c[None, :]
    T = (C * same).sum(axis=1)
    nk0 = np.bincount(c, minlength=K).astype(np.float64)
    gain = 0.0
    for i in range(n):
        a = c[i]
        row = C[i].copy()
        row[i] = 0.0                                                # i itself is out
        Tr = T - np.where(c == a, row, 0.0)
        Tr[i] = 1.0                                                 # (unused: row[i] = 0)
        nk = nk0.copy()
        nk[a] -= 1
        S = np.bincount(c, weights=row, minlength=K)
        Ls = np.bincount(c, weights=np.log1p(row / Tr), minlength=K)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = (nk + 1) * np.log(nk + 1) - np.where(nk > 0, nk * np.log(np.maximum(nk, 1)), 0.0) - 2.0 * Ls - 2.0 * np.log(S + m)
        dnew = -2.0 * np.log(m)
        stay = d[a] if nk[a] > 0 else dnew
        d = np.where(nk > 0, d, np.inf)
        gain = max(gain, stay - min(float(d.min()), dnew))
    return gain


def best_single_move_gain(c, C, m, loss, maxK=0):
    """The largest decrease of the criterion (Binder: num, an int; VI: f) any single-point move achieves, by brute force
    over every point and every target (existing clusters and a new one): <= 0 means c is a local optimum."""
    value = (lambda x: binder_num(x, C, m)) if loss == BINDER else (lambda x: vi_f(x, C))
    return greedy_search_ref.best_single_move_gain(c, value, lambda k, alone: maxK == 0 or k < maxK)
