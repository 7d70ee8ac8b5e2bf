"""NumPy restatement of the PEAR search (DESIGN.md §8 "PEAR search", include/redclust_hip.h rc_pear_search): the run loop
of greedy_search_ref.py with the posterior expected adjusted Rand index as the criterion, in Python integers and
fractions.Fraction, so every comparison is exact.  Test infrastructure only; the device has to reproduce a run bit for bit.

  T = n(n−1)/2,  P = Σ_{i<j} C_ij,  X(c) = Σ_{i<j, c_i=c_j≠0} C_ij,  A(c) = Σ_k n_k(n_k−1)/2
  PEAR(c) = num/den,  num = 2·(T·X − A·P),  den = T·(m·A + P) − 2·A·P;  0/1 where den = 0
The run maximises the fraction; greedy_search minimises (score, priority), so a score is −Fraction(num, den)."""
from fractions import Fraction

import numpy as np

import greedy_search_ref
from greedy_search_ref import sortlabels  # noqa: F401  (the tests take it from here)
from psm_search_ref import planted_counts  # noqa: F401


def pear_parts(c, C):
    """(X, A, P) of a labelling (0 = unallocated: a singleton) as Python ints, cluster by cluster"""
    c = np.asarray(c, np.int64)
    Ci = np.asarray(C).astype(np.int64)
    X = A = 0
    for k in np.unique(c[c > 0]):
        idx = np.flatnonzero(c == k)
        X += (int(Ci[np.ix_(idx, idx)].sum()) - int(Ci[idx, idx].sum())) // 2
        A += len(idx) * (len(idx) - 1) // 2
    return X, A, (int(Ci.sum()) - int(np.trace(Ci))) // 2


def fraction_of(X, A, P, m, T):
    """(num, den) of a state in Python ints, (0, 1) where den = 0"""
    den = T * (m * A + P) - 2 * A * P
    return (2 * (T * X - A * P), den) if den else (0, 1)


def pear_num_den(c, C, m):
    n = len(c)
    X, A, P = pear_parts(c, C)
    return fraction_of(X, A, P, int(m), n * (n - 1) // 2)


def pear_float(c, C, m):
    """mcclust's pear(cl, psm) with psm = C/m, in floating point (nan where its denominator is 0)"""
    c = np.asarray(c)
    n = len(c)
    iu = np.triu_indices(n, 1)
    psm = (np.asarray(C).astype(np.float64) / float(m))[iu]
    ind = (c[:, None] == c[None, :])[iu].astype(np.float64)
    no2 = n * (n - 1) / 2.0
    sum_psm, sum_i, sum_i_psm = psm.sum(), ind.sum(), (ind * psm).sum()
    correc = sum_i * sum_psm / no2 if no2 else 0.0
    den = 0.5 * (sum_psm + sum_i) - correc
    return (sum_i_psm - correc) / den if den else float("nan")


class _Pear:
    """The criterion for greedy_search: X and A of the current labelling, kept up to date as points leave and enter"""

    def __init__(self, C, m, init):
        n = len(init)
        self.C, self.m, self.T = C, m, n * (n - 1) // 2
        self.lab = np.asarray(init, np.int64).copy()
        self.sz = np.bincount(self.lab, minlength=n + 2)
        self.sz[0] = 0
        self.X, self.A, self.P = pear_parts(self.lab, C)
        self.min_den = None                                     # the smallest raw den among the states scored

    def _score(self, X, A):
        den = self.T * (self.m * A + self.P) - 2 * A * self.P
        self.min_den = den if self.min_den is None else min(self.min_den, den)
        return -Fraction(*fraction_of(X, A, self.P, self.m, self.T))

    @property
    def new_score(self):
        return self._score(self.X, self.A)

    def take_out(self, i, a):
        self.X -= int(self.C[i][self.lab == a].sum())           # lab[i] is 0 already
        self.A -= int(self.sz[a])                               # n_a − 1 pairs, with sz[a] already lowered

    def scores(self, i, occ):
        n = len(self.lab)
        S = np.bincount(self.lab, weights=self.C[i].astype(np.float64), minlength=n + 2).astype(np.int64)[occ].tolist()
        return [self._score(self.X + s, self.A + int(nk)) for s, nk in zip(S, self.sz[occ])], S

    def put_in(self, i, w, S):
        self.X += int(S)
        self.A += int(self.sz[w])


def pear_search_ref(C, m, init, order, maxK=0, maxsweeps=100):
    """One run.  init: n labels, 0 = unallocated; order: a permutation of 1..n.  Returns greedy_search's dict (raw, labels,
    sweeps, converged, moves, K) and num, den — recomputed from the matrix — pear, start (the start's fraction) and min_den."""
    C = np.asarray(C).astype(np.int64)
    n, m = len(init), int(m)
    crit = _Pear(C, m, init)
    start = Fraction(*fraction_of(crit.X, crit.A, crit.P, m, crit.T))
    out = greedy_search_ref.greedy_search(crit, order, maxK if maxK else n + 1, maxsweeps)
    num, den = pear_num_den(out["raw"], C, m)
    assert (num, den) == fraction_of(crit.X, crit.A, crit.P, m, crit.T)      # the running state is the labelling's
    out.update(num=num, den=den, pear=num / den, start=start, min_den=crit.min_den)
    return out


def best_run(runs):
    """the first run of maximal fraction"""
    fr = [Fraction(r["num"], r["den"]) for r in runs]
    return fr.index(max(fr))
