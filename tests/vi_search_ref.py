"""NumPy restatement of the exact expected-VI search (DESIGN.md §8 "Exact expected VI search", include/redclust_hip.h
rc_vi_search): a plain loop that keeps the contingency tables N^s, test infrastructure only.  Everything is integer
arithmetic on a given table G (Gq of the design: G[x] = rint((φ(x+1) − φ(x))·2^32)), so the device has to reproduce a run
bit for bit when the reference is handed the library's table."""
import numpy as np

import greedy_search_ref
from greedy_search_ref import sortlabels


def numpy_G(n):
    """The table as NumPy computes it: G[0] = 0, G[x] = rint((log(x+1) + x·log1p(1/x))·2^32) for x = 1..n−1."""
    x = np.arange(1, n, dtype=np.float64)
    out = np.zeros(n, np.int64)
    out[1:] = np.rint((np.log(x + 1.0) + x * np.log1p(1.0 / x)) * 2.0 ** 32).astype(np.int64)
    return out


def phi_table(G):
    """Φ(x) = Σ_{y<x} G[y] for x = 0..len(G), as Python ints (exact)"""
    out = [0]
    for g in G:
        out.append(out[-1] + int(g))
    return out


def relabel(samples):
    """every sample to 0..L_s−1 by order of first appearance; returns (m×n int64, Lmax)"""
    S = np.stack([sortlabels(s) - 1 for s in np.asarray(samples)])
    return S, int(S.max()) + 1


def compact(init):
    """starting labels to slots 1..K0 by order of first appearance, 0 stays 0"""
    out, seen = np.zeros(len(init), np.int64), {}
    for j, v in enumerate(init):
        if v:
            out[j] = seen.setdefault(int(v), len(seen) + 1)
    return out


def q_direct(c, samples, G):
    """Q(c) = m·Σ_k Φ(n_k) − 2·Σ_s Σ_kl Φ(N^s_kl) from scratch, a Python int; c must have no unallocated point"""
    c = sortlabels(c) - 1
    S, Lmax = relabel(samples)
    m = len(S)
    Phi = phi_table(G)
    q = m * sum(Phi[int(x)] for x in np.bincount(c))
    for s in S:
        q -= 2 * sum(Phi[int(x)] for x in np.bincount(c * Lmax + s))
    return q


def constant(samples, G):
    """Σ_s Σ_l Φ(n^s_l): what turns Q into n·m·2^32·E[VI]"""
    Phi = phi_table(G)
    return sum(Phi[int(x)] for s in np.asarray(samples) for x in np.bincount(s))


class Tables:
    """The exact VI score on the contingency tables N (m × Lmax × Kcap): Δ_k = m·G[n_k] − 2·Σ_s G[N^s[l_s(i)][k]]"""
    new_score = 0

    def __init__(self, samples, G, init, maxK):
        self.S, self.Lmax = relabel(samples)
        self.m, n = self.S.shape
        self.G = np.asarray(G, np.int64)
        self.Kcap = min(maxK if maxK > 0 else self.Lmax, n)
        self.lab = compact(np.asarray(init, np.int64))
        assert int(self.lab.max()) <= self.Kcap
        self.sz = np.bincount(self.lab, minlength=self.Kcap + 2)
        self.sz[0] = 0
        self.N = np.zeros((self.m, self.Lmax, self.Kcap), np.int64)
        self.rows = np.arange(self.m)
        for j in np.flatnonzero(self.lab):
            self.N[self.rows, self.S[:, j], self.lab[j] - 1] += 1

    def take_out(self, i, a):
        self.N[self.rows, self.S[:, i], a - 1] -= 1

    def table_sums(self, i, occ):
        """Σ_s G[N^s[l_s(i)][k]] of the slots k of occ (int64: m·G < 2^62)"""
        return self.G[self.N[self.rows, self.S[:, i]][:, occ - 1]].sum(axis=0)

    def scores(self, i, occ):
        return (self.m * self.G[self.sz[occ]] - 2 * self.table_sums(i, occ)).tolist(), None

    def put_in(self, i, w, _):
        self.N[self.rows, self.S[:, i], w - 1] += 1

    def phi_of_tables(self, Phi):
        """Σ_s Σ_kl Φ(N^s_kl), a Python int"""
        return sum(Phi[x] * int(cnt) for x, cnt in enumerate(np.bincount(self.N.ravel())))


def vi_search_ref(samples, G, init, order, maxK=0, maxsweeps=100):
    """One run.  samples: m×n labels; init: n labels, 0 = unallocated; order: a permutation of 1..n.  Returns a dict with
    the raw slots and the sortlabels'd labels, loss_num (Q of the final labelling, summed over the tables it kept), sweeps,
    converged, moves, K, and the final tables N (m × Lmax × Kcap)."""
    t = Tables(samples, G, init, maxK)
    out = greedy_search_ref.greedy_search(t, order, t.Kcap, maxsweeps)
    Phi = phi_table(G)
    out.update(loss_num=t.m * sum(Phi[int(x)] for x in t.sz) - 2 * t.phi_of_tables(Phi), N=t.N)
    return out


def best_single_move_gain(c, samples, G, maxK=0, q=None):
    """The largest decrease of Q (q = q_direct of this module unless given) any single-point move achieves, by brute force
    over every point and every target (existing clusters and, below the cap, a new one): <= 0 means c is a local optimum of
    the integer criterion."""
    Kcap = min(maxK if maxK > 0 else relabel(samples)[1], len(c))
    return greedy_search_ref.best_single_move_gain(c, lambda x: (q or q_direct)(x, samples, G), lambda k, alone: not alone and k < Kcap)
