"""NumPy / Python-int restatement of the exact expected-ID search (DESIGN.md §8 "Exact expected ID search",
include/redclust_hip.h rc_id_search): vi_search_ref's loop with the information distance's score, test infrastructure only.
Everything is integer arithmetic on a given table G, and F — the one piece that is not a table sum — is evaluated with
Python ints, so the device has to reproduce a run bit for bit when the reference is handed the library's table.

  Q_ID(c) = F(A(c)) − Σ_s Σ_kl Φ(N^s_kl),   A(c) = Σ_k Φ(n_k),   F(x) = Σ_s max(x, B_s),   B_s = Σ_l Φ(n^s_l)."""
import bisect

import numpy as np

import greedy_search_ref
import vi_search_ref
from greedy_search_ref import sortlabels
from vi_search_ref import compact, phi_table, relabel  # noqa: F401  (the tests take them from here)


def sample_sums(samples, Phi):
    """B_s = Σ_l Φ(n^s_l) of every sample, Python ints"""
    return [sum(Phi[int(x)] for x in np.bincount(s)) for s in np.asarray(samples)]


def F(x, B):
    """Σ_s max(x, B_s), a Python int"""
    return sum(max(int(x), b) for b in B)


def sorted_table(B):
    """(Bs, Pre): the B_s ascending and Pre[p] = Σ_{t<p} Bs[t], Python ints"""
    Bs, Pre = sorted(B), [0]
    for b in Bs:
        Pre.append(Pre[-1] + b)
    return Bs, Pre


def F_sorted(x, Bs, Pre):
    """F(x) = x·p + Pre[m] − Pre[p], p = #{t : Bs[t] <= x} — equal to F(x, B) (tests/test_idsearch_cpu.py checks it); what the
    search loop below uses, since it evaluates F for every candidate of every step.  Python ints throughout."""
    p = bisect.bisect_right(Bs, int(x))
    return int(x) * p + Pre[-1] - Pre[p]


def q_direct(c, samples, G):
    """Q_ID(c) from scratch, a Python int; c must have no unallocated point"""
    c = sortlabels(c) - 1
    S, Lmax = relabel(samples)
    Phi = phi_table(G)
    q = F(sum(Phi[int(x)] for x in np.bincount(c)), sample_sums(S, Phi))
    for s in S:
        q -= sum(Phi[int(x)] for x in np.bincount(c * Lmax + s))
    return q


class _IdTables(vi_search_ref.Tables):
    """The exact ID score on the same tables: Δ_k = F(A₀ + G[n_k]) − F(A₀) − Σ_s G[N^s[l_s(i)][k]], with A = Σ_k Φ(n_k) kept up to
    date as a Python int.  below / above / equal: how the scored candidates lay against the B_s."""

    def __init__(self, samples, G, init, maxK):
        super().__init__(samples, G, init, maxK)
        self.Gi = [int(g) for g in self.G]
        self.Phi = phi_table(G)
        self.B = sample_sums(self.S, self.Phi)
        self.Bs, self.Pre = sorted_table(self.B)
        self.Bset = set(self.B)
        self.A = sum(self.Phi[int(x)] for x in self.sz)
        self.below = self.above = self.equal = 0

    def take_out(self, i, a):
        super().take_out(i, a)
        self.A -= self.Gi[int(self.sz[a])]

    def scores(self, i, occ):
        FA = F_sorted(self.A, self.Bs, self.Pre)
        xs = [self.A + self.Gi[int(self.sz[k])] for k in occ]
        self.below += sum(x < self.Bs[-1] for x in xs)
        self.above += sum(x > self.Bs[0] for x in xs)
        self.equal += sum(x in self.Bset for x in xs)
        return [F_sorted(x, self.Bs, self.Pre) - FA - int(ak) for x, ak in zip(xs, self.table_sums(i, occ))], None

    def put_in(self, i, w, _):
        super().put_in(i, w, _)
        self.A += self.Gi[int(self.sz[w])]


def id_search_ref(samples, G, init, order, maxK=0, maxsweeps=100):
    """One run; arguments and the returned dict as vi_search_ref, and besides: below / above, the numbers of scored
    candidates A₀ + G[n_k] that lay strictly below some B_s / strictly above some B_s — whether both sides of the max were
    visited — and equal, the number that met a B_s exactly."""
    t = _IdTables(samples, G, init, maxK)
    out = greedy_search_ref.greedy_search(t, order, t.Kcap, maxsweeps)
    assert t.A == sum(t.Phi[int(x)] for x in t.sz)
    out.update(loss_num=F(t.A, t.B) - t.phi_of_tables(t.Phi), N=t.N, below=t.below, above=t.above, equal=t.equal)
    return out


def best_single_move_gain(c, samples, G, maxK=0):
    """The largest decrease of Q_ID any single-point move achieves, by brute force over every point and every target
    (existing clusters and, below the cap, a new one): <= 0 means c is a local optimum of the integer criterion."""
    return vi_search_ref.best_single_move_gain(c, samples, G, maxK, q=q_direct)
