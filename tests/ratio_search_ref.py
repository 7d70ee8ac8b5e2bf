"""NumPy / Python-int restatement of the ratio-loss search (DESIGN.md §8 "Ratio-loss search", include/redclust_hip.h
rc_ratio_search): vi_search_ref's loop and tables with the three ratio criteria, test infrastructure only.  The state is Python
ints and int64 arrays (exact: every value is below 2^53), the one division per sample is np.float64's, so the device has to reproduce a run bit for bit when the reference is handed
the library's table.

  entropic: T_s = Σ_kl Φ(N^s_kl), A = Σ_k Φ(n_k), B_s = Σ_l Φ(n^s_l), C = Φ(n);   omARI: the same with C2(x) = x(x−1)/2 for Φ
  NVI (A + B − 2T)/(C − T);  NID (max(A, B) − T)/(C − min(A, B));  omARI C(A + B − 2T)/(C(A + B) − 2AB);  term = rint(ratio·2^40)"""
import numpy as np

import greedy_search_ref
import vi_search_ref
from greedy_search_ref import sortlabels
from vi_search_ref import phi_table, relabel

LOSSES = ("omARI", "NVI", "NID")


def weights(G, loss):
    """(δ, W): what one more member adds to a cell of size x, and its running sum W(x) = Σ_{y<x} δ(y) — Python ints"""
    d = list(range(len(G))) if loss == "omARI" else [int(g) for g in G]
    return d, phi_table(d)


def num_den(T, A, B, C, loss):
    """(num, den) of the states (T, A) against (B, C) as int64 arrays: T and B int64 arrays or ints, A and C ints.  Every value is
    below 2^53 (asserted), so int64 is exact and so is the conversion to float64"""
    T, B = np.asarray(T, np.int64), np.asarray(B, np.int64)
    if loss == "omARI":
        num, den = C * (A + B - 2 * T), C * (A + B) - 2 * A * B + 0 * T
    elif loss == "NVI":
        num, den = A + B - 2 * T, C - T + 0 * B
    else:
        num, den = np.maximum(A, B) - T, C - np.minimum(A, B) + 0 * T
    assert num.min() >= 0 and den.min() >= 0 and max(num.max(), den.max()) < 2 ** 53
    return num, den


def term(T, A, B, C, loss):
    """0 where den = 0, else rint(float64(num) / float64(den) · 2^40), int64"""
    num, den = num_den(T, A, B, C, loss)
    ratio = np.float64(num) / np.where(den == 0, 1, den).astype(np.float64)
    return np.where(den == 0, 0, np.rint(ratio * np.float64(2.0 ** 40)).astype(np.int64))


def sample_states(c, samples, G, loss):
    """(T_s array, A, B_s array, C) of a complete labelling c; labels are used as they come (empty bins weigh W(0) = 0)"""
    c, S = np.asarray(c, np.int64), np.asarray(samples, np.int64)
    Lmax = int(S.max()) + 1
    W = np.concatenate([[0], np.cumsum(np.arange(len(G)) if loss == "omARI" else np.asarray(G, np.int64))]).astype(np.int64)
    T = np.array([W[np.bincount(c * Lmax + s)].sum() for s in S], np.int64)
    B = np.array([W[np.bincount(s)].sum() for s in S], np.int64)
    return T, int(W[np.bincount(c)].sum()), B, int(W[len(c)])


def q_direct(c, samples, G, loss):
    """Q(c) = Σ_s term_s from scratch, a Python int; c must have no unallocated point"""
    return int(term(*sample_states(c, samples, G, loss), loss).sum())


class RatioTables(vi_search_ref.Tables):
    """score_k = Σ_s term_s(T_s + δ(N^s[l_s(i)][k]), A + δ(n_k)) − Σ_s term_s(T_s, A), T_s and A kept with the visited point out;
    B_s and C are the full samples' throughout"""

    def __init__(self, samples, G, init, maxK, loss):
        super().__init__(samples, G, init, maxK)
        self.loss = loss
        self.d, self.W = weights(G, loss)
        self.dv = np.asarray(self.d, np.int64)
        self.C = self.W[self.S.shape[1]]
        Wv = np.asarray(self.W, np.int64)
        self.B = np.array([Wv[np.bincount(s)].sum() for s in self.S], np.int64)
        self.A = sum(self.W[int(x)] for x in self.sz)
        self.T = Wv[self.N].sum(axis=(1, 2))

    def _cells(self, i, k):
        return self.N[self.rows, self.S[:, i], k - 1]

    def take_out(self, i, a):
        super().take_out(i, a)
        self.A -= self.d[int(self.sz[a])]
        self.T -= self.dv[self._cells(i, a)]

    def scores(self, i, occ):
        base = int(term(self.T, self.A, self.B, self.C, self.loss).sum())
        return [int(term(self.T + self.dv[self._cells(i, k)], self.A + self.d[int(self.sz[k])], self.B, self.C, self.loss).sum()) - base
                for k in occ], None

    def put_in(self, i, w, _):
        self.A += self.d[int(self.sz[w])]
        self.T += self.dv[self._cells(i, w)]
        super().put_in(i, w, _)


def ratio_search_ref(samples, G, loss, init, order, maxK=0, maxsweeps=100):
    """One run; arguments and the returned dict as vi_search_ref.  loss_num is Q of the state the run kept."""
    t = RatioTables(samples, G, init, maxK, loss)
    out = greedy_search_ref.greedy_search(t, order, t.Kcap, maxsweeps)
    out.update(loss_num=int(term(t.T, t.A, t.B, t.C, loss).sum()), N=t.N)
    return out
