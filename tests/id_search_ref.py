"""NumPy / Python-int restatement of the exact expected-ID search (DESIGN.md §8 "Exact expected ID search",
include/redclust_hip.h rc_id_search): vi_search_ref's loop with the information distance's score, test infrastructure only.
Everything is integer arithmetic on a given table G, and F — the one piece that is not a table sum — is evaluated with
Python ints, so the device has to reproduce a run bit for bit when the reference is handed the library's table.

  Q_ID(c) = F(A(c)) − Σ_s Σ_kl Φ(N^s_kl),   A(c) = Σ_k Φ(n_k),   F(x) = Σ_s max(x, B_s),   B_s = Σ_l Φ(n^s_l)."""
import bisect

import numpy as np

from psm_search_ref import sortlabels
from vi_search_ref import compact, phi_table, relabel


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


def id_search_ref(samples, G, init, order, maxK=0, maxsweeps=100):
    """One run; arguments and the returned dict as vi_search_ref, and besides: below / above, the numbers of scored
    candidates A₀ + G[n_k] that lay strictly below some B_s / strictly above some B_s — whether both sides of the max were
    visited — and equal, the number that met a B_s exactly."""
    S, Lmax = relabel(samples)
    m, n = S.shape
    G = np.asarray(G, np.int64)
    Gi = [int(g) for g in G]
    Phi = phi_table(G)
    B = sample_sums(S, Phi)
    Bmin, Bmax = min(B), max(B)
    Bs, Pre = sorted_table(B)
    Bset = set(B)
    Kcap = min(maxK if maxK > 0 else Lmax, n)
    lab = compact(np.asarray(init, np.int64))
    K = int(lab.max())
    assert K <= Kcap
    sz = np.zeros(Kcap + 2, np.int64)
    N = np.zeros((m, Lmax, Kcap), np.int64)
    rows = np.arange(m)
    for j in range(n):
        if lab[j]:
            sz[lab[j]] += 1
            N[rows, S[:, j], lab[j] - 1] += 1
    A = sum(Phi[int(x)] for x in sz)
    sweeps = moves = below = above = equal = 0
    converged = False
    while sweeps < maxsweeps:
        moved = 0
        for i in (int(o) - 1 for o in order):
            a = int(lab[i])
            li = S[:, i]
            if a:
                lab[i] = 0
                sz[a] -= 1
                N[rows, li, a - 1] -= 1
                A -= Gi[int(sz[a])]
                if sz[a] == 0:
                    K -= 1
            emptied = a != 0 and sz[a] == 0
            occ = np.flatnonzero(sz[1:Kcap + 1]) + 1
            best = None                                            # (score, priority, slot, is_new)
            if len(occ):
                acc = G[N[rows, li][:, occ - 1]].sum(axis=0)       # Σ_s G[N^s[l_s(i)][k]] (int64: m·G < 2^62)
                FA = F_sorted(A, Bs, Pre)
                for k, ak in zip(occ, acc):
                    x = A + Gi[int(sz[k])]
                    below += int(x < Bmax)
                    above += int(x > Bmin)
                    equal += int(x in Bset)
                    cand = (F_sorted(x, Bs, Pre) - FA - int(ak), 0 if k == a else int(k), int(k), False)
                    if best is None or cand[:2] < best[:2]:
                        best = cand
            if K < Kcap:
                slot = a if emptied else int(np.flatnonzero(sz[1:Kcap + 1] == 0)[0]) + 1
                cand = (0, 0 if emptied else slot, slot, True)
                if best is None or cand[:2] < best[:2]:
                    best = cand
            _, _, w, isnew = best
            lab[i] = w
            A += Gi[int(sz[w])]
            sz[w] += 1
            N[rows, li, w - 1] += 1
            K += int(isnew)
            moved += int(a == 0 or w != a)
        sweeps += 1
        moves += moved
        if moved == 0:
            converged = True
            break
    assert A == sum(Phi[int(x)] for x in sz)
    q = F(A, B) - sum(Phi[x] * int(cnt) for x, cnt in enumerate(np.bincount(N.ravel())))
    return dict(raw=lab.copy(), labels=sortlabels(lab), loss_num=q, sweeps=sweeps, converged=converged, moves=moves, K=K, N=N,
                below=below, above=above, equal=equal)


def best_single_move_gain(c, samples, G, maxK=0):
    """The largest decrease of Q_ID any single-point move achieves, by brute force over every point and every target
    (existing clusters and, below the cap, a new one): <= 0 means c is a local optimum of the integer criterion."""
    c = np.asarray(c, np.int64)
    n = len(c)
    _, Lmax = relabel(samples)
    Kcap = min(maxK if maxK > 0 else Lmax, n)
    base, gain = q_direct(c, samples, G), 0
    labels = list(np.unique(c))
    fresh = int(c.max()) + 1
    for i in range(n):
        alone = int((c == c[i]).sum()) == 1
        targets = [l for l in labels if l != c[i]]
        if len(labels) - int(alone) < Kcap and not alone:
            targets.append(fresh)
        for l in targets:
            x = c.copy()
            x[i] = l
            gain = max(gain, base - q_direct(x, samples, G))
    return gain
