"""NumPy restatement of the exact expected-VI search (DESIGN.md §8 "Exact expected VI search", include/redclust_hip.h
rc_vi_search): a plain loop that keeps the contingency tables N^s, test infrastructure only.  Everything is integer
arithmetic on a given table G (Gq of the design: G[x] = rint((φ(x+1) − φ(x))·2^32)), so the device has to reproduce a run
bit for bit when the reference is handed the library's table."""
import numpy as np

from psm_search_ref import sortlabels


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


def vi_search_ref(samples, G, init, order, maxK=0, maxsweeps=100):
    """One run.  samples: m×n labels; init: n labels, 0 = unallocated; order: a permutation of 1..n.  Returns a dict with
    the raw slots and the sortlabels'd labels, loss_num (Q of the final labelling, summed over the tables it kept), sweeps,
    converged, moves, K, and the final tables N (m × Lmax × Kcap)."""
    S, Lmax = relabel(samples)
    m, n = S.shape
    G = np.asarray(G, np.int64)
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
    sweeps = moves = 0
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
                if sz[a] == 0:
                    K -= 1
            emptied = a != 0 and sz[a] == 0
            occ = np.flatnonzero(sz[1:Kcap + 1]) + 1
            best = None                                            # (score, priority, slot, is_new)
            if len(occ):
                acc = G[N[rows, li][:, occ - 1]].sum(axis=0)       # Σ_s G[N^s[l_s(i)][k]] (int64: m·G < 2^62)
                d = m * G[sz[occ]] - 2 * acc
                prio = np.where(occ == a, 0, occ)
                q = int(np.lexsort((prio, d))[0])
                best = (int(d[q]), int(prio[q]), int(occ[q]), False)
            if K < Kcap:
                slot = a if emptied else int(np.flatnonzero(sz[1:Kcap + 1] == 0)[0]) + 1
                cand = (0, 0 if emptied else slot, slot, True)
                if best is None or cand[:2] < best[:2]:
                    best = cand
            _, _, w, isnew = best
            lab[i] = w
            sz[w] += 1
            N[rows, li, w - 1] += 1
            K += int(isnew)
            moved += int(a == 0 or w != a)
        sweeps += 1
        moves += moved
        if moved == 0:
            converged = True
            break
    Phi = phi_table(G)
    q = m * sum(Phi[int(x)] for x in sz) - 2 * sum(Phi[x] * int(cnt) for x, cnt in enumerate(np.bincount(N.ravel())))
    return dict(raw=lab.copy(), labels=sortlabels(lab), loss_num=q, sweeps=sweeps, converged=converged, moves=moves, K=K, N=N)


def best_single_move_gain(c, samples, G, maxK=0):
    """The largest decrease of Q any single-point move achieves, by brute force over every point and every target
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
