"""NumPy / Python-int restatement of the hierarchical point estimates (DESIGN.md §8 "Hierarchical point estimates",
include/redclust_hip.h rc_hclust and rc_psm_expected_loss): test infrastructure only.  Every decision is exact integer
arithmetic — float ratios only shortlist candidates — so the device has to reproduce merges, Binder curve and cuts bit for
bit.  hclust_ref keeps per-row caches (n = 1025 in seconds); hclust_naive scans every pair at every step and is what
hclust_ref itself is checked against at small n (test_hclust_cpu.py)."""
import numpy as np

import psm_search_ref as R

AVERAGE, COMPLETE, SINGLE = 0, 1, 2
LINKAGES = {"average": AVERAGE, "complete": COMPLETE, "single": SINGLE}
MERGE = np.dtype([("a", np.int32), ("b", np.int32), ("size", np.int32), ("m_ab", np.uint32), ("s_ab", np.int64)], align=True)
SHORTLIST = 1.0 - 1e-12         # float ratios of integers below 2^53 are within a few ulp: nothing exact-maximal is dropped


def _first_max(vals, dens):
    """Position of the exactly largest vals[k]/dens[k]; among equals the first.  vals, dens: int64 arrays, dens > 0."""
    r = vals / dens
    best = None
    for k in np.flatnonzero(r >= r.max() * SHORTLIST):
        x, d = int(vals[k]), int(dens[k])
        if best is None or x * bd > bx * d:                  # strictly larger, by cross-multiplication in Python ints
            best, bx, bd = int(k), x, d
    return best


def _record(merges, bnum, t, a, b, sz, S, M, m, linkage):
    sab = int(S[a, b])
    merges[t] = (a + 1, b + 1, int(sz[a] + sz[b]), 0 if linkage == AVERAGE else int(M[a, b]), sab)
    bnum.append(bnum[-1] + int(sz[a]) * int(sz[b]) * int(m) - 2 * sab)


def _merge(a, b, S, M, sz, active, linkage):
    active[b] = False
    others = np.flatnonzero(active)
    others = others[others != a]
    S[a, others] += S[b, others]
    S[others, a] = S[a, others]
    if linkage != AVERAGE:
        M[a, others] = (np.minimum if linkage == COMPLETE else np.maximum)(M[a, others], M[b, others])
        M[others, a] = M[a, others]
    sz[a] += sz[b]
    return others


def hclust_naive(C, m, linkage):
    """The definition, literally: at every step all active pairs a < b in lexicographic order, the first of the largest
    similarity.  O(n³)."""
    S = np.asarray(C).astype(np.int64).copy()
    M = S.copy()
    n = len(S)
    sz, active = np.ones(n, np.int64), np.ones(n, bool)
    merges, bnum = np.zeros(max(n - 1, 0), MERGE), [int(np.triu(S, 1).sum())]
    for t in range(n - 1):
        best = None
        act = np.flatnonzero(active)
        for i, a in enumerate(act):
            for b in act[i + 1:]:
                x, d = (int(S[a, b]), int(sz[a] * sz[b])) if linkage == AVERAGE else (int(M[a, b]), 1)
                if best is None or x * bd > bx * d:
                    best, bx, bd = (int(a), int(b)), x, d
        a, b = best
        _record(merges, bnum, t, a, b, sz, S, M, m, linkage)
        _merge(a, b, S, M, sz, active, linkage)
    return dict(merges=merges, binder_num=np.array(bnum, np.int64))


def hclust_ref(C, m, linkage):
    """The same run with a per-row cache of the best partner among the larger names."""
    S = np.asarray(C).astype(np.int64).copy()
    M = S.copy()
    V = S if linkage == AVERAGE else M                                  # what similarities are read from
    n = len(S)
    sz, active = np.ones(n, np.int64), np.ones(n, bool)
    val, part = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    ones = np.ones(n, np.int64)

    def dens(r, cols):
        return sz[r] * sz[cols] if linkage == AVERAGE else ones[: len(np.atleast_1d(cols))]

    def rescan(r):
        cols = np.flatnonzero(active[r + 1:]) + r + 1
        if len(cols) == 0:
            part[r] = -1
            return
        k = _first_max(V[r, cols], dens(r, cols))
        val[r], part[r] = V[r, cols[k]], cols[k]

    for r in range(n):
        rescan(r)
    merges, bnum = np.zeros(max(n - 1, 0), MERGE), [int(np.triu(S, 1).sum())]
    for t in range(n - 1):
        rows = np.flatnonzero(active & (part >= 0))
        a = int(rows[_first_max(val[rows], sz[rows] * sz[part[rows]] if linkage == AVERAGE else ones[: len(rows)])])
        b = int(part[a])
        _record(merges, bnum, t, a, b, sz, S, M, m, linkage)
        others = _merge(a, b, S, M, sz, active, linkage)
        lower = others[others < b]
        stale = lower[(part[lower] == a) | (part[lower] == b)]          # the cached entry changed (a) or is gone (b)
        for r in [a] + [int(x) for x in stale]:
            rescan(r)
        keep = lower[(lower < a) & (part[lower] != a) & (part[lower] != b)]
        if len(keep):                                                   # their entry at column a is new: better than the cached one?
            nv, nd = V[keep, a], dens(a, keep)
            cv, cd = val[keep], (sz[keep] * sz[part[keep]] if linkage == AVERAGE else ones[: len(keep)])
            for k in np.flatnonzero(nv / nd >= (cv / cd) * SHORTLIST):
                l, r_ = int(nv[k]) * int(cd[k]), int(cv[k]) * int(nd[k])
                if l > r_ or (l == r_ and a < part[keep[k]]):
                    val[keep[k]], part[keep[k]] = nv[k], a
    return dict(merges=merges, binder_num=np.array(bnum, np.int64))


def cut(merges, n, K):
    """The partition after the first n − K merges, sortlabels'd."""
    names = np.arange(1, n + 1)
    for g in merges[: n - K]:
        names[names == g["b"]] = g["a"]
    return R.sortlabels(names)


def heights(merges, m, linkage):
    """1 − similarity/m per merge, in f64 — what SciPy calls the merge distance"""
    n = len(merges) + 1
    size, out = np.ones(n + 1, np.int64), []
    for g in merges:
        a, b = int(g["a"]), int(g["b"])
        sim = int(g["s_ab"]) / (int(size[a]) * int(size[b])) if linkage == AVERAGE else int(g["m_ab"])
        out.append(1.0 - sim / m)
        size[a] = g["size"]
    return np.array(out)


def eloss_T(c, C):
    """T_i = Σ_{j: c_j = c_i} C_ij as int64"""
    c = np.asarray(c)
    return (np.asarray(C).astype(np.int64) * (c[:, None] == c[None, :])).sum(axis=1)


def binder_num_from_T(c, C, m):
    """Σ_{i<j} C_ij + m·#{i<j: c_i = c_j} − Σ_i (T_i − m): the header's formula, as a Python int"""
    c = np.asarray(c)
    nk = np.bincount(c)
    return int(np.triu(np.asarray(C).astype(np.int64), 1).sum()) + int(m) * int((nk * (nk - 1) // 2).sum()) - int((eloss_T(c, C) - int(m)).sum())
