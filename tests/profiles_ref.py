"""Reference for the cluster profiles (csrc/profile.inc.hip): the definitions of include/redclust_hip.h in Python integers.  Not
product code.

Dq is the integer matrix (caller's order); its diagonal never counts.  A labelling's K clusters are taken in ascending label
order, slots 0..K−1 of sizes n_k; A(i) is the slot of point i.
    within[i]  = Σ_{j in A(i), j != i} Dq[i][j]
    S_t(i)     = Σ_{j in t} Dq[i][j], t != A(i); the neighbour is the t of least S_t/n_t, compared as S_t·n_u against S_u·n_t in
                 Python integers, ties to the lower slot; nearest[i] = S_t(i), neighbour[i] = that cluster's label; 0, 0 if K = 1
    medoid of slot k: the member of least within, ties to the smallest index; reported 1-based with its within."""
from fractions import Fraction

import numpy as np

from score_ref import clusters


def _select(S_row, sizes, own):
    """(slot, S) of the neighbour among the slots other than own, or (None, 0)"""
    best = None
    for t in range(len(sizes)):
        if t == own:
            continue
        if best is None or int(S_row[t]) * int(sizes[best]) < int(S_row[best]) * int(sizes[t]):   # strictly less: lower slot on ties
            best = t
    return (None, 0) if best is None else (best, int(S_row[best]))


def _medoids(within, ids, K):
    med, medw = [], []
    for k in range(K):
        members = [i for i in range(len(ids)) if ids[i] == k]
        i = min(members, key=lambda i: (within[i], i))
        med.append(i + 1); medw.append(within[i])
    return med, medw


def profile(Dq, z):
    """dict(K, labels, sizes, medoids, medoid_within, within, nearest, neighbour): lists of Python integers.  The sums are
    Dq (diagonal zeroed) @ membership in int64 — a row's sum to a cluster fits int64, that is how the matrix is quantised."""
    names, ids, sizes = clusters(z)
    n, K = len(ids), len(sizes)
    Q = np.array(Dq, dtype=np.int64)
    np.fill_diagonal(Q, 0)
    M = (ids[:, None] == np.arange(K)[None, :]).astype(np.int64)
    S = Q @ M                                                            # [i][t]
    within = [int(S[i, ids[i]]) for i in range(n)]
    nearest, neighbour = [], []
    for i in range(n):
        t, s = _select(S[i], sizes, int(ids[i]))
        nearest.append(s); neighbour.append(0 if t is None else int(names[t]))
    med, medw = _medoids(within, ids, K)
    return dict(K=K, labels=[int(x) for x in names], sizes=[int(x) for x in sizes], medoids=med, medoid_within=medw,
                within=within, nearest=nearest, neighbour=neighbour)


def profile_bruteforce(Dq, z):
    """the same by the definition: a double loop over the entries, no matrix product, no shared helper for the sums"""
    n = len(z)
    names = sorted(set(int(x) for x in z))
    slot = {l: t for t, l in enumerate(names)}
    ids = [slot[int(x)] for x in z]
    sizes = [ids.count(t) for t in range(len(names))]
    K = len(names)
    within, nearest, neighbour = [], [], []
    for i in range(n):
        S = [0] * K
        for j in range(n):
            if j != i:
                S[ids[j]] += int(Dq[i][j])
        within.append(S[ids[i]])
        best = None
        for t in range(K):
            if t == ids[i]:
                continue
            if best is None:
                best = t
            else:
                c = Fraction(S[t], sizes[t]) - Fraction(S[best], sizes[best])     # exact means
                if c < 0:
                    best = t
        nearest.append(0 if best is None else S[best]); neighbour.append(0 if best is None else names[best])
    med, medw = [], []
    for k in range(K):
        bi = None
        for i in range(n):
            if ids[i] == k and (bi is None or within[i] < within[bi]):
                bi = i
        med.append(bi + 1); medw.append(within[bi])
    return dict(K=K, labels=names, sizes=sizes, medoids=med, medoid_within=medw, within=within, nearest=nearest, neighbour=neighbour)


def silhouette_exact(p, z):
    """[Fraction]: the silhouette of every point of labelling z from its profile dict, by the formula in exact rationals"""
    size_of = dict(zip(p["labels"], p["sizes"]))
    n = len(p["within"])
    out = []
    for i in range(n):
        na = size_of[int(z[i])]
        if na == 1 or p["neighbour"][i] == 0:
            out.append(Fraction(0)); continue
        a, b = Fraction(p["within"][i], na - 1), Fraction(p["nearest"][i], size_of[p["neighbour"][i]])
        hi = max(a, b)
        out.append(Fraction(0) if hi == 0 else (b - a) / hi)
    return out


def mean_silhouette(Dq, z):
    """the mean silhouette of a labelling as a Fraction"""
    s = silhouette_exact(profile(Dq, z), z)
    return sum(s, Fraction(0)) / len(s)


def mismatches(out, l, ref):
    """the fields in which labelling l of a Context.profiles dict differs from a reference profile, integer for integer"""
    fields = ["labels", "sizes", "medoids", "medoid_within"] + (["within", "nearest", "neighbour"] if out["within"] is not None else [])
    bad = [f for f in fields if [int(x) for x in out[f][l]] != ref[f]]
    return bad + (["K"] if int(out["K"][l]) != ref["K"] else [])
