"""NumPy restatement of the several-partition summary (DESIGN.md §8 "Several-partition summary", redclust.jl_amd/wasabi.py):
the driver loop in Python integers on top of vi_search_ref (the group search is vi_search_ref on the sub-array) and
partdist_ref (the distances), test infrastructure only.  Everything is integer arithmetic on a given table G, so the library has
to reproduce every number bit for bit when the reference is handed the library's table."""
import numpy as np

import partdist_ref as PD
import vi_search_ref as V
from greedy_search_ref import sortlabels


def vi_distances(labellings, samples, G):
    """P×m lists of Python ints: VI_q = A_q + B_q − 2T"""
    P, T, A, B = PD.distances_ref(labellings, samples, G)
    return [[int(x) for x in row] for row in PD.numerators(P, T, A, B, "VI")]


def assign(dist):
    """(assignment, each sample's distance, W): the nearest particle, ties to the lowest index"""
    m = len(dist[0])
    a = [min(range(len(dist)), key=lambda l: (dist[l][s], l)) for s in range(m)]
    d = [dist[a[s]][s] for s in range(m)]
    return a, d, sum(d)


def farthest(d, used):
    cand = [s for s in range(len(d)) if s not in used and d[s] > 0]
    return min(cand, key=lambda s: (-d[s], s)) if cand else -1


def seed_particles(S, L, u, G):
    m = len(S)
    chosen = [(int(u[0]) * m) >> 53]
    dmin = vi_distances(S[chosen[0]], S, G)[0]
    for j in range(1, L):
        W = sum(dmin)
        if W == 0:
            break
        thr, run = (int(u[j]) * W) >> 53, 0
        for idx in range(m):
            run += dmin[idx]
            if run > thr:
                break
        chosen.append(idx)
        dmin = [min(a, b) for a, b in zip(dmin, vi_distances(S[idx], S, G)[0])]
    return [sortlabels(S[i]) for i in chosen]


def search_group(S, members, G, particle, orders, cap, maxsweeps):
    """the group's new particle: the first run of least loss_num among the one from the particle and those from empty labels"""
    n = S.shape[1]
    sub = S[members]
    runs = [V.vi_search_ref(sub, G, particle, np.arange(1, n + 1), maxK=cap, maxsweeps=maxsweeps)]
    runs += [V.vi_search_ref(sub, G, np.zeros(n, np.int64), o, maxK=cap, maxsweeps=maxsweeps) for o in orders]
    best = min(range(len(runs)), key=lambda r: (runs[r]["loss_num"], r))
    return sortlabels(runs[best]["labels"])


def lloyd(S, particles, orders, G, cap, maxiter, maxsweeps):
    P = [np.asarray(p, np.int64) for p in particles]
    trace, prev, converged, it = [], None, False, 0
    a, d, W = assign(vi_distances(np.stack(P), S, G))
    trace.append(W)
    while it < maxiter:
        it += 1
        repaired = False
        empty = [l for l in range(len(P)) if l not in a]
        if empty:
            if W == 0:
                break
            used = set()
            for l in empty:
                s = farthest(d, used)
                if s < 0:
                    break
                used.add(s)
                P[l] = sortlabels(S[s])
                repaired = True
            if repaired:
                a, d, W = assign(vi_distances(np.stack(P), S, G))
                trace.append(W)
        changed = False
        for l in sorted(set(a)):
            new = search_group(S, [s for s in range(len(S)) if a[s] == l], G, P[l], orders, cap, maxsweeps)
            if not np.array_equal(new, P[l]):
                P[l], changed = new, True
        if not changed and not repaired and prev == a:
            converged = True
            break
        prev = a
        a, d, W = assign(vi_distances(np.stack(P), S, G))
        trace.append(W)
    return dict(particles=P, assignment=a, d=d, W=W, trace=trace, iterations=it, converged=converged or W == 0)


def wasabi_ref(samples, L, G, nstarts=4, maxiter=50, nruns=1, maxK=0, maxsweeps=100, seed=0, init=None):
    """The driver: a dict with particles, weights, assignment, group_num, objective_num, trace, iterations, converged, start,
    starts — the fields of WasabiResult that are exact."""
    S = np.asarray(samples, np.int64)
    m, n = S.shape
    given = None if init is None else [sortlabels(c) for c in np.atleast_2d(np.asarray(init))]
    cap = maxK if maxK else max(len(set(r.tolist())) for r in list(S) + (given or []))
    rng = np.random.Generator(np.random.Philox(key=seed))
    orders = [rng.permutation(n) + 1 for _ in range(nruns)]
    runs = []
    for t in range(nstarts):
        u = np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, 0, t + 1])).integers(0, 1 << 53, size=L)
        runs.append(lloyd(S, seed_particles(S, L, u, G), orders, G, cap, maxiter, maxsweeps))
    if given is not None:
        runs.append(lloyd(S, given, orders, G, cap, maxiter, maxsweeps))
    starts = [r["W"] for r in runs]
    win = starts.index(min(starts))
    r = runs[win]
    sizes = [r["assignment"].count(l) for l in range(len(r["particles"]))]
    keep = sorted((l for l in range(len(sizes)) if sizes[l]), key=lambda l: (-sizes[l], l))
    assignment = [keep.index(l) for l in r["assignment"]]
    return dict(particles=np.stack([r["particles"][l] for l in keep]), weights=np.array([sizes[l] / m for l in keep]),
                assignment=np.array(assignment), group_num=[sum(x for x, g in zip(r["d"], assignment) if g == l) for l in range(len(keep))],
                objective_num=r["W"], wasserstein=r["W"] / (2.0 ** 32 * n * m), trace=r["trace"], iterations=r["iterations"],
                converged=r["converged"], start=win, starts=starts)


def scan_ref(samples, Ls, G, **kw):
    """wasabi_scan: ({L: result}, curve)"""
    S = np.asarray(samples, np.int64)
    out, prev = {}, None
    for L in sorted(set(Ls)):
        init = None
        if prev is not None:
            rows = list(prev["particles"])
            dist = vi_distances(prev["particles"], S, G)
            d = [dist[prev["assignment"][s]][s] for s in range(len(S))]
            used = set()
            while len(rows) < L:
                s = farthest(d, used)
                if s < 0:
                    break
                used.add(s)
                rows.append(sortlabels(S[s]))
            init = np.stack(rows)
        out[L] = prev = wasabi_ref(S, L, G, init=init, **kw)
    return out, np.array([out[L]["wasserstein"] for L in sorted(set(Ls))])


def planted_bimodal(n=40, m=48, nA=30, seed=0):
    """Two modes: A = arange(n) % 3 and B = arange(n) // 9 (labels from 1); nA noisy copies of A, then m − nA of B, each with 2..8
    random label flips (a point moved to another of the mode's labels)"""
    rng = np.random.default_rng(seed)
    A, B = np.arange(n) % 3 + 1, np.arange(n) // 9 + 1
    S = []
    for s in range(m):
        c = (A if s < nA else B).copy()
        names = np.unique(c)
        for j in rng.choice(n, size=int(rng.integers(2, 9)), replace=False):
            c[j] = rng.choice(names[names != c[j]])
        S.append(c)
    S = np.stack(S).astype(np.int64)
    S.setflags(write=False)
    return S, sortlabels(A), sortlabels(B)


def brute_force_pairs(S, G):
    """min over all unordered pairs of partitions of n points (n small) of Σ_s min(d(c1, s), d(c2, s)); and min over single
    partitions of Σ_s d(c, s)"""
    n = S.shape[1]
    parts = []

    def grow(prefix, k):
        if len(prefix) == n:
            parts.append(list(prefix))
            return
        for l in range(1, k + 2):
            grow(prefix + [l], max(k, l))
    grow([], 0)
    D = np.array(vi_distances(np.array(parts), S, G), dtype=np.int64)          # |parts| × m, each below 2^52
    best2 = min(int(np.minimum(D[i], D[i:]).sum(axis=1).min()) for i in range(len(parts)))
    return best2, int(D.sum(axis=1).min())
