"""NumPy restatement of one run of the MAP search (csrc/mapsearch.inc.hip, include/redclust_hip.h rc_map_search, DESIGN.md §8
"MAP search") — TEST INFRASTRUCTURE, not product code.

It takes a context's integer matrices (Dq = D·2^eD, Lq = logD·2^eL in the caller's order: score_ref.quantised of
Context.get_matrix, or the C oracle's quantisation where there is no device), keeps the K×K block sums as Python integers in
object arrays and updates them by adding and subtracting row sums, and computes every Δ in float64 with math.lgamma and
math.log1p.  search() returns the labels, the record, the blocks and min_gap — the smallest difference between the best and the
second-best candidate over every visit of the run, "stay" included — which the CPU suite holds above 1e-6 on every fixed input
of the GPU tests: the device's Δ differ from these by rounding only, so exact equality of the labels is a fair demand of it
only where no decision is closer than that.  The fixed inputs of the GPU tests are defined at the end."""
import functools
import math

import numpy as np

_LG = np.frompyfunc(math.lgamma, 1, 1)
_L1P = np.frompyfunc(math.log1p, 1, 1)


def _f(x):
    """Python integers (or an object array of them) as float64, each rounded once"""
    return np.asarray(x, dtype=object).astype(np.float64)


def _term(d, a0, base, pairs, bd, bl):
    """within (d, a0, base = δ1, α, β; the halved block) or between (δ2, ζ, γ) plus the constant lgΓ(a0), in the regrouped form:
    (d−1)·bl − pairs·lgΓ(d) + lgΓ(a0+d·pairs) − d·pairs·log(base) − (a0+d·pairs)·log1p(bd/base)"""
    pairs, bd, bl = (np.asarray(x, dtype=np.float64) for x in (pairs, bd, bl))
    a = a0 + d * pairs
    return ((d - 1.0) * bl - pairs * math.lgamma(d) + np.asarray(_LG(a), dtype=np.float64) - d * pairs * math.log(base)
            - a * np.asarray(_L1P(bd / base), dtype=np.float64))


def compact(z):
    """labels 0..n (0 = unallocated) as slots 1..K by first appearance"""
    out, names = np.zeros(len(z), np.int64), {}
    for j, l in enumerate(z):
        if l:
            out[j] = names.setdefault(int(l), len(names) + 1)
    return out, len(names)


def sortlabels(z):
    return compact(z)[0]


def blocks_of(Dq, Lq, slots, Kcap):
    """(B_D, B_L): (Kcap+1)² object arrays of Python integers, B[k][t] = Σ_{i in k, j in t} Xq[i][j], D's diagonal included"""
    K = int(slots.max()) if len(slots) else 0
    M = (slots[:, None] == np.arange(K + 1)[None, :]).astype(np.int64)    # only the slots in use: the rest of B stays 0
    M[:, 0] = 0
    out = []
    for X in (Dq, Lq):
        R = np.asarray(X, dtype=np.int64) @ M                           # row sums: they fit int64
        B = np.zeros((Kcap + 1, Kcap + 1), dtype=object)
        for k in range(1, K + 1):
            rows = np.flatnonzero(slots == k)
            if len(rows):
                B[k, :K + 1] = R[rows].astype(object).sum(axis=0)
        out.append(B)
    return out


def logposterior(Dq, Lq, eD, eL, z, r, p, P):
    """lp of a labelling (0 = unallocated: such points do not exist) from its exact blocks, float64: the issue's criterion"""
    slots, K = compact(np.asarray(z))
    BD, BL = blocks_of(Dq, Lq, slots, max(K, 1))
    sz = np.bincount(slots, minlength=K + 1)
    fD, fL = math.ldexp(1.0, -eD), math.ldexp(1.0, -eL)
    lp = 0.0
    for k in range(1, K + 1):
        nk = int(sz[k])
        lp += float(_term(P["delta1"], P["alpha"], P["beta"], nk * (nk - 1) / 2, float(BD[k, k]) * fD / 2, float(BL[k, k]) * fL / 2)) - math.lgamma(P["alpha"])
        if P.get("repulsion", True):
            for t in range(k + 1, K + 1):
                lp += float(_term(P["delta2"], P["zeta"], P["gamma"], nk * int(sz[t]), float(BD[k, t]) * fD, float(BL[k, t]) * fL)) - math.lgamma(P["zeta"])
    n1 = int((slots > 0).sum())
    lp += math.lgamma(K + 1) + (n1 - K) * math.log(p) + r * K * math.log1p(-p) - K * math.lgamma(r)
    for k in range(1, K + 1):
        lp += math.log(float(sz[k])) + math.lgamma(float(sz[k]) + r - 1)
    eta, sigma, u, v = (float(P.get(x, 1.0)) for x in ("eta", "sigma", "u", "v"))
    lp += eta * math.log(sigma) - math.lgamma(eta) + (eta - 1) * math.log(r) - sigma * r
    lp += math.lgamma(u + v) - math.lgamma(u) - math.lgamma(v) + (u - 1) * math.log(p) + (v - 1) * math.log1p(-p)
    return lp


def search(Dq, Lq, eD, eL, init, order, r, p, P, maxK=0, maxsweeps=100, max_visits=None, trace=None):
    """One run.  init: labels 0..n; order: a 1-based permutation.  Returns a dict: labels (sortlabels'd), slots (1-based, as the
    kernel ends), sweeps, moves, converged, K, capped, Kcap, BD, BL ((Kcap+1)² object arrays by slot, row and column 0 unused),
    min_gap.  max_visits: stop after that many visits (the record is then partial); trace: a list that receives per visit
    (i, the slots with i out, the chosen slot)."""
    Dq, Lq = np.asarray(Dq, dtype=np.int64), np.asarray(Lq, dtype=np.int64)
    n = len(init)
    rep = bool(P.get("repulsion", True))
    d1, al, be, d2, ze, ga = (float(P[k]) for k in ("delta1", "alpha", "beta", "delta2", "zeta", "gamma"))
    fD, fL = math.ldexp(1.0, -eD), math.ldexp(1.0, -eL)
    Kcap = int(maxK) if maxK > 0 else min(n, 1024)
    slot, K = compact(np.asarray(init))
    assert K <= Kcap
    sz = np.bincount(slot, minlength=Kcap + 2).astype(np.int64)
    sz[0] = 0
    BD, BL = blocks_of(Dq, Lq, slot, Kcap)
    logp, rl1mp = math.log(p), r * math.log1p(-p)
    min_gap, moves, sweeps, converged, capped, visits = math.inf, 0, 0, 0, 0, 0
    done = False
    while not done:
        moved = 0
        for i in (int(o) - 1 for o in order):
            a = int(slot[i])
            mask = slot > 0
            mask[i] = False
            s, l = np.zeros(Kcap + 1, np.int64), np.zeros(Kcap + 1, np.int64)
            np.add.at(s, slot[mask], Dq[i][mask])
            np.add.at(l, slot[mask], Lq[i][mask])
            S, Lo = s.astype(object), l.astype(object)
            dii = int(Dq[i, i])
            nk_all = sz.copy()
            if a:
                nk_all[a] -= 1
            occ = np.flatnonzero(nk_all[1:Kcap + 1] > 0) + 1
            Know = len(occ)
            nk = nk_all[occ].astype(np.float64)
            so, lo = S[occ], Lo[occ]
            # the within blocks with i out, and with i in each candidate
            wd, wl = BD[occ, occ].copy(), BL[occ, occ].copy()
            if a and nk_all[a] > 0:
                ia = int(np.searchsorted(occ, a))
                wd[ia] -= 2 * so[ia] + dii
                wl[ia] -= 2 * lo[ia]
            cands = []
            if Know:
                pk = nk * (nk - 1) / 2
                delta = (_term(d1, al, be, pk + nk, _f(wd + 2 * so + dii) * fD / 2, _f(wl + 2 * lo) * fL / 2)
                         - _term(d1, al, be, pk, _f(wd) * fD / 2, _f(wl) * fL / 2))
                if rep and Know > 1:
                    bd, bl = BD[np.ix_(occ, occ)].copy(), BL[np.ix_(occ, occ)].copy()
                    if a and nk_all[a] > 0:
                        bd[ia, :] -= so; bd[:, ia] -= so
                        bl[ia, :] -= lo; bl[:, ia] -= lo
                    pairs = nk[:, None] * nk[None, :]
                    diff = (_term(d2, ze, ga, pairs + nk[None, :], _f(bd + so[None, :]) * fD, _f(bl + lo[None, :]) * fL)
                            - _term(d2, ze, ga, pairs, _f(bd) * fD, _f(bl) * fL))
                    np.fill_diagonal(diff, 0.0)
                    delta = delta + diff.sum(axis=1)
                delta = delta + (np.log(nk + 1) - np.log(nk) + np.log(nk + r - 1) + logp)
                cands = [(-float(delta[x]), 0 if int(occ[x]) == a else int(occ[x]), int(occ[x])) for x in range(Know)]
            emptied = bool(a) and nk_all[a] == 0
            if Know < Kcap:
                dn = float(_term(d1, al, be, 0.0, dii * fD / 2, 0.0)) - math.lgamma(al)
                if rep and Know:
                    dn += float((_term(d2, ze, ga, nk, _f(so) * fD, _f(lo) * fL) - math.lgamma(ze)).sum())
                dn += math.log(Know + 1) + rl1mp
                free = a if emptied else int(np.flatnonzero(nk_all[1:Kcap + 1] == 0)[0]) + 1
                cands.append((-dn, 0 if emptied else free, free))
            elif maxK == 0:
                capped += 1
            cands.sort()
            if len(cands) > 1:
                min_gap = min(min_gap, cands[1][0] - cands[0][0])
            w = cands[0][2]
            if trace is not None:
                out = slot.copy(); out[i] = 0
                trace.append((i, out, w))
            if w != a:
                if a:
                    BD[a, :] -= S; BD[:, a] -= S; BD[a, a] -= dii
                    BL[a, :] -= Lo; BL[:, a] -= Lo
                    sz[a] -= 1
                BD[w, :] += S; BD[:, w] += S; BD[w, w] += dii
                BL[w, :] += Lo; BL[:, w] += Lo
                sz[w] += 1
                slot[i] = w
                moved += 1
            visits += 1
            if max_visits is not None and visits >= max_visits:
                done = True
                break
        if done:
            break
        sweeps += 1
        moves += moved
        if not moved:
            converged = 1
            break
        if sweeps >= maxsweeps:
            break
    return dict(labels=sortlabels(slot), slots=slot.copy(), sweeps=sweeps, moves=moves, converged=converged,
                K=int((sz[1:Kcap + 1] > 0).sum()), capped=capped, Kcap=Kcap, BD=BD, BL=BL, min_gap=min_gap)


# ---------------------------------------------------------------------------------------------------------------
# The fixed inputs of the GPU tests (tests/test_gpu_mapsearch.py); tests/test_mapsearch_cpu.py holds the reference's gaps on them.
# ---------------------------------------------------------------------------------------------------------------
P0 = dict(delta1=2.0, alpha=8.0, beta=3.0, delta2=3.0, zeta=6.0, gamma=4.0, eta=2.0, sigma=1.5, u=2.0, v=3.0, repulsion=True, maxK=0)


def planted(n, K, sigma, seed, dim=3):
    """(D, the planted labels 1..K): K centres on the unit sphere, Gaussian noise around them"""
    g = np.random.default_rng(seed)
    cen = g.normal(size=(K, dim))
    cen /= np.linalg.norm(cen, axis=1)[:, None]
    z = g.integers(0, K, n)
    X = cen[z] + sigma * g.normal(size=(n, dim))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    D = np.maximum(D, D.T)
    np.fill_diagonal(D, 0.0)
    return D, z.astype(np.int64) + 1


def starts(n, K, truth, seed, kinds):
    g = np.random.default_rng(1000 + seed)
    rows = dict(empty=np.zeros(n, np.int64), planted=truth.copy(),
                noisy=np.where(g.random(n) < 0.3, g.integers(1, K + 3, n), truth).astype(np.int64),
                one=np.ones(n, np.int64), singletons=np.arange(1, n + 1, dtype=np.int64))
    init = np.stack([rows[k] for k in kinds])
    order = np.stack([g.permutation(n) + 1 for _ in kinds]).astype(np.int32)
    return init, order


ALL_STARTS = ("empty", "planted", "noisy", "one", "singletons")
# name: (n, planted K, sigma, seed, starts, r, p, maxK, maxsweeps, overrides of P0, diagonal)
SHAPES = {
    "n1": (1, 1, 0.3, 11, ("empty", "one"), 1.5, 0.1, 0, 100, {}, None),
    "n2": (2, 1, 0.3, 12, ("empty", "one", "singletons"), 1.5, 0.1, 0, 100, {}, None),
    "n63": (63, 3, 0.25, 13, ("empty", "planted", "noisy"), 1.5, 0.1, 0, 100, {}, None),
    "n64": (64, 3, 0.25, 14, ("empty", "planted", "noisy"), 1.5, 0.1, 0, 100, {}, None),
    "n65": (65, 3, 0.25, 15, ("empty", "planted", "noisy"), 1.5, 0.1, 0, 100, {}, None),
    "n257": (257, 8, 0.15, 3, ("empty", "planted", "noisy", "one"), 1.5, 0.1, 0, 100, {}, None),
    "n1025": (1025, 8, 0.15, 4, ("noisy",), 1.5, 0.1, 0, 2, {}, None),
    "n130": (130, 5, 0.3, 2, ALL_STARTS, 1.5, 0.1, 0, 100, {}, None),
    "maxK3": (130, 5, 0.3, 2, ("empty", "one"), 1.5, 0.1, 3, 100, {}, None),
    "norep": (130, 5, 0.3, 5, ALL_STARTS, 1.5, 0.5, 0, 100, dict(repulsion=False, alpha=20.0), None),
    "diag": (130, 5, 0.3, 6, ("empty", "planted", "noisy"), 1.5, 0.1, 0, 100, {}, "positive"),
}


def case(name):
    """dict(D, P, init, order, r, p (one per run), maxK, maxsweeps)"""
    if name == "capped":
        return capped_case()
    n, K, sigma, seed, kinds, r, p, maxK, maxsweeps, over, diag = SHAPES[name]
    D, truth = planted(n, K, sigma, seed)
    if diag:
        from helpers import with_diagonal
        D = with_diagonal(D, diag)
    init, order = starts(n, K, truth, seed, kinds)
    nr = len(kinds)
    return dict(D=D, P=dict(P0, **over), init=init, order=order, r=r + 0.25 * np.arange(nr), p=np.full(nr, p), maxK=maxK, maxsweeps=maxsweeps)


def capped_case():
    """n = 1100 points 50 apart on a line (jittered), no repulsion, a small p: every point wants a cluster of its own, the
    implicit cap of 1024 slots withholds it from the last 76 visits of the one sweep."""
    n = 1100
    g = np.random.default_rng(77)
    x = 50.0 * np.arange(n) + g.uniform(-10, 10, n)
    D = np.abs(x[:, None] - x[None, :])
    order = (g.permutation(n) + 1).astype(np.int32)[None, :]
    return dict(D=D, P=dict(P0, repulsion=False), init=np.zeros((1, n), np.int64), order=order, r=np.array([1.5]), p=np.array([0.01]),
                maxK=0, maxsweeps=1)


CASES = tuple(SHAPES) + ("capped",)


def run_case(c, Dq, Lq, eD, eL):
    """the reference's runs of a case on the given integer matrices"""
    return [search(Dq, Lq, eD, eL, c["init"][q], c["order"][q], float(c["r"][q]), float(c["p"][q]), c["P"], c["maxK"], c["maxsweeps"])
            for q in range(len(c["init"]))]


@functools.lru_cache(maxsize=None)
def host_ref(name):
    """(case, runs) on the C oracle's 64-bit quantisation of D and log D — what a context with a stored log holds, up to the
    exponents the library caps — for the tests that have no device"""
    import oracle_lib as O
    c = case(name)
    orc = O.Oracle(c["D"], c["P"])
    return c, run_case(c, orc.Dq, orc.Lq, orc.eD, orc.eL), orc
