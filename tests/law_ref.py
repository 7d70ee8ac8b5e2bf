"""Exact laws of the sampler's steps, and the statistics that hold counts of draws against them — TEST INFRASTRUCTURE,
host only (DESIGN.md "Testing the draws").

The parity tests hold the device bit for bit against restatements that consume the same Philox stream; an error both sides
share (a counter layout that correlates two draws, a noise transform slightly off, a seed word that never reaches the key, a
tie rule that shifts mass) passes them.  Here every step's outcome probabilities are computed from the transcription's own
scores — never from the library, never from a uniform — and the frequencies of what the device (or the oracle) drew are
held against them.

A law is a dict outcome -> probability (f64, summing to 1 within 1e-12).  Outcomes are tuples of Python ints."""
from __future__ import annotations

import math

import numpy as np

import kmeans_ref as KM
import np_transcription as T

P_BOUND = 1e-6            # every chi-square test fails beyond the upper 1e-6 quantile of chi2(df)
Z_BOUND = 4.9             # the same level, two-sided, for a standard normal (2·sf(4.9) = 0.96e-6)


def softmax(logprobs) -> np.ndarray:
    """The probabilities a Gumbel-max draw over logprobs realises.  A +inf entry takes everything; with a NaN the first NaN
    wins, as np.argmax has it."""
    lp = np.asarray(logprobs, dtype=np.float64)
    if np.isnan(lp).any():
        out = np.zeros(len(lp))
        out[int(np.flatnonzero(np.isnan(lp))[0])] = 1.0
        return out
    top = lp.max()
    if math.isinf(top) and top > 0:
        out = (lp == top).astype(np.float64)
        return out / out.sum()
    e = np.exp(lp - top)
    return e / e.sum()


def bound(df: int) -> float:
    from scipy.stats import chi2
    return float(chi2.isf(P_BOUND, df))


def pvalue(stat: float, df: int) -> float:
    from scipy.stats import chi2
    return float(chi2.sf(stat, df))


def _check(law: dict) -> dict:
    total = math.fsum(law.values())
    assert abs(total - 1.0) <= 1e-12, total
    return law


# ---------------------------------------------------------------------------------------------------------------
# The cases the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------
PARAMS = dict(delta1=2.0, delta2=3.0, alpha=4.0, beta=3.0, zeta=6.0, gamma=8.0, eta=1.0, sigma=1.0, u=1.0, v=1.0,
              repulsion=True, maxK=0)
R0, P0 = 1.5, 0.4
SEEDS = (12345, 0xC0FFEE00000005, 2 ** 64 - 1)
PERTURBED = {"p*1.05": dict(p=P0 * 1.05), "r*1.1": dict(r=R0 * 1.1), "delta1+0.1": dict(delta1=PARAMS["delta1"] + 0.1)}


def high_index(k: int) -> int:
    """Sweep indices with the high word set and the low word about to wrap."""
    return k * 2 ** 32 + 0xFFFFFFF0 + (k % 32)


def streams():
    """(seed, index map, name): every seed with sweep index k, the two with a high word also with high_index(k)."""
    out = [(s, int, f"{s:#x}") for s in SEEDS]
    return out + [(s, high_index, f"{s:#x}-high") for s in SEEDS[1:]]


def planted_points(n, groups=2, sep=1.5, sd=0.25, seed=5, wide=None):
    """n points in the plane, point i in planted group i mod groups, the groups' centres sep apart on a line, scattered with
    standard deviation sd — the last two points with `wide` instead, where it is given."""
    rng = np.random.default_rng(seed + n)
    g = np.arange(n) % groups
    sdv = np.where(np.arange(n) >= n - 2, sd if wide is None else wide, sd)
    X = rng.normal(0.0, 1.0, (n, 2)) * sdv[:, None] + np.c_[g * sep, np.zeros(n)]
    return X, (g + 1).astype(np.int64)


def distances(X):
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    return (D + D.T) / 2


def small_case(n):
    """(D, planted labels) of the n = 5 and n = 6 cases: two planted groups two units apart, each a tight core (sd 0.1), and
    the last two points scattered widely (sd 1.5), so that they keep moving between a group and a cluster of their own while
    the labels of the cores hold still.  The chain protocol needs both at once: few source states (at n = 6 the rows of
    at least 200 visits hold 91 % of 100 000 transitions) and transitions that are far from certain (its power against a
    law with p, r or delta1 slightly off).  The case was picked from a grid of spreads and data seeds on those two figures
    alone, measured on the oracle; agreement with the exact law was no criterion."""
    X, g = planted_points(n, sep=2.0, sd=0.1, seed=11, wide=1.5)
    return distances(X), g


def perturbed(name):
    """(params, r, p) of one of the three wrong laws of the power assertions"""
    d = PERTURBED[name]
    return dict(PARAMS, **{k: v for k, v in d.items() if k == "delta1"}), d.get("r", R0), d.get("p", P0)


# ---------------------------------------------------------------------------------------------------------------
# The Gibbs label sweep
# ---------------------------------------------------------------------------------------------------------------
def transcription_scores(D, P, r, p):
    logD = T.make_logD(D)
    return lambda clusts, sizes, i: T.point_scores(D, logD, clusts, sizes, P, r, p, i)


def oracle_scores(orc, r, p):
    """The same interface from Oracle.point_scores_stable (candidate scores up to one constant per point)."""
    def scores(clusts, sizes, i):
        orc.clusts[:] = clusts
        orc.sizes[:] = sizes
        return orc.point_scores_stable(r, p, i)
    return scores


def sweep_law(D, P, labels, r, p, depth=None, scores=None) -> dict:
    """The law of the labels of the first `depth` points (all n by default) after one sweep from `labels`: the tree of
    point_scores' candidates, each taken with the softmax of its logprobs, walked depth first."""
    labels = np.asarray(labels, dtype=np.int64)
    n = len(labels)
    depth = n if depth is None else int(depth)
    scores = transcription_scores(D, P, r, p) if scores is None else scores
    law: dict = {}

    def walk(clusts, sizes, i, mass):
        if i == depth:
            key = tuple(int(x) for x in clusts[:depth])
            law[key] = law.get(key, 0.0) + mass
            return
        cands, lp = scores(clusts, sizes, i)
        pr = softmax(lp)
        for c, q in zip(cands, pr):
            if q == 0.0:
                continue
            c2, s2 = clusts.copy(), sizes.copy()
            s2[c2[i] - 1] -= 1
            c2[i] = c
            s2[c - 1] += 1
            walk(c2, s2, i + 1, mass * float(q))

    walk(labels.copy(), T.state_from_labels(labels)[0], 0, 1.0)
    return _check(law)


def sweep_law2(D, P, labels, r, p, law_of=None) -> dict:
    """The law of the labelling after two consecutive sweeps: sweep_law composed with itself."""
    law_of = (lambda lab: sweep_law(D, P, lab, r, p)) if law_of is None else law_of
    out: dict = {}
    for mid, q in law_of(tuple(int(x) for x in labels)).items():
        for end, q2 in law_of(mid).items():
            out[end] = out.get(end, 0.0) + q * q2
    return _check(out)


class LawCache:
    """sweep_law per source state, computed once: the chain protocol asks for the same rows again and again."""

    def __init__(self, D, P, r, p):
        self.D, self.P, self.r, self.p, self.laws, self.nodes = D, P, r, p, {}, {}
        self.fresh = transcription_scores(D, P, r, p)

    def scores(self, clusts, sizes, i):
        """point_scores per (labels, point), computed once: the trees of different source states share nodes"""
        key = (clusts.tobytes(), i)
        if key not in self.nodes:
            self.nodes[key] = self.fresh(clusts, sizes, i)
        return self.nodes[key]

    def __call__(self, labels) -> dict:
        key = tuple(int(x) for x in labels)
        if key not in self.laws:
            self.laws[key] = sweep_law(self.D, self.P, np.array(key, np.int64), self.r, self.p, scores=self.scores)
        return self.laws[key]


# ---------------------------------------------------------------------------------------------------------------
# One split–merge proposal
# ---------------------------------------------------------------------------------------------------------------
def splitmerge_law(D, P, labels, r, p, numGibbs, mode) -> dict:
    """The law of (accept, split, labelling afterwards) of one proposal, by enumerating np_transcription.mh_proposal: the
    n(n-1) ordered pairs, the 2^|S| launch allocations, every choice of the numGibbs restricted scans with the probability
    the Gumbel-max realises, the final scan (free for a split, forced for a merge), and acceptance with probability
    exp(min(0, x)) — 0 where x is NaN, as the code as written has it.  mode "intended": an accepted proposal becomes the
    state; "as_written": the caller's labels never change (quirk Q1), so only the flags carry the law."""
    assert mode in ("as_written", "intended")
    labels = np.asarray(labels, dtype=np.int64)
    n = len(labels)
    logD = T.make_logD(D)
    sizes, K = T.state_from_labels(labels)
    before = tuple(int(x) for x in labels)
    law: dict = {}

    def add(key, mass):
        if mass > 0.0:
            law[key] = law.get(key, 0.0) + mass

    def scans(cl, sz, S, cand, left, mass, leaf):
        """every outcome of `left` free restricted scans from (cl, sz): leaf(cl, sz, mass, ltp of the last scan)"""
        if left == 0:
            leaf(cl, sz, mass, 0.0)
            return
        C, cinds = T.restricted_frame(sz, cand)

        def item(cl, sz, q, mass, ltp):
            if q == len(S):
                if left == 1:
                    leaf(cl, sz, mass, ltp)
                else:
                    scans(cl, sz, S, cand, left - 1, mass, leaf)
                return
            cl, sz = cl.copy(), sz.copy()
            lp = T.restricted_item(D, logD, cl, sz, P, r, p, S[q], cand, C, cinds)
            pr = softmax(lp)
            lp = lp - lp.min()                                # what sample_logweights leaves behind
            for k in range(2):
                if pr[k] == 0.0:
                    continue
                c2, s2 = cl.copy(), sz.copy()
                t = T.restricted_place(c2, s2, S[q], cand, k, lp)
                item(c2, s2, q + 1, mass * float(pr[k]), ltp + t)

        item(cl, sz, 0, mass, 0.0)

    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                launch = T.mh_launch(labels, sizes, K, P, i, j)
                m_pair = 1.0 / (n * (n - 1))
                if launch is None:
                    add((False, False, before), m_pair)
                    continue
                S, claunch0, szlaunch0, Klaunch, cand = launch
                for bits in range(1 << len(S)):
                    claunch, szlaunch = claunch0.copy(), szlaunch0.copy()
                    for q, k in enumerate(S):
                        T.mh_allocate(labels, claunch, szlaunch, k, cand[(bits >> q) & 1])
                    m_launch = m_pair / (1 << len(S))

                    def after_gibbs(cl, sz, mass, _ltp):
                        def finish(cl, sz, mass, ltp_free):
                            def final_scan(cl2, sz2, final_clusts):
                                if final_clusts is None:       # the free scan was enumerated by the caller
                                    return ltp_free
                                return T.restricted_scan(D, logD, cl2, sz2, P, r, p, S, cand, final_clusts, 0, 0, 0, numGibbs)
                            split, final, _, _, _, x = T.mh_finish(D, logD, labels, sizes, K, P, r, p, i, j, S, cl, sz, Klaunch,
                                                                   cand, final_scan)
                            acc = 0.0 if np.isnan(x) else math.exp(min(0.0, float(x)))
                            after = tuple(int(v) for v in final[0]) if mode == "intended" else before
                            add((True, split, after), mass * acc)
                            add((False, split, before), mass * (1.0 - acc))

                        if labels[i] == labels[j]:
                            scans(cl, sz, S, cand, 1, mass, finish)            # the final scan of a split is free
                        else:
                            finish(cl.copy(), sz.copy(), mass, 0.0)

                    scans(claunch, szlaunch, S, cand, numGibbs, m_launch, after_gibbs)
    return _check(law)


# ---------------------------------------------------------------------------------------------------------------
# The seeding draws of the prior fits
# ---------------------------------------------------------------------------------------------------------------
def _seeding_law(n, k, first_costs, later_costs, weights) -> dict:
    law: dict = {}

    def walk(seeds, mincost, mass):
        if len(seeds) == k:
            law[tuple(seeds)] = law.get(tuple(seeds), 0.0) + mass
            return
        q = weights(mincost)
        W = int(q.sum())
        assert W > 0, "every weight of the draw is zero"
        for j in np.flatnonzero(q > 0):
            mc = later_costs(mincost, int(j))
            walk(seeds + [int(j)], mc, mass * (int(q[j]) / W))

    for s in range(n):
        walk([s], first_costs(s), 1.0 / n)
    return _check(law)


def _tilted(weights, tilt):
    """weights with the weight of point tilt[0] scaled by tilt[1] in every draw: a deliberately wrong law (power checks)"""
    if tilt is None:
        return weights

    def w(mincost):
        q = weights(mincost).astype(np.float64)
        q[tilt[0]] *= tilt[1]
        return np.floor(q / 1024.0).astype(np.int64)            # one scale for all, small enough for exact integer sums
    return w


def kmeanspp_law(X, k, tilt=None) -> dict:
    """The law of k-means++'s seed sequence (0-based point indices): the first uniform, each later seed j with probability
    q_j / W, q = kmeans_ref.draw_weights of the squared distance to the nearest seed so far."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    shift = KM.draw_shift(X)

    def first(s):
        mc = KM.sqdist(X, X[s:s + 1])[:, 0]
        mc[s] = 0.0
        return mc

    def later(mc, j):
        mc = np.minimum(mc, KM.sqdist(X, X[j:j + 1])[:, 0])
        mc[j] = 0.0
        return mc

    return _seeding_law(X.shape[0], k, first, later, _tilted(lambda w: KM.draw_weights(w, shift), tilt))


def kmedoidspp_law(Dq, k, tilt=None) -> dict:
    """The law of k-medoids++'s seed sequence on the fixed-point matrix: the weights are its integer costs themselves."""
    Dq = np.asarray(Dq, dtype=np.int64)

    def first(s):
        mc = Dq[s].copy()
        mc[s] = 0
        return mc

    def later(mc, j):
        mc = np.minimum(mc, Dq[j])
        mc[j] = 0
        return mc

    return _seeding_law(Dq.shape[0], k, first, later, _tilted(lambda w: w, tilt))


# ---------------------------------------------------------------------------------------------------------------
# Statistics
# ---------------------------------------------------------------------------------------------------------------
def count(outcomes) -> dict:
    out: dict = {}
    for key in outcomes:
        out[key] = out.get(key, 0) + 1
    return out


def chi2_against(counts: dict, law: dict, N: int, emin: float = 10):
    """Pearson's statistic of `counts` (outcome -> count, N draws) against `law` over the outcomes of expected count >= emin,
    the rest pooled into one cell; a pooled cell below emin joins the smallest kept cell.  An outcome the law gives no
    probability at all makes the statistic infinite.  Returns (statistic, degrees of freedom, share of N in unpooled cells)."""
    assert sum(counts.values()) == N
    if any(law.get(key, 0.0) <= 0.0 for key in counts):
        return math.inf, 1, 0.0
    kept = sorted((key for key, q in law.items() if N * q >= emin), key=lambda key: (law[key], key))
    E = [N * law[key] for key in kept]
    O = [counts.get(key, 0) for key in kept]
    share = sum(O) / N
    e_pool, o_pool = N - math.fsum(E), N - sum(O)
    if len(kept) < len(law) or o_pool:
        if e_pool >= emin or not kept:
            E.append(e_pool); O.append(o_pool)
        else:                                                  # kept is sorted by expectation: [0] is the smallest
            E[0] += e_pool; O[0] += o_pool
    stat = math.fsum((o - e) ** 2 / e for o, e in zip(O, E))
    return stat, max(len(E) - 1, 1), share


def chi2_transitions(trans: dict, law_of, emin: float = 10, min_visits: int = 200):
    """chi2_against summed over the source states of `trans` (source -> {destination -> count}) with at least min_visits
    visits, each row against law_of(source); the degrees of freedom add.  Returns (statistic, degrees of freedom, share of
    all transitions in the rows used)."""
    stat, df, used, total = 0.0, 0, 0, 0
    for src in sorted(trans):
        visits = sum(trans[src].values())
        total += visits
        if visits < min_visits:
            continue
        s, d, _ = chi2_against(trans[src], law_of(src), visits, emin)
        stat += s; df += d; used += visits
    return stat, df, used / max(total, 1)


def transitions(path) -> dict:
    """source -> {destination -> count} of consecutive states of a chain (a sequence of label tuples)."""
    trans: dict = {}
    for a, b in zip(path[:-1], path[1:]):
        row = trans.setdefault(a, {})
        row[b] = row.get(b, 0) + 1
    return trans


def calibration(device_path, oracle):
    """For sizes at which the tree cannot be walked.  device_path: (r, p, labels before, labels after) of each sweep the
    device made.  Every visit is replayed on the oracle at the labels the device actually drew (points < i after, points
    >= i before): point_scores_stable gives the candidates' probabilities, and the visit records p_top of the most probable
    candidate and whether it was drawn, p_new of the new-cluster candidate and whether it was drawn.
    Z = (Σ hit − Σ p) / sqrt(Σ p(1 − p)) is a martingale sum, about N(0, 1) whatever the path.
    Returns dict(z_top, z_new, visits, new_visits, median_p_top)."""
    import ctypes
    n = oracle.n
    top_s, new_s = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]            # Σ hit, Σ p, Σ p(1 − p)
    ptops, new_visits = [], 0
    cands, sc = np.zeros(n + 1, np.int64), np.zeros(n + 1)
    Dq, Lq = oracle.Dq.reshape(-1), oracle.Lq.reshape(-1)
    score, par = oracle.L.orc_point_scores_stable, ctypes.byref(oracle.P)
    for r, p, before, after in device_path:
        oracle.set_state(before)
        clusts, sizes = oracle.clusts, oracle.sizes
        for i in range(n):
            m = score(n, Dq, Lq, oracle.eD, oracle.eL, oracle.A, clusts, sizes, par, r, p, i, cands, sc)
            cl, pr = cands[:m].tolist(), softmax(sc[:m]).tolist()
            drawn, old = int(after[i]), int(clusts[i])
            assert drawn in cl, (i, drawn, cl)
            q = max(pr)
            top_s[0] += cl[pr.index(q)] == drawn; top_s[1] += q; top_s[2] += q * (1.0 - q)
            ptops.append(q)
            last = cl[-1]
            if sizes[last - 1] - (last == old) == 0:            # the last candidate is the new cluster (empty once i has left)
                q = pr[-1]
                new_s[0] += last == drawn; new_s[1] += q; new_s[2] += q * (1.0 - q)
                new_visits += 1
            sizes[old - 1] -= 1
            clusts[i] = drawn
            sizes[drawn - 1] += 1
        assert np.array_equal(clusts, after)
    acc, visits = {"top": top_s, "new": new_s}, len(ptops)
    z = {k: (a[0] - a[1]) / math.sqrt(a[2]) if a[2] > 0 else 0.0 for k, a in acc.items()}
    return dict(z_top=z["top"], z_new=z["new"], visits=visits, new_visits=new_visits, median_p_top=float(np.median(ptops)))


# ---------------------------------------------------------------------------------------------------------------
# Protocols: how draws are collected, from the oracle or from the device alike
# ---------------------------------------------------------------------------------------------------------------
def as_key(labels) -> tuple:
    return tuple(int(x) for x in labels)


def restart_counts(sweep_from, seed, index, N, take=None) -> dict:
    """Restart protocol: sweep_from(seed, s) makes one sweep from the same start with sweep index s = index(k), k < N, and
    returns the labels; the outcomes (their first `take` labels) are counted."""
    return count(as_key(sweep_from(seed, index(k))[:take]) for k in range(N))


def chain_path(sweep, start, seed, N) -> list:
    """Chain protocol: sweep(seed, s) advances a free-running chain by sweep s = 0..N-1 and returns the labels."""
    return [as_key(start)] + [as_key(sweep(seed, s)) for s in range(N)]


def oracle_restart(orc, start, r, p):
    def sweep_from(seed, s):
        orc.set_state(start)
        orc.sweep_stable(r, p, seed, s)
        return orc.clusts
    return sweep_from


def oracle_chain(orc, start, r, p):
    orc.set_state(start)

    def sweep(seed, s):
        orc.sweep_stable(r, p, seed, s)
        return orc.clusts
    return sweep


def report(name, stat, df, **more) -> str:
    """One line per test for the record (DESIGN.md "Testing the draws"); printed before the assertion."""
    line = f"LAW {name}: stat={stat:.2f} df={df} bound={bound(df):.2f} p={pvalue(stat, df):.3g}"
    line += "".join(f" {k}={v:.4g}" if isinstance(v, float) else f" {k}={v}" for k, v in more.items())
    print(line)
    return line


def assert_consistent(name, counts, law, N, min_share=0.9, **more):
    stat, df, share = chi2_against(counts, law, N)
    report(name, stat, df, N=N, share=share, **more)
    assert share >= min_share, (name, share)
    assert stat <= bound(df), (name, stat, df, bound(df))
    return stat, df


def assert_rejected(name, counts, law, N, **more):
    stat, df, _ = chi2_against(counts, law, N)
    report(name + " [wrong law, must be rejected]", stat, df, N=N, **more)
    assert stat > bound(df), (name, stat, df, bound(df))


# ---------------------------------------------------------------------------------------------------------------
# Laws of the shared cases, computed once per process (the CPU and the GPU tests ask for the same ones)
# ---------------------------------------------------------------------------------------------------------------
_LAWS: dict = {}


def law_cache(n, which="exact") -> LawCache:
    """The sweep laws of small_case(n) under the true parameters ("exact") or one of PERTURBED."""
    if (n, which) not in _LAWS:
        params, r, p = (PARAMS, R0, P0) if which == "exact" else perturbed(which)
        _LAWS[n, which] = LawCache(small_case(n)[0], params, r, p)
    return _LAWS[n, which]


def small_law2(n) -> dict:
    if ("law2", n) not in _LAWS:
        D, start = small_case(n)
        _LAWS["law2", n] = sweep_law2(D, PARAMS, start, R0, P0, law_of=law_cache(n))
    return _LAWS["law2", n]


SM_STATES = {"merge": (1, 2, 3, 2, 1),     # two clusters of the first planted group (points 0, 2, 4): merges are likely
             "split": (1, 1, 1, 1, 1)}     # one cluster over both groups: every proposal is a split
SM_N = 5


def sm_law(state, mode="intended", r=R0) -> dict:
    if ("sm", state, mode, r) not in _LAWS:
        _LAWS["sm", state, mode, r] = splitmerge_law(small_case(SM_N)[0], PARAMS, np.array(SM_STATES[state], np.int64), r, P0,
                                                     1, mode)
    return _LAWS["sm", state, mode, r]


def seeding_points(case):
    """n = 8 points for the seeding laws.  "coincident": points 2 and 5 coincide, so a weight of zero occurs (the library
    refuses such data, so only the restatements see it); "close": they lie 1e-6 apart and point 7 lies 600 away, which the library
    accepts; the far point stretches the bounding box until the pair's squared distance, 1e-12, quantises to a k-means++
    weight of zero (floor(1e-12 · 2^39) = 0)."""
    X = planted_points(8, sep=1.0, sd=0.5)[0]
    if case == "coincident":
        X[5] = X[2]
    elif case == "close":
        X[5] = X[2] + np.array([1e-6, 0.0])
        X[7] = [600.0, 0.0]
    else:
        assert case == "plain"
    return X


def seeding_counts(draw, N) -> dict:
    """seed sequences of draw(s) for s < N and for 2^40 + s (the high seed word in play)"""
    return count(tuple(int(x) for x in draw(s)) for base in (0, 2 ** 40) for s in range(base, base + N))


# ---------------------------------------------------------------------------------------------------------------
# The oracle's draws for the shared cases, computed once per process
# ---------------------------------------------------------------------------------------------------------------
_ORACLE: dict = {}


def small_oracle(n):
    import oracle_lib as O
    return O.Oracle(small_case(n)[0], PARAMS)


def oracle_restart_counts(n, seed, index, N) -> dict:
    key = ("restart", n, seed, index(1), N)
    if key not in _ORACLE:
        _ORACLE[key] = restart_counts(oracle_restart(small_oracle(n), small_case(n)[1], R0, P0), seed, index, N)
    return _ORACLE[key]


def oracle_chain_path(seed, N) -> list:
    """the oracle's free-running chain at n = 6 from the planted labels"""
    if ("chain", seed, N) not in _ORACLE:
        start = small_case(6)[1]
        _ORACLE["chain", seed, N] = chain_path(oracle_chain(small_oracle(6), start, R0, P0), start, seed, N)
    return _ORACLE["chain", seed, N]


def oracle_proposals(state, seed, N) -> list:
    """(accept, split, labels afterwards) of Oracle.mh_proposal (stable arithmetic, numGibbs = 1) from SM_STATES[state],
    iteration counter 0..N-1"""
    if ("sm", state, seed, N) not in _ORACLE:
        orc = small_oracle(SM_N)
        start = np.array(SM_STATES[state], np.int64)
        outs = []
        for it in range(N):
            orc.set_state(start)
            inf = orc.mh_proposal(R0, P0, 1, seed, it, 0, mode=1)
            outs.append((bool(inf.accept), bool(inf.split), as_key(orc.clusts)))
        _ORACLE["sm", state, seed, N] = outs
    return _ORACLE["sm", state, seed, N][:N]


LARGE_R, LARGE_P = 1.5, 0.4


def large_case(n):
    """(D, params, planted labels) at the sizes where the tree cannot be walked: three planted groups on a line, their
    centres one unit apart, scattered with sd 3 (n < 1000) or 8, so that most visits are far from certain (median p_top
    0.82 at n = 135 and 0.86 at n = 1029, asserted below 0.9 where the chain is replayed); hyperparameters fitted to the planted labels as the other tests fit them."""
    if ("large", n) not in _LAWS:
        X, g = planted_points(n, groups=3, sep=1.0, sd=3.0 if n < 1000 else 8.0)
        D = distances(X)
        _LAWS["large", n] = (D, T.likelihood_hyperparams(D, g), g)
    return _LAWS["large", n]


def device_path(sweep, start, r, p, seed, nsweeps) -> list:
    """the (r, p, labels before, labels after) records calibration() takes, from a free-running chain"""
    path, before = [], np.asarray(start, dtype=np.int64).copy()
    for s in range(nsweeps):
        after = np.asarray(sweep(seed, s), dtype=np.int64).copy()
        path.append((r, p, before, after))
        before = after
    return path
