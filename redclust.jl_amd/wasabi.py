"""Several-partition summaries of the posterior (DESIGN.md §8 "Several-partition summary"): L weighted partitions that
minimise the Wasserstein distance to the sample distribution with VI as ground metric (Balocchi & Wade's WASABI) — a Lloyd
iteration on partition space.  The distances (rc_partition_distances) and the update step (rc_vi_search_groups: every group's
exact minimum-expected-VI search in one launch) run on the GPU; what is here is exact integer bookkeeping between the calls.
There is no CPU fallback."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .pointestimate import (_sample_matrix, _labels, _sortlabels, _numerators, credibleball, expecteddistances)

_U53 = 1 << 53


def searchvigroups(samples, group, inits, orders, run_group, maxK: int = 0, maxsweeps: int = 100, device: int = 0):
    """Many exact expected-VI searches in one launch (rc_vi_search_groups): run r searches all partitions for the minimum
    expected VI over the samples s with group[s] == run_group[r], from the labels inits[r] (0 = unallocated) in the order
    orders[r] (a 1-based permutation) — bit for bit what searchpointestimate's exact search does on that sub-array.  samples:
    an MCMCResult, anything with `.clusts`, or an m×n label matrix; group: m ids in 0..G−1, −1 for a sample in no group.
    Returns (labels, info): labels[g] is the best labelling of group g (sortlabels'd; zeros where no run searches g); info
    has the per-run labels, loss, loss_num, sweeps, converged, moves, K, the per-group best (−1 = no run) and kernel_ms."""
    S = _sample_matrix(samples)
    res = _lib.vi_search_groups(S, group, inits, orders, run_group, maxK=maxK, maxsweeps=maxsweeps, device=device)
    out = np.zeros((len(res["best"]), S.shape[1]), np.int64)
    for g, b in enumerate(res["best"]):
        if b >= 0:
            out[g] = res["labels"][b]
    return out, res


@dataclass
class WasabiResult:
    """L weighted partitions summarising m samples.  particles (L×n, sortlabels'd) in order of descending weight, then of their
    index during the iteration; weights = group sizes / m; assignment[s]: the particle sample s belongs to; group_num[l]: Σ of
    the integer VI distances (units of 2^-32/n nats) from particle l to its samples; objective_num = Σ group_num = W;
    wasserstein = W/(2^32·n·m) nats, the only f64 value; trace: W after every assignment of the winning start; iterations,
    converged; start: the winning start's index (nstarts = the one from init); starts: every start's final W; kernel_ms: the
    search and distance kernels of the whole call."""
    particles: np.ndarray
    weights: np.ndarray
    assignment: np.ndarray
    group_num: list
    objective_num: int
    wasserstein: float
    trace: list
    iterations: int
    converged: bool
    start: int
    starts: list
    kernel_ms: float = 0.0
    _samples: np.ndarray = field(default=None, repr=False)
    _device: int = field(default=0, repr=False)

    def expectedvi(self) -> np.ndarray:
        """Each particle's posterior expected VI over ALL samples (nats), from one distance call."""
        return expecteddistances(self.particles, self._samples, "VI", device=self._device)[0]

    def credibleball(self, l: int, alpha: float = 0.05) -> dict:
        """credibleball (VI) of particle l within its own group of samples; `members` are the group's sample indices, which the
        ball's index lists refer to."""
        members = np.flatnonzero(self.assignment == l)
        out = credibleball(self.particles[l], self._samples[members], "VI", alpha, device=self._device)
        out["members"] = members
        return out


class _Device:
    """the two device calls of the driver, with their kernel time summed"""

    def __init__(self, S, cap, maxsweeps, device):
        self.S, self.cap, self.maxsweeps, self.device, self.ms = S, cap, maxsweeps, device, 0.0

    def distances(self, labellings):
        """P×m integer VI distances; their row sums over any subset of the samples must fit int64"""
        dist = _lib.partition_distances(np.atleast_2d(labellings), self.S, want_sq=False, want_phi=True, device=self.device)
        self.ms += dist["kernel_ms"]
        num = _numerators(dist, "VI")
        if int(num.max()) * num.shape[1] >= 2 ** 63:
            raise OverflowError("the sum of the VI distances over the samples does not fit 63 bits")
        return num

    def search(self, assign, inits, orders, run_group):
        res = _lib.vi_search_groups(self.S, assign, inits, orders, run_group, maxK=self.cap, maxsweeps=self.maxsweeps, device=self.device)
        self.ms += res["kernel_ms"]
        return res


def _assign(num):
    """every sample to the particle of least distance, ties to the lowest index: (assignment, the samples' distances, W)"""
    a = np.argmin(num, axis=0)
    d = num[a, np.arange(num.shape[1])]
    return a, d, int(d.sum())


def _farthest(d, used):
    """the unused sample of greatest positive distance, ties to the lowest index; −1 when there is none"""
    best = -1
    for s in range(len(d)):
        if s not in used and d[s] > 0 and (best < 0 or d[s] > d[best]):
            best = s
    return best


def _seed_particles(dev, S, L, u):
    """k-medoids++ on partition space from the L draws u of 53 bits: the sample (u[0]·m) >> 53, then samples drawn with
    probability proportional to their distance from the nearest particle so far"""
    m = len(S)
    chosen = [(int(u[0]) * m) >> 53]
    dmin = dev.distances(S[chosen[0]])[0]
    for j in range(1, L):
        W = int(dmin.sum())
        if W == 0:
            break
        thr = (int(u[j]) * W) >> 53
        idx = int(np.searchsorted(np.cumsum(dmin), thr, side="right"))       # the first inclusive prefix sum above thr
        chosen.append(idx)
        dmin = np.minimum(dmin, dev.distances(S[idx])[0])
    return [_sortlabels(S[i]) for i in chosen]


def _lloyd(dev, S, particles, orders, maxiter):
    """One start: the iteration from the given particles.  Returns a dict with particles, assignment, d (each sample's distance
    to its particle), W, trace, iterations, converged."""
    m, n = S.shape
    P = [np.asarray(p, np.int64) for p in particles]
    ident = np.arange(1, n + 1, dtype=np.int32)
    trace, prev, converged, it = [], None, False, 0
    assign, d, W = _assign(dev.distances(np.stack(P)))
    trace.append(W)
    while it < maxiter:
        it += 1
        repaired = False
        sizes = np.bincount(assign, minlength=len(P))
        if (sizes == 0).any():
            if W == 0:
                break
            used = set()
            for l in np.flatnonzero(sizes == 0):
                s = _farthest(d, used)
                if s < 0:
                    break
                used.add(s)
                P[l] = _sortlabels(S[s])
                repaired = True
            if repaired:
                assign, d, W = _assign(dev.distances(np.stack(P)))
                trace.append(W)
                sizes = np.bincount(assign, minlength=len(P))
        groups = [int(l) for l in np.flatnonzero(sizes)]
        inits, ords, run_group = [], [], []
        for l in groups:
            inits.append(P[l]); ords.append(ident); run_group.append(l)
            for o in orders:
                inits.append(np.zeros(n, np.int64)); ords.append(o); run_group.append(l)
        res = dev.search(assign.astype(np.int32), np.stack(inits), np.stack(ords), np.array(run_group, np.int32))
        changed = False
        for l in groups:
            new = res["labels"][res["best"][l]]
            if not np.array_equal(new, P[l]):
                P[l], changed = new.copy(), True
        if not changed and not repaired and prev is not None and np.array_equal(prev, assign):
            converged = True
            break
        prev = assign
        assign, d, W = _assign(dev.distances(np.stack(P)))
        trace.append(W)
    if W == 0:
        converged = True
    return dict(particles=P, assignment=assign, d=d, W=W, trace=trace, iterations=it, converged=converged)


def _check_arguments(L, nstarts, maxiter, nruns, maxK, maxsweeps, init):
    if int(L) < 1:
        raise ValueError("L must be at least 1")
    if int(nstarts) < 0 or (int(nstarts) == 0 and init is None):
        raise ValueError("no start: nstarts = 0 and no init")
    if int(maxiter) < 1 or int(maxsweeps) < 1:
        raise ValueError("maxiter and maxsweeps must be at least 1")
    if int(nruns) < 0 or int(maxK) < 0:
        raise ValueError("nruns and maxK must not be negative")


def wasabi(samples, L: int, *, nstarts: int = 4, maxiter: int = 50, nruns: int = 1, maxK: int = 0, maxsweeps: int = 100,
           seed: int = 0, init=None, device: int = 0) -> WasabiResult:
    """Summarise the samples (an MCMCResult, anything with `.clusts`, or an m×n label matrix) by L weighted partitions
    ("particles") that minimise W = Σ_s d(particle(s), s), d the VI in the exact searches' fixed point (partitiondistances'
    info["num"]: units of 2^-32/n nats) — the Wasserstein distance between the sample distribution and the weighted particles
    with VI as ground metric, times 2^32·n·m (Balocchi & Wade's WASABI).  Everything but WasabiResult.wasserstein is exact
    integer arithmetic, so the result is a pure function of (samples, L, the arguments, seed).

    Each start alternates (1) assigning every sample to its nearest particle, ties to the lowest particle index, and (2)
    replacing every particle by the partition of minimum expected VI over its own samples, searched over ALL partitions: one
    rc_vi_search_groups launch for all groups, per group one run from the current particle in identity order and nruns runs from
    empty labels, of which the first of least loss wins.  The current particle is a start and a run only accepts strictly
    improving moves, so no group's sum rises and W never increases.  A particle left without samples is replaced by the sample
    farthest from its own particle (ties: the lowest index; a sample serves one repair per iteration; only samples at positive
    distance serve) and the assignment is redone; with W = 0 the empty particles are dropped and the start ends.  A start ends
    converged when an iteration repeats the previous assignment and changes no particle, else after maxiter iterations (a last
    assignment then gives its W).  The start of least final W wins, ties to the first.

    One slot cap serves every group, so that a particle fits whichever samples it is given: maxK if positive, else the largest
    cluster count among the samples and the rows of init.

    Starts: nstarts seeded in the manner of k-medoids++ and, with init (L×n labels), one more from those
    particles.  Start t takes its L draws u = Generator(Philox(key=seed, counter=[0, 0, 0, t + 1])).integers(0, 2^53, size=L): the
    first particle is the sample (u[0]·m) >> 53; step j >= 1 draws a sample with probability proportional to its distance to the
    nearest particle so far — threshold (u[j]·W) >> 53, W the total, the first sample whose inclusive prefix sum exceeds it — and
    with W = 0 (fewer than L distinct partitions among the samples) the start has fewer particles.  The nruns orders are
    searchpointestimate's: Generator(Philox(key=seed)).permutation(n) in run order, the same for every group, iteration and start."""
    _check_arguments(L, nstarts, maxiter, nruns, maxK, maxsweeps, init)
    S = _sample_matrix(samples)
    m, n = S.shape
    L = int(L)
    given = None
    if init is not None:
        given = np.stack([_sortlabels(_labels(c)) for c in np.atleast_2d(np.asarray(init))])
        if given.shape[1] != n or not 1 <= given.shape[0] <= L:
            raise ValueError("init must hold between 1 and L labellings of n entries")
    cap = int(maxK) if maxK else max(len(np.unique(r)) for r in (S if given is None else np.concatenate([S, given])))
    dev = _Device(S, cap, int(maxsweeps), device)
    rng = np.random.Generator(np.random.Philox(key=int(seed)))
    orders = [rng.permutation(n).astype(np.int32) + 1 for _ in range(int(nruns))]
    runs = []
    for t in range(int(nstarts)):
        u = np.random.Generator(np.random.Philox(key=int(seed), counter=[0, 0, 0, t + 1])).integers(0, _U53, size=L)
        runs.append(_lloyd(dev, S, _seed_particles(dev, S, L, u), orders, int(maxiter)))
    if given is not None:
        runs.append(_lloyd(dev, S, list(given), orders, int(maxiter)))
    starts = [r["W"] for r in runs]
    win = min(range(len(starts)), key=lambda t: starts[t])               # the first of least W
    return _result(runs[win], S, win, starts, dev.ms, device)


def _result(r, S, win, starts, ms, device) -> WasabiResult:
    m, n = S.shape
    sizes = np.bincount(r["assignment"], minlength=len(r["particles"]))
    keep = sorted((l for l in range(len(sizes)) if sizes[l]), key=lambda l: (-int(sizes[l]), l))
    new = np.full(len(sizes), -1, np.int64)
    new[keep] = np.arange(len(keep))
    assign = new[r["assignment"]]
    group_num = [int(r["d"][assign == l].sum()) for l in range(len(keep))]
    return WasabiResult(particles=np.stack([r["particles"][l] for l in keep]), weights=sizes[keep] / float(m), assignment=assign,
                        group_num=group_num, objective_num=r["W"], wasserstein=r["W"] / (2.0 ** 32 * n * m), trace=list(r["trace"]),
                        iterations=r["iterations"], converged=bool(r["converged"]), start=win, starts=starts, kernel_ms=ms,
                        _samples=S, _device=device)


def wasabi_scan(samples, Ls, **kw):
    """wasabi for each L of Ls in ascending order: ({L: WasabiResult}, curve) with curve[i] the wasserstein of the i-th smallest
    L.  Every L after the first gets one more start (init): the previous result's particles plus the samples farthest from their
    own particle, enough to reach L, chosen by the repair rule — its first assignment is no worse than the previous result and W
    never rises, so the curve is non-increasing by construction.  Choosing L is the caller's: the curve flattens once the modes
    are covered (prior.detectknee finds an elbow of such a curve).  kw: wasabi's keyword arguments, without init."""
    if "init" in kw:
        raise ValueError("wasabi_scan sets init itself")
    Ls = sorted({int(L) for L in Ls})
    if not Ls or Ls[0] < 1:
        raise ValueError("Ls must hold positive integers")
    S = _sample_matrix(samples)
    out, prev = {}, None
    for L in Ls:
        init = None
        if prev is not None:
            rows = [p for p in prev.particles]
            d = _numerators(_lib.partition_distances(prev.particles, S, want_sq=False, want_phi=True, device=kw.get("device", 0)), "VI")
            d = d[prev.assignment, np.arange(len(S))]
            used = set()
            while len(rows) < L:
                s = _farthest(d, used)
                if s < 0:
                    break
                used.add(s)
                rows.append(_sortlabels(S[s]))
            init = np.stack(rows)
        out[L] = prev = wasabi(S, L, init=init, **kw)
    return out, np.array([out[L].wasserstein for L in Ls])
