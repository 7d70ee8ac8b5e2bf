"""Scoring labellings under the model on the GPU (csrc/score.inc.hip through rc_score_labellings; include/redclust_hip.h has
the contract, DESIGN.md §8 "Scoring labellings" the design): the log-likelihood, log-prior and log-posterior of any batch of
labellings — chain samples, point estimates, dendrogram cuts, another sampler's draws — against a context's matrices, without
touching its state.  The block sums of a labelling are its sufficient statistics: once they are on the host its log-likelihood
under any hyperparameters is host arithmetic (loglik_from_blocks), which is what reweight builds on.  There is no CPU fallback
for the device pass."""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from ._lib import Context
from .types import MCMCData


def _params_dict(params) -> dict:
    return params.as_dict() if hasattr(params, "as_dict") else dict(params)


def _labellings(x) -> np.ndarray:
    """an MCMCResult (its clusts), a label matrix, one labelling or a list of vectors as an L×n int64 matrix"""
    clusts = x.clusts if hasattr(x, "clusts") else x
    if len(clusts) == 0:
        raise ValueError("no labellings")
    S = np.asarray(clusts if isinstance(clusts, np.ndarray) else np.stack([np.asarray(c) for c in clusts]))
    if S.ndim == 1:
        S = S[None, :]
    if S.ndim != 2 or not np.issubdtype(S.dtype, np.integer):
        raise ValueError("labellings must be an L×n matrix of integer labels")
    return np.ascontiguousarray(S, dtype=np.int64)


def _context(data_or_ctx, device):
    """(context, whether it is ours to close) for a Context, an MCMCData or a dissimilarity matrix"""
    if isinstance(data_or_ctx, Context):
        return data_or_ctx, False
    if isinstance(data_or_ctx, MCMCData):
        d = data_or_ctx
        return (Context.from_points(d.points, device=device, metric=d.metric) if d.points is not None else Context(d.D, device=device)), True
    return Context(np.asarray(data_or_ctx, dtype=np.float64), device=device), True


def _per_labelling(x, L, what):
    if x is None:
        return None
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.shape not in ((1,), (L,)):
        raise ValueError(f"{what} must be a scalar or hold one value per labelling ({L})")
    return np.ascontiguousarray(np.broadcast_to(x, (L,)))


def scorelabellings(data_or_ctx, labellings, params=None, r=None, p=None, *, want_blocks: bool = False, device: int = 0) -> dict:
    """Log-likelihood, log-prior and log-posterior of every labelling under the model.

    data_or_ctx: a Context (used as it is: its state, layout and counts are untouched), an MCMCData or a dissimilarity matrix
    (a context is made for the call).  labellings: an MCMCResult — its r and p are then the default, and its params when
    none are given and the context is not the caller's — an L×n label matrix, one labelling or a list of vectors.  params: a
    PriorHyperparamsList or a dict (None with a Context: the context's).  r, p: scalars or one per labelling; without them
    only the log-likelihood is returned.  The dict of Context.score."""
    S = _labellings(labellings)
    if r is None and p is None and hasattr(labellings, "clusts"):
        r, p = getattr(labellings, "r", None), getattr(labellings, "p", None)
    ctx, own = _context(data_or_ctx, device)
    try:
        if params is None and own:
            params = getattr(labellings, "params", None)
            if params is None:
                raise ValueError("params are needed with data that is not a Context")
        return ctx.score(S, _per_labelling(r, len(S), "r"), _per_labelling(p, len(S), "p"),
                         None if params is None else _params_dict(params), want_blocks=want_blocks)
    finally:
        if own:
            ctx.close()


def loglik_from_blocks(blocks, sizes, n: int, eD: int, eL: int, params) -> float:
    """The log-likelihood of one labelling from its block sums (host only): blocks and sizes as one entry of
    scorelabellings(..., want_blocks=True)["blocks"] / ["sizes"], eD and eL from the same dict, params any hyperparameters."""
    return _lib.loglik_from_blocks(blocks, sizes, n, eD, eL, _params_dict(params))


def logprior(sizes, n: int, r: float, p: float, params) -> float:
    """logprior (src/mcmc.jl:58-78) of a labelling with the given cluster sizes, on the host in double precision."""
    P = _params_dict(params)
    eta, sigma, u, v = (float(P.get(k, 1.0)) for k in ("eta", "sigma", "u", "v"))
    sz = np.asarray(sizes, dtype=np.int64)
    sz = sz[sz > 0]
    K = len(sz)
    lgam = eta * math.log(sigma) - math.lgamma(eta) + (eta - 1) * math.log(r) - sigma * r
    lbet = math.lgamma(u + v) - math.lgamma(u) - math.lgamma(v) + (u - 1) * math.log(p) + (v - 1) * math.log(1 - p)
    L = math.lgamma(K + 1) + (n - K) * math.log(p) + (r * K) * math.log(1 - p) - K * math.lgamma(r) + lgam + lbet
    for s in sz:
        L += math.log(float(s)) + math.lgamma(float(s) + r - 1)
    return L


def mapestimate(data_or_ctx, candidates, params=None, r=None, p=None, *, scores: dict | None = None, device: int = 0):
    """The candidate of highest log-posterior, the smallest index on ties.  candidates: as scorelabellings' labellings; r, p:
    scalars or one per candidate (an MCMCResult brings its own).  scores: a dict scorelabellings returned for the same
    candidates — nothing is computed then and data_or_ctx is not looked at.  Returns (clust, info): the candidate and a dict
    with index (0-based), loglik, logprior, logposterior, K (all candidates) and kernel_ms."""
    S = _labellings(candidates)
    sc = scores if scores is not None else scorelabellings(data_or_ctx, candidates, params, r, p, device=device)
    lpost = sc.get("logposterior")
    if lpost is None:
        raise ValueError("the log-posterior needs r and p")
    lpost = np.asarray(lpost, dtype=np.float64)
    if lpost.shape != (len(S),):
        raise ValueError("the scores are not of these candidates")
    best = int(np.argmax(lpost))            # numpy's argmax is the first maximum
    info = dict(index=best, loglik=sc["loglik"], logprior=sc["logprior"], logposterior=lpost, K=sc.get("K"),
                kernel_ms=sc.get("kernel_ms", 0.0))
    return S[best].copy(), info


def searchmapestimate(data_or_ctx, candidates=None, params=None, r=None, p=None, *, nruns: int = 16, maxK: int = 0, maxsweeps: int = 100,
                      seed: int = 0, init=None, scores: dict | None = None, device: int = 0):
    """Search ALL partitions for the clustering of maximum log-posterior (csrc/mapsearch.inc.hip through rc_map_search; DESIGN.md
    §8 "MAP search"): a one-point-at-a-time climb of loglik + logprior from the best candidates, where mapestimate only picks
    among them.  Runs on the GPU, every run one workgroup; there is no CPU fallback.

    data_or_ctx, candidates, params, r, p, scores: as mapestimate's (an MCMCResult brings its r and p, and its params for data
    that is not a Context).  The candidates are scored and the climb starts from the nruns distinct ones of highest
    log-posterior, each under its own r and p; every row of init (labels 0..n, 0 = unallocated) is a start too, and so is the
    empty labelling — a sequential allocation — these under the best candidate's r and p.  candidates=None: r and p must be
    given (scalars) and the starts are init and the empty labelling.  Every run visits the points in a permutation of its own,
    drawn from seed in run order as _search_starts draws them (Philox, key = seed).  maxK: the cap on the number of
    clusters (0: min(n, 1024)); a start with more clusters than the cap is an error; maxsweeps bounds the sweeps.

    Returns (clust, info) shaped like mapestimate's: info has index (of the best candidate, None without candidates),
    start_logposterior and logposterior (per run; the first is NaN for a start with unallocated points), loglik, logprior,
    sweeps, converged, moves, K, capped, labels (per run), runs (the starts as rows of labels), best (the run returned, or −1
    when no run beat the best candidate, which is then returned as mapestimate would), candidate_logposterior and kernel_ms.
    The result is never worse than mapestimate's on the same candidates."""
    ctx, own = _context(data_or_ctx, device)
    try:
        if params is None and own:
            params = getattr(candidates, "params", None)
            if params is None:
                raise ValueError("params are needed with data that is not a Context")
        P = None if params is None else _params_dict(params)
        n = ctx.n
        starts, rs, ps = [], [], []
        cand_best, cand_lp, S = None, None, None
        if candidates is not None:
            S = _labellings(candidates)
            if S.shape[1] != n:
                raise ValueError("the candidates must have the data's n columns")
            if r is None and p is None and hasattr(candidates, "clusts"):
                r, p = getattr(candidates, "r", None), getattr(candidates, "p", None)
            if r is None or p is None:
                raise ValueError("the log-posterior needs r and p")
            rc_, pc_ = _per_labelling(r, len(S), "r"), _per_labelling(p, len(S), "p")
            sc = scores if scores is not None else ctx.score(S, rc_, pc_, P)
            cand_lp = np.asarray(sc["logposterior"], dtype=np.float64)
            if cand_lp.shape != (len(S),):
                raise ValueError("the scores are not of these candidates")
            cand_best = int(np.argmax(cand_lp))
            seen = set()
            for c in np.argsort(-cand_lp, kind="stable"):               # the highest first, the smaller index on ties
                key = _lib_sortlabels(S[c]).tobytes()
                if key in seen:
                    continue
                seen.add(key)
                if len(starts) == int(nruns):
                    break
                starts.append(S[c]); rs.append(rc_[c]); ps.append(pc_[c])
            r0, p0 = float(rc_[cand_best]), float(pc_[cand_best])
        else:
            if r is None or p is None:
                raise ValueError("without candidates r and p must be given")
            r0, p0 = float(np.asarray(r).reshape(-1)[0]), float(np.asarray(p).reshape(-1)[0])
        for lab in ([] if init is None else np.atleast_2d(np.asarray(init))):
            if len(lab) != n:
                raise ValueError("every labelling in init must have n entries")
            starts.append(np.asarray(lab, np.int64)); rs.append(r0); ps.append(p0)
        starts.append(np.zeros(n, np.int64)); rs.append(r0); ps.append(p0)
        rng = np.random.Generator(np.random.Philox(key=int(seed)))
        orders = [rng.permutation(n).astype(np.int32) + 1 for _ in range(len(starts))]
        runs = np.stack(starts)
        need = max(len(np.unique(x[x > 0])) for x in runs)
        if maxK and need > maxK:
            raise ValueError(f"a start has {need} clusters, more than maxK = {maxK}")
        res = ctx.map_search(runs, np.stack(orders), np.asarray(rs), np.asarray(ps), P, maxK=maxK, maxsweeps=maxsweeps)
        best = res["best"]
        info = {k: res[k] for k in ("start_logposterior", "logposterior", "loglik", "logprior", "sweeps", "converged", "moves", "K",
                                    "capped", "labels", "kernel_ms")}
        info.update(runs=runs, index=cand_best, candidate_logposterior=cand_lp, best=best)
        if cand_lp is not None and not res["logposterior"][best] > cand_lp[cand_best]:
            info["best"] = -1                                           # no run beat the best candidate: mapestimate's answer
            return S[cand_best].copy(), info
        return res["labels"][best].copy(), info
    finally:
        if own:
            ctx.close()


def _lib_sortlabels(z) -> np.ndarray:
    """labels renamed 1..K by first appearance: equal for equal partitions"""
    _, first, inv = np.unique(z, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(1, len(first) + 1)
    return rank[inv.reshape(-1)]


def reweight(data_or_ctx, result, new_params, *, scores: dict | None = None, device: int = 0):
    """Prior-sensitivity analysis without running the chain again: importance weights of the samples of an MCMCResult under
    other hyperparameters.  One device pass gives every sample's block sums (scores: that pass's dict, if the caller has it —
    scorelabellings(..., want_blocks=True) — and no device is touched); the log-posterior under result.params and under
    new_params is host arithmetic from there.  new_params: a PriorHyperparamsList or dict, or a list of them.  Returns a dict
    (a list of dicts for a list): weights (normalised, Σ = 1), logweights (their logarithm), ess = (Σw)²/Σw², and
    logposterior_new, logposterior_old."""
    S = _labellings(result)
    m, n = S.shape
    r = np.asarray(result.r, dtype=np.float64).reshape(-1)
    p = np.asarray(result.p, dtype=np.float64).reshape(-1)
    if r.shape != (m,) or p.shape != (m,):
        raise ValueError("the result must hold one r and p per sample")
    sc = scores if scores is not None else scorelabellings(data_or_ctx, result, result.params, r, p, want_blocks=True, device=device)
    if sc.get("blocks") is None:
        raise ValueError("reweight needs the block sums (want_blocks=True)")

    def logpost(P):
        return np.array([loglik_from_blocks(sc["blocks"][s], sc["sizes"][s], n, sc["eD"], sc["eL"], P) +
                         logprior(sc["sizes"][s], n, r[s], p[s], P) for s in range(m)])

    old = logpost(result.params)
    many = isinstance(new_params, (list, tuple))
    outs = []
    for P in (new_params if many else [new_params]):
        new = logpost(P)
        lw = new - old
        w = np.exp(lw - lw.max())
        tot = float(w.sum())
        outs.append(dict(weights=w / tot, logweights=lw - lw.max() - math.log(tot), ess=tot * tot / float((w * w).sum()),
                         logposterior_new=new, logposterior_old=old))
    return outs if many else outs[0]
