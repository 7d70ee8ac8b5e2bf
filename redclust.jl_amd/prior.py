"""fitprior (src/prior.jl:22-128), its elbow rule detectknee (src/prior.jl:340-360), sample_rp (src/mcmc.jl:592-636) and
Clustering.jl's kmedoids, which fitprior and runsampler's default start (src/mcmc.jl:516-527) call.

The k-medoids runs — one per k of the elbow scan, then the notional clustering — are batched on the device
(rc_kmedoids_scan / rc_kmedoids, csrc/kmedoids.inc.hip); the within / between split of the distances under the notional
clustering comes from the device's block sums (rc_within_between).  On the host, as in the reference: the elbow, the
scalar chain of sample_rp and the maximum-likelihood fits.  The k-means path of fitprior is not in this build."""
from __future__ import annotations

import math
import warnings

import numpy as np
from scipy.special import digamma, polygamma

from ._lib import Context
from .datagen import _gamma_shape_mle
from .sampler import sample_p, sample_r
from .types import KmedoidsResult, MCMCData, MCMCOptionsList, PriorHyperparamsList

# Seeds of the k-medoids streams the reference draws from its one global RNG: the elbow scan uses `seed` itself, the
# notional clustering and runsampler's starting labels fresh streams derived from it (kmedoids_stream_seed).
KMED_STREAM_SCAN, KMED_STREAM_NOTIONAL, KMED_STREAM_INIT = 0, 1, 2


def kmedoids_stream_seed(seed: int, stream: int) -> int:
    return (int(seed) + int(stream) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def kmedoids(D_or_ctx, k: int, *, maxiter: int = 200, tol: float = 1e-8, seed: int = 0, device: int = 0) -> KmedoidsResult:
    """kmedoids(D, k; maxiter, tol) of Clustering.jl (k-medoids++ seeding by costs) on the device.  D_or_ctx: an n×n
    dissimilarity matrix or a Context (its staged matrix is used; its chain state is left as it is)."""
    if isinstance(D_or_ctx, Context):
        return D_or_ctx.kmedoids(k, maxiter=maxiter, tol=tol, seed=seed)
    ctx = Context(D_or_ctx, device=device)
    try:
        return ctx.kmedoids(k, maxiter=maxiter, tol=tol, seed=seed)
    finally:
        ctx.close()


def detectknee(xvalues, yvalues):
    """src/prior.jl:340-360: the point farthest from the line through the two extreme points (first one on ties)."""
    x0 = np.asarray(xvalues, dtype=np.float64)
    ind = np.argsort(x0, kind="stable")
    x, y = x0[ind], np.asarray(yvalues, dtype=np.float64)[ind]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (y[-1] - y[0]) / (x[-1] - x[0])
        b = y[0] - a * x[0]
        distances = np.abs(a * x + b - y) / math.sqrt(a * a + 1) if np.isfinite(a) else np.full(len(x), np.nan)
    m = int(np.argmax(distances))
    xs = np.asarray(xvalues)[ind]
    return xs[m].item(), float(y[m])


def _beta_mle(x, maxiter: int = 1000, tol: float = 1e-14):
    """fit_mle(Beta, x): Newton's method on ψ(u) - ψ(u+v) = mean log x, ψ(v) - ψ(u+v) = mean log(1-x), started from the
    method of moments.  Returns (u, v)."""
    x = np.asarray(x, dtype=np.float64)
    g1, g2 = float(np.mean(np.log(x))), float(np.mean(np.log1p(-x)))
    m, s2 = float(np.mean(x)), float(np.var(x))
    c = m * (1 - m) / s2 - 1 if s2 > 0 else 1.0
    th = np.array([m * c, (1 - m) * c]) if c > 0 else np.array([1.0, 1.0])
    for _ in range(maxiter):
        t = th[0] + th[1]
        grad = np.array([g1 - digamma(th[0]) + digamma(t), g2 - digamma(th[1]) + digamma(t)])
        tt = polygamma(1, t)
        H = np.array([[tt - polygamma(1, th[0]), tt], [tt, tt - polygamma(1, th[1])]])
        step = np.linalg.solve(H, grad)
        new = th - step
        new = np.where(new > 0, new, th / 2)   # stay in the domain
        done = np.max(np.abs(new - th)) < tol * np.max(np.abs(th))
        th = new
        if done:
            break
    return float(th[0]), float(th[1])


def _gamma_mle(x):
    """fit_mle(Gamma, x) as (shape, rate)."""
    x = np.asarray(x, dtype=np.float64)
    mean = float(np.mean(x))
    shape = _gamma_shape_mle(mean, float(np.mean(np.log(x))))
    return shape, shape / mean


def sample_rp(clustsizes, options: MCMCOptionsList | None = None, params: PriorHyperparamsList | None = None, *,
              verbose: bool = True, rng=None, seed: int = 0):
    """src/mcmc.jl:592-636: the r / p chain of the sampler for fixed cluster sizes.  As written, the starting r is drawn
    from Gamma(η, σ) with σ as the SCALE (the sampler's prior uses it as a rate).  Returns dict(r=..., p=...)."""
    options = options or MCMCOptionsList()
    params = params or PriorHyperparamsList()
    rng = rng if rng is not None else np.random.default_rng(seed)
    cs = np.asarray(clustsizes, dtype=np.int64)
    C = cs[cs > 0]
    n, K = int(C.sum()), len(C)
    eta, sigma, proposalsd_r, u, v = params.eta, params.sigma, params.proposalsd_r, params.u, params.v
    r = float(rng.gamma(eta, sigma))
    p = float(rng.beta(u, v))
    numiters, burnin, thin = options.numiters, options.burnin, options.thin
    numsamples = options.numsamples
    out = dict(r=np.zeros(numsamples), p=np.zeros(numsamples))
    j = 0
    for i in range(1, numiters + 1):
        r, _ = sample_r(rng, r, p, C, K, eta, sigma, proposalsd_r)
        p = sample_p(rng, K, n, r, u, v)
        if i > burnin and (i - burnin) % thin == 0:
            out["r"][j], out["p"][j] = r, p
            j += 1
    return out


def _staging(data, diss):
    """(n, kind, payload) of fitprior's input; kind 'D' or 'points'."""
    if isinstance(data, MCMCData):
        return (data.n, "points", data.points) if data.points is not None else (data.n, "D", data.D)
    if isinstance(data, (list, tuple)):
        if diss:
            raise ValueError("diss = true but data is not a dissimilarity matrix. Assuming that the data is a vector of observations.")
        x = np.asarray(data, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("data must be a vector of equal-length observations")
        return x.shape[0], "points", x
    x = np.asarray(data, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("data must be a matrix: one observation per row, or a square dissimilarity matrix with diss = True")
    if diss:
        if x.shape[0] != x.shape[1]:
            raise ValueError("Supplied dissimilarity matrix is not square.")
        return x.shape[0], "D", x
    return x.shape[0], "points", x


def fitprior(data, algo: str, diss: bool = False, *, Kmin: int = 1, Kmax: int | None = None, verbose: bool = True,
             seed: int = 0, device: int = 0, ctx: Context | None = None) -> PriorHyperparamsList:
    """fitprior(data, algo, diss; Kmin, Kmax, verbose) — src/prior.jl:22-128, algo = "k-medoids".

    data: points (one observation per row, this package's convention: the reference's columns), a dissimilarity matrix
    with diss=True, or an MCMCData.  ctx reuses a Context that holds the same matrix (its label state is overwritten
    with the notional clustering); otherwise one is staged for the call — from points the device computes the distances.
    seed keys the k-medoids streams (kmedoids_stream_seed) and the sample_rp chain."""
    out = print if verbose else (lambda *a, **k: None)
    out("Fitting prior hyperparameters")
    is_data = isinstance(data, MCMCData)
    N, kind, x = _staging(data, diss)
    if is_data or kind == "D":
        out(f"Input: pairwise dissimilarities between {N} observations.")
    else:
        out(f"Input: {N} observations of dimension {x.shape[1]}.")
    if Kmax is None:
        Kmax = N // 2
    if algo == "k-means" and kind == "D":
        raise ValueError("Cannot use algorithm `k-means` with a dissimilarity matrix.")
    if algo not in ("k-means", "k-medoids"):
        raise ValueError("Algo must be 'k-means' or 'k-medoids'.")
    if not (1 <= Kmin <= Kmax <= N):
        raise ValueError("Kmin and Kmax must satisfy 1 ≤ Kmin ≤ Kmax ≤ N")
    if algo == "k-means":
        raise NotImplementedError("fitprior(algo='k-means') is not in this build: use algo='k-medoids'")
    if ctx is not None and ctx.n != N:
        raise ValueError(f"ctx holds {ctx.n} observations, data {N}")
    own = ctx is None
    if own:
        ctx = Context.from_points(x, device=device) if kind == "points" else Context(x, device=device)
    try:
        out("Computing notional clustering.")
        # as written (prior.jl:63-70): the runs are for k = 1:(Kmax-Kmin+1), their costs are labelled Kmin:Kmax
        scan = ctx.kmedoids_scan(1, Kmax - Kmin + 1, maxiter=1000, seed=kmedoids_stream_seed(seed, KMED_STREAM_SCAN))
        for k in np.flatnonzero(~scan["converged"]) + 1:
            warnings.warn(f"Clustering did not converge at K = {k}")
        K = int(detectknee(np.arange(Kmin, Kmax + 1), scan["totalcost"])[0])
        notional = ctx.kmedoids(K, maxiter=1000, seed=kmedoids_stream_seed(seed, KMED_STREAM_NOTIONAL)).assignments
        ctx.set_state(notional)
        wb = ctx.within_between()

        out("Computing partition prior hyperparameters.")
        clustsizes = np.bincount(notional)[1:]
        temp = sample_rp(clustsizes, verbose=verbose, seed=seed)
        proposalsd_r = float(np.std(temp["r"], ddof=1))
        eta, sigma = _gamma_mle(temp["r"])
        u, v = _beta_mle(temp["p"])

        out("Computing likelihood hyperparameters.")
        if K == N:   # A is empty
            warnings.warn("Got a notional clustering of entirely singletons. Falling back to defaults for cohesion parameters.")
            delta1, alpha, beta = 1.0, 1.0, 1.0
        else:
            cA = wb["count_within"]
            delta1 = _gamma_shape_mle(wb["sum_within"] / cA, wb["sumlog_within"] / cA)
            alpha, beta = cA * delta1, wb["sum_within"]
        if K == 1:
            warnings.warn("Got a notional clustering with a single cluster. Falling back to defaults for repulsion parameters.")
            delta2, zeta, gamma = 1.0, 1.0, 1.0
        else:
            cB = wb["count_between"]
            delta2 = _gamma_shape_mle(wb["sum_between"] / cB, wb["sumlog_between"] / cB)
            zeta, gamma = cB * delta2, wb["sum_between"]
        return PriorHyperparamsList(delta1=delta1, delta2=delta2, alpha=alpha, beta=beta, zeta=zeta, gamma=gamma, eta=eta,
                                    sigma=sigma, proposalsd_r=proposalsd_r, u=u, v=v, K_initial=K)
    finally:
        if own:
            ctx.close()
