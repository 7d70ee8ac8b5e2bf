"""fitprior (src/prior.jl:22-128), fitprior2 (:151-277), sampledist (:284-308), sampleK (:316-338), pmf (:362-367), the
elbow rule detectknee (:340-360), sample_rp (src/mcmc.jl:592-636) and Clustering.jl's kmedoids, which fitprior, fitprior2
and runsampler's default start (src/mcmc.jl:516-527) call.

The k-medoids runs — one per k of the elbow scan, then the notional clustering — are batched on the device
(rc_kmedoids_scan / rc_kmedoids, csrc/kmedoids.inc.hip); the within / between split of the distances under the notional
clustering comes from the device's block sums (rc_within_between), fitprior2's split under every k of the scan from the
scan itself (rc_kmedoids_scan_split).  sampleK's Gumbel-max draws run on the device (rc_sample_k, csrc/samplek.inc.hip).
On the host, as in the reference: the elbow, the scalar chain of sample_rp, the draws of r / p and the maximum-likelihood
fits.

The k-means path (Clustering.jl's kmeans on the observations, csrc/kmeans.inc.hip: rc_kmeans / rc_kmeans_scan[_split]) is
reached through fitprior_kmeans / fitprior2_kmeans, which share one body with the k-medoids fits; the string "k-means"
given to fitprior / fitprior2 still raises NotImplementedError."""
from __future__ import annotations

import math
import warnings

import numpy as np
from scipy.special import digamma, polygamma

from ._lib import Context, sample_k
from .datagen import _gamma_shape_mle
from .sampler import sample_p, sample_r
from .types import KmeansResult, KmedoidsResult, MCMCData, MCMCOptionsList, PriorHyperparamsList

# Seeds of the k-medoids streams the reference draws from its one global RNG: the elbow scan uses `seed` itself, the
# notional clustering and runsampler's starting labels fresh streams derived from it (kmedoids_stream_seed).
KMED_STREAM_SCAN, KMED_STREAM_NOTIONAL, KMED_STREAM_INIT = 0, 1, 2
# fitprior2's sampleK call (host r / p draws and the device's Gumbel noise) draws from a stream of its own as well
SAMPLEK_STREAM = 3


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


def kmeans(points_or_ctx, k: int, *, maxiter: int = 100, tol: float = 1e-6, seed: int = 0, init=None,
           device: int = 0) -> KmeansResult:
    """kmeans(X, k; maxiter, tol, init) of Clustering.jl (k-means++ seeding, or init: k distinct 1-based point indices) on
    the device.  points_or_ctx: n×dim observations (one per row) or a Context made by Context.from_points (its chain state
    is left as it is)."""
    if isinstance(points_or_ctx, Context):
        return points_or_ctx.kmeans(k, maxiter=maxiter, tol=tol, seed=seed, init=init)
    ctx = Context.from_points(points_or_ctx, device=device)
    try:
        return ctx.kmeans(k, maxiter=maxiter, tol=tol, seed=seed, init=init)
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


def _prepare(name, data, algo, diss, Kmin, Kmax, ctx, out, kmeans_built=False):
    """The input handling and checks fitprior and fitprior2 share (src/prior.jl:30-56, :160-188): (N, kind, payload, Kmax)."""
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
    if algo == "k-means" and not kmeans_built:
        raise NotImplementedError(f"{name}(algo='k-means') is not in this build: use algo='k-medoids'")
    if ctx is not None and ctx.n != N:
        raise ValueError(f"ctx holds {ctx.n} observations, data {N}")
    if algo == "k-means" and ctx is not None and not getattr(ctx, "dim", 0):
        raise ValueError("Cannot use algorithm `k-means` with a dissimilarity matrix.")   # a Context made from a matrix
    return N, kind, x, Kmax


def _clusterer(ctx, algo):
    """(scan, single run) of the backend: both take (…, maxiter=, seed=), the scan also split=."""
    return (ctx.kmeans_scan, ctx.kmeans) if algo == "k-means" else (ctx.kmedoids_scan, ctx.kmedoids)


def _stage(kind, x, device, data=None):
    """the context of the staged input; an MCMCData with points brings its metric"""
    metric = data.metric if isinstance(data, MCMCData) else None
    return Context.from_points(x, device=device, metric=metric) if kind == "points" else Context(x, device=device)


def _partition_prior(notional, verbose, seed):
    """src/prior.jl:88-94 (and :229-235): sample_rp on the notional clustering's sizes, then the Gamma fit of r and the Beta
    fit of p.  Returns (proposalsd_r, eta, sigma, u, v)."""
    temp = sample_rp(np.bincount(notional)[1:], verbose=verbose, seed=seed)
    proposalsd_r = float(np.std(temp["r"], ddof=1))
    eta, sigma = _gamma_mle(temp["r"])
    u, v = _beta_mle(temp["p"])
    return proposalsd_r, eta, sigma, u, v


def fitprior(data, algo: str, diss: bool = False, *, Kmin: int = 1, Kmax: int | None = None, verbose: bool = True,
             seed: int = 0, device: int = 0, ctx: Context | None = None) -> PriorHyperparamsList:
    """fitprior(data, algo, diss; Kmin, Kmax, verbose) — src/prior.jl:22-128, algo = "k-medoids".

    data: points (one observation per row, this package's convention: the reference's columns), a dissimilarity matrix
    with diss=True, or an MCMCData.  ctx reuses a Context that holds the same matrix (its label state is overwritten
    with the notional clustering); otherwise one is staged for the call — from points the device computes the distances.
    seed keys the k-medoids streams (kmedoids_stream_seed) and the sample_rp chain.
    algo = "k-means" raises NotImplementedError: that path is fitprior_kmeans."""
    return _fitprior(data, algo, diss, Kmin, Kmax, verbose, seed, device, ctx, False)


def fitprior_kmeans(data, *, Kmin: int = 1, Kmax: int | None = None, verbose: bool = True, seed: int = 0, device: int = 0,
                    ctx: Context | None = None) -> PriorHyperparamsList:
    """What the reference's fitprior(data, "k-means"; Kmin, Kmax, verbose) computes (src/prior.jl:22-128 with
    kmeans(x, k; maxiter = 1000) at :64 and :72): the elbow scan and the notional clustering by k-means on the observations
    (rc_kmeans_scan / rc_kmeans), the distance split and every fit as in fitprior.

    data: points (one observation per row) or an MCMCData built from points; dissimilarities alone are the reference's
    ValueError.  ctx: a Context made by Context.from_points from the same points (its label state is overwritten with the
    notional clustering).  Seeds and streams as in fitprior.  fitprior(data, "k-means") itself still raises
    NotImplementedError because the suite pins that; routing the string here is a one-line follow-up (kmeans_built=True in
    fitprior's call of the shared body) once those two assertions may change."""
    return _fitprior(data, "k-means", False, Kmin, Kmax, verbose, seed, device, ctx, True)


def _fitprior(data, algo, diss, Kmin, Kmax, verbose, seed, device, ctx, kmeans_built):
    """The body fitprior (k-medoids) and fitprior_kmeans share."""
    out = print if verbose else (lambda *a, **k: None)
    N, kind, x, Kmax = _prepare("fitprior", data, algo, diss, Kmin, Kmax, ctx, out, kmeans_built)
    own = ctx is None
    if own:
        ctx = _stage(kind, x, device, data)
    try:
        out("Computing notional clustering.")
        scan_fn, run_fn = _clusterer(ctx, algo)
        # as written (prior.jl:63-70): the runs are for k = 1:(Kmax-Kmin+1), their costs are labelled Kmin:Kmax
        scan = scan_fn(1, Kmax - Kmin + 1, maxiter=1000, seed=kmedoids_stream_seed(seed, KMED_STREAM_SCAN))
        for k in np.flatnonzero(~scan["converged"]) + 1:
            warnings.warn(f"Clustering did not converge at K = {k}")
        K = int(detectknee(np.arange(Kmin, Kmax + 1), scan["totalcost"])[0])
        notional = run_fn(K, maxiter=1000, seed=kmedoids_stream_seed(seed, KMED_STREAM_NOTIONAL)).assignments
        ctx.set_state(notional)
        wb = ctx.within_between()

        out("Computing partition prior hyperparameters.")
        proposalsd_r, eta, sigma, u, v = _partition_prior(notional, verbose, seed)

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


def pmf(X, N: int | None = None):
    """src/prior.jl:362-367: p[k-1] = #{X == k} / length(X) for k = 1..max X; with N, padded with zeros to length N as
    fitprior2 does."""
    X = np.asarray(X, dtype=np.int64)
    if X.size == 0 or X.min() < 1:
        raise ValueError("pmf needs a non-empty vector of positive integers")
    p = np.bincount(X)[1:] / len(X)
    if N is not None and len(p) < N:
        p = np.concatenate([p, np.zeros(N - len(p))])
    return p


def sampleK(*args, seed: int = 0, device: int = 0):
    """sampleK(params, numsamples, n) or sampleK(η, σ, u, v, numsamples, n) — src/prior.jl:316-338: numsamples draws of K
    from its prior predictive for n observations, as int64 in 1..n.  r ~ Gamma(η, 1/σ) then p ~ Beta(u, v) come from
    np.random.default_rng(seed); the Gumbel-max draw over K = 1..n runs on the device (rc_sample_k, uniforms keyed by seed)."""
    if len(args) == 3:
        params, numsamples, n = args
        eta, sigma, u, v = params.eta, params.sigma, params.u, params.v
    elif len(args) == 6:
        eta, sigma, u, v, numsamples, n = args
    else:
        raise TypeError("sampleK(params, numsamples, n) or sampleK(eta, sigma, u, v, numsamples, n)")
    if n < 1:
        raise ValueError("n must be a positive integer.")
    if numsamples < 1:
        raise ValueError("numsamples must be a positive integer.")
    rng = np.random.default_rng(seed)
    r = rng.gamma(eta, 1.0 / sigma, int(numsamples))
    p = rng.beta(u, v, int(numsamples))
    return sample_k(int(n), r, p, seed=seed, device=device)[0]


def sampledist(params: PriorHyperparamsList, type: str, numsamples: int = 1, *, seed: int = 0):
    """src/prior.jl:284-308: numsamples draws from the prior predictive of the within-cluster ("intracluster": α, β, δ1) or
    between-cluster ("intercluster": ζ, γ, δ2) distances: λ ~ Gamma(a, 1/b), then x ~ Gamma(δ, 1/λ).  Host NumPy."""
    if type not in ("intercluster", "intracluster"):
        raise ValueError('type must be either "intercluster" or "intracluster".')
    if numsamples < 1:
        raise ValueError("numsamples must be a positive integer.")
    a, b, d = (params.alpha, params.beta, params.delta1) if type == "intracluster" else (params.zeta, params.gamma, params.delta2)
    rng = np.random.default_rng(seed)
    lam = rng.gamma(a, 1.0 / b, int(numsamples))
    return rng.gamma(d, 1.0 / lam)


def _fit_weighted(stats, Kprior, Kmin: int, Kmax: int):
    """fitprior2's likelihood fits (src/prior.jl:238-266) from the per-k sufficient statistics: stats holds count_, sum_ and
    sumlog_ within / between arrays indexed by k - Kmin for k = Kmin..Kmax, Kprior[k - 1] the weight of k.  fit_mle(Gamma, x,
    w) is the unweighted fit of the weighted statistics; the sums run over k in ascending order.  Returns (δ1, α, β, δ2, ζ, γ)."""
    w = np.asarray(Kprior, dtype=np.float64)[Kmin - 1:Kmax]
    res = []
    for side, what in (("within", "cohesion"), ("between", "repulsion")):
        c = np.asarray(stats["count_" + side], dtype=np.int64)[:Kmax - Kmin + 1]
        S = np.asarray(stats["sum_" + side], dtype=np.float64)[:Kmax - Kmin + 1]
        L = np.asarray(stats["sumlog_" + side], dtype=np.float64)[:Kmax - Kmin + 1]
        if not c.any():
            if side == "within":
                warnings.warn("The ensemble of clusterings has only one clustering, consisting of all singletons. This might be "
                              "because you have set Kmin = Kmax = number of points. Falling back to defaults for cohesion parameters.")
            else:
                warnings.warn("The ensemble of clusterings has only one clustering, consisting of a single cluster. This might be "
                              "because you have set Kmin = Kmax = 1. Falling back to defaults for repulsion parameters.")
            res += [1.0, 1.0, 1.0]
            continue
        tw = sx = slx = 0.0
        for k in range(len(c)):
            tw += w[k] * c[k]
            sx += w[k] * S[k]
            slx += w[k] * L[k]
        if not tw > 0:
            raise ValueError(f"fitprior2: the sampled prior on K puts no weight on Kmin..Kmax = {Kmin}..{Kmax}, so the weighted "
                             f"{what} fit has total weight zero (the reference fails in fit_mle here)")
        shape = _gamma_shape_mle(sx / tw, slx / tw)
        res += [shape, tw * shape, sx]
    return tuple(res)


def fitprior2(data, algo: str, diss: bool = False, *, Kmin: int = 1, Kmax: int | None = None, verbose: bool = True,
              seed: int = 0, device: int = 0, ctx: Context | None = None) -> PriorHyperparamsList:
    """fitprior2(data, algo, diss; Kmin, Kmax, verbose) — src/prior.jl:151-277, algo = "k-medoids".

    As fitprior (same inputs, checks and partition-prior fit), but the likelihood hyperparameters are fitted to the
    within / between distances of the clusterings of EVERY k in Kmin..Kmax, each weighted by the prior probability of k
    (pmf of sampleK with max(10^4, 100 N) samples).  The per-k splits come from the device scan (rc_kmedoids_scan_split)
    as exact sufficient statistics; no distance vector is formed.  Streams: the scan and the notional run as in fitprior,
    sample_rp keyed by seed, sampleK by kmedoids_stream_seed(seed, SAMPLEK_STREAM).  ctx: a Context holding the same matrix
    (its state is left as it is).  algo = "k-means" raises NotImplementedError: that path is fitprior2_kmeans."""
    return _fitprior2(data, algo, diss, Kmin, Kmax, verbose, seed, device, ctx, False)


def fitprior2_kmeans(data, *, Kmin: int = 1, Kmax: int | None = None, verbose: bool = True, seed: int = 0, device: int = 0,
                     ctx: Context | None = None) -> PriorHyperparamsList:
    """What the reference's fitprior2(data, "k-means"; Kmin, Kmax, verbose) computes (src/prior.jl:151-277 with
    kmeans(x, k; maxiter = 1000)): as fitprior2, with the scan, its per-k splits (rc_kmeans_scan_split) and the notional
    clustering by k-means on the observations.  data, ctx, seeds and streams as in fitprior_kmeans (the context's state is
    left as it is).  fitprior2(data, "k-means") itself still raises NotImplementedError because the suite pins that; routing
    the string here is a one-line follow-up once that assertion may change."""
    return _fitprior2(data, "k-means", False, Kmin, Kmax, verbose, seed, device, ctx, True)


def _fitprior2(data, algo, diss, Kmin, Kmax, verbose, seed, device, ctx, kmeans_built):
    """The body fitprior2 (k-medoids) and fitprior2_kmeans share."""
    out = print if verbose else (lambda *a, **k: None)
    N, kind, x, Kmax = _prepare("fitprior2", data, algo, diss, Kmin, Kmax, ctx, out, kmeans_built)
    own = ctx is None
    if own:
        ctx = _stage(kind, x, device, data)
    try:
        out("Computing notional clustering.")
        scan_fn, run_fn = _clusterer(ctx, algo)
        scan = scan_fn(Kmin, Kmax, maxiter=1000, seed=kmedoids_stream_seed(seed, KMED_STREAM_SCAN), split=True)
        for k in np.flatnonzero(~scan["converged"]) + Kmin:
            warnings.warn(f"Clustering did not converge at K = {k}")
        K = int(detectknee(np.arange(Kmin, Kmax + 1), scan["totalcost"])[0])
        notional = run_fn(K, maxiter=1000, seed=kmedoids_stream_seed(seed, KMED_STREAM_NOTIONAL)).assignments

        out("Computing partition prior hyperparameters.")
        proposalsd_r, eta, sigma, u, v = _partition_prior(notional, verbose, seed)
        Ks = sampleK(eta, sigma, u, v, max(10000, 100 * N), N, seed=kmedoids_stream_seed(seed, SAMPLEK_STREAM), device=device)
        Kprior = pmf(Ks, N)

        out("Computing likelihood hyperparameters.")
        delta1, alpha, beta, delta2, zeta, gamma = _fit_weighted(scan, Kprior, Kmin, Kmax)
        return PriorHyperparamsList(delta1=delta1, delta2=delta2, alpha=alpha, beta=beta, zeta=zeta, gamma=gamma, eta=eta,
                                    sigma=sigma, proposalsd_r=proposalsd_r, u=u, v=v, K_initial=K)
    finally:
        if own:
            ctx.close()
