"""Synthetic benchmark inputs with the distribution of the reference's generatemixture
(/root/reference/src/utils.jl:101-147) — the build's own generator (Julia's RNG stream cannot be reproduced) — its
oracle co-clustering matrix (utils.jl:130-143, O(5000·N²·K): built on the device by rc_oracle_coclustering)
and the likelihood hyperparameters fitted from a labelling with fitprior's formulas
(/root/reference/src/prior.jl:73-75,96-110)."""
from __future__ import annotations

import numpy as np
from scipy.special import digamma, polygamma

ORACLE_TAG = 0x4F524143   # "ORAC": the oracle's Dirichlet draws come from default_rng([ORACLE_TAG, seed])
ORACLE_MAX_N = 1 << 16    # rc_oracle_coclustering holds the n² sum on the device


def _int(name, v, lo):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo} (got {v!r}).")
    return int(v)


def _positive(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not (
            np.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be positive and finite (got {v!r}).")
    return float(v)


def _oracle_inputs(points, K, alpha, radius, sigma, numiters, seed, weights):
    """Checks the arguments of oracle_coclustering on the host; returns (points, K, radius, sigma, weights) as the
    library takes them."""
    X = np.asarray(points)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or not np.issubdtype(X.dtype, np.number) \
            or np.iscomplexobj(X):
        raise ValueError("points must be a real N×dim matrix, one observation per row.")
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, dim = X.shape
    if n > ORACLE_MAX_N:
        raise ValueError(f"N must be at most {ORACLE_MAX_N} (the device holds the N² sum).")
    K = _int("K", K, 1)
    if K > dim:
        raise ValueError("K must satisfy 1 ≤ K ≤ dim.")
    radius, sigma = _positive("radius", radius), _positive("σ", sigma)
    if not np.all(np.isfinite(X)):
        raise ValueError("points must be finite.")
    with np.errstate(over="ignore"):
        if not np.all(np.isfinite(radius * X[:, :K] / sigma ** 2)):
            raise ValueError("radius·x/σ² must be finite.")
    if weights is None:
        alpha = float(K) if alpha is None else _positive("α", alpha)
        numiters = 5000 if numiters is None else _int("numiters", numiters, 1)
        W = np.random.default_rng([ORACLE_TAG, _int("seed", seed, 0)]).dirichlet(np.full(K, alpha), size=numiters)
    else:
        if alpha is not None:
            _positive("α", alpha)
        W = np.asarray(weights)
        if W.ndim != 2 or W.shape[1] != K or W.shape[0] < 1 or not np.issubdtype(W.dtype, np.number) \
                or np.iscomplexobj(W):
            raise ValueError("weights must be a real numiters×K matrix.")
        if numiters is not None and _int("numiters", numiters, 1) != W.shape[0]:
            raise ValueError(f"numiters ({numiters}) differs from the rows of weights ({W.shape[0]}).")
        W = np.ascontiguousarray(W, dtype=np.float64)
        if not np.all(np.isfinite(W)) or np.any(W < 0) or not np.all(W.max(axis=1) > 0):
            raise ValueError("every weight row must be finite and non-negative with a positive entry.")
    return X, K, radius, sigma, W


def oracle_coclustering(points, K: int, *, alpha: float | None = None, radius: float = 1.0, sigma: float = 0.1,
                        numiters: int | None = None, seed: int = 0, weights=None, iters_per_chunk: int = 0,
                        device: int = 0) -> np.ndarray:
    """generatemixture's oracle co-clustering matrix (utils.jl:130-143) for N×dim points (one observation per row):
    (1/T)·Σ_t P_t P_tᵀ with P_t the posterior of the K components, centres radius·e_j and covariance σ²I, under
    weights w_t ~ Dirichlet(K, α), α = K by default.  The weights come from a stream of their own,
    default_rng([ORACLE_TAG, seed]), or are the caller's `weights` (numiters × K, non-negative, rows need not sum to 1;
    numiters then defaults to its rows).  numiters defaults to 5000, as in the reference.

    Computed on the device as softmax_j(log w_tj + radius·x_ij/σ²): finite where the reference's literal
    pdf ratio is Inf/Inf or 0/0.  The result is exactly symmetric and the same bits for any
    iters_per_chunk (iterations per device pass, 0 = automatic).  Returns an N×N float64 array."""
    X, K, radius, sigma, W = _oracle_inputs(points, K, alpha, radius, sigma, numiters, seed, weights)
    iters_per_chunk, device = _int("iters_per_chunk", iters_per_chunk, 0), _int("device", device, 0)
    from ._lib import oracle_coclustering as _device_oracle
    return _device_oracle(X, K, radius, sigma, W, iters_per_chunk, device)[0]


_oracle_coclustering = oracle_coclustering   # generatemixture's flag of the same name shadows it there


def generatemixture(N: int, K: int, *, alpha: float | None = None, dim: int | None = None, radius: float = 1.0,
                    sigma: float = 0.1, seed: int = 0, dtype=np.float64, points_only: bool = False,
                    oracle_coclustering: bool = False, device: int = 0):
    """Points, generating labels, mixture weights and (unless points_only) the distance matrix.  With
    oracle_coclustering=True the dict also holds "oracle_coclustering", the reference's fifth output (T = 5000) for
    the returned points, computed on `device`; it equals the standalone function with the same α, radius, σ and seed."""
    if N < 1:
        raise ValueError("N must be greater than 1.")
    if K < 1 or K > N:
        raise ValueError("K must satisfy 1 ≤ K ≤ N.")
    alpha = float(K) if alpha is None else float(alpha)
    dim = K if dim is None else int(dim)
    if alpha <= 0:
        raise ValueError("α must be positive.")
    if dim < K:
        raise ValueError("dim must be ≥ K.")
    if radius <= 0 or sigma <= 0:
        raise ValueError("radius and σ must be positive.")
    rng = np.random.default_rng(seed)
    probs = rng.dirichlet(np.full(K, alpha))                      # utils.jl:113
    clusts = np.sort(rng.choice(K, size=N, p=probs)) + 1          # utils.jl:114 (sorted labels)
    pts = rng.normal(0.0, sigma, size=(N, dim))                   # utils.jl:123-128
    pts[np.arange(N), clusts - 1] += radius                       # centre k = radius·e_k, utils.jl:117-120
    out = dict(points=pts, distancematrix=None, clusts=clusts.astype(np.int64), probs=probs)
    if oracle_coclustering:
        out["oracle_coclustering"] = _oracle_coclustering(pts, K, alpha=alpha, radius=radius, sigma=sigma, seed=seed,
                                                          device=device)
    if points_only:   # the n×n matrix is left to the device (MCMCData(points), rc_create_from_points)
        return out
    # pairwise Euclidean distances (utils.jl:144-145), built block-row-wise so that N = 32768 needs one N×N array
    sq = np.einsum("ij,ij->i", pts, pts)
    D = np.empty((N, N), dtype=np.float64)
    B = 2048
    for i0 in range(0, N, B):
        i1 = min(N, i0 + B)
        blk = pts[i0:i1] @ pts.T
        blk *= -2.0
        blk += sq[i0:i1, None]
        blk += sq[None, :]
        np.maximum(blk, 0.0, out=blk)
        np.sqrt(blk, out=D[i0:i1])
    # exact symmetry (types.jl:149-151 requires it): mirror the upper triangle, zero diagonal
    for i0 in range(0, N, B):
        i1 = min(N, i0 + B)
        for j0 in range(i0, N, B):
            j1 = min(N, j0 + B)
            if i0 == j0:
                t = D[i0:i1, j0:j1]
                iu = np.triu_indices(i1 - i0, 1)
                t.T[iu] = t[iu]
            else:
                D[j0:j1, i0:i1] = D[i0:i1, j0:j1].T
    np.fill_diagonal(D, 0.0)
    out["distancematrix"] = D if dtype == np.float64 else D.astype(dtype)
    return out


def _gamma_shape_mle(mean_x, mean_logx):
    s = np.log(mean_x) - mean_logx
    k = (3 - s + np.sqrt((s - 3) ** 2 + 24 * s)) / (12 * s)
    for _ in range(100):
        k_new = k - (np.log(k) - digamma(k) - s) / (1 / k - polygamma(1, k))
        if abs(k_new - k) < 1e-14 * k:
            return float(k_new)
        k = k_new
    return float(k)


def likelihood_hyperparams(D: np.ndarray, labels: np.ndarray, block: int = 2048) -> dict:
    """δ1, α, β from within-cluster distances A; δ2, ζ, γ from between-cluster distances B (upper triangle)."""
    n = D.shape[0]
    cntA = cntB = 0
    sumA = sumB = slogA = slogB = 0.0
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        sub = D[i0:i1]
        same = labels[i0:i1, None] == labels[None, :]
        upper = np.arange(i0, i1)[:, None] < np.arange(n)[None, :]
        a = sub[same & upper]
        b = sub[(~same) & upper]
        cntA += a.size; cntB += b.size
        sumA += float(a.sum()); sumB += float(b.sum())
        slogA += float(np.log(a).sum()); slogB += float(np.log(b).sum())
    d1 = _gamma_shape_mle(sumA / cntA, slogA / cntA)
    d2 = _gamma_shape_mle(sumB / cntB, slogB / cntB)
    return dict(delta1=d1, delta2=d2, alpha=cntA * d1, beta=sumA, zeta=cntB * d2, gamma=sumB,
                eta=1.0, sigma=1.0, u=1.0, v=1.0, repulsion=True, maxK=0)


def likelihood_hyperparams_device(ctx, labels) -> dict:
    """likelihood_hyperparams with the within / between sums taken from the device's block sums (rc_within_between):
    no host pass over the n×n matrix.  ctx: a Context holding D; its state is set to `labels`."""
    ctx.set_state(np.asarray(labels, dtype=np.int64))
    w = ctx.within_between()
    cntA, cntB = w["count_within"], w["count_between"]
    d1 = _gamma_shape_mle(w["sum_within"] / cntA, w["sumlog_within"] / cntA)
    d2 = _gamma_shape_mle(w["sum_between"] / cntB, w["sumlog_between"] / cntB)
    return dict(delta1=d1, delta2=d2, alpha=cntA * d1, beta=w["sum_within"], zeta=cntB * d2, gamma=w["sum_between"],
                eta=1.0, sigma=1.0, u=1.0, v=1.0, repulsion=True, maxK=0)
