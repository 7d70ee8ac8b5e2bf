"""NumPy restatement of generatemixture's oracle co-clustering matrix (src/utils.jl:130-143 of the reference; the device
form is csrc/mixture.inc.hip, rc_oracle_coclustering), written from DESIGN.md §8 (TEST INFRASTRUCTURE):

    b_ij = radius·x_ij/σ²   (j = 1..K: the centres are radius·e_j, every other factor of the pdf cancels),
    P_t[i, j] = softmax_j(log w_tj + b_ij)   (row maximum subtracted),
    oracle = (1/T)·Σ_t P_t P_tᵀ,

and the literal form of the reference, w_j·exp(logpdf(MvNormal(c_j, σ²I), x_i)) normalised over j."""
from __future__ import annotations

import numpy as np

ORACLE_TAG = 0x4F524143   # "ORAC": the Dirichlet stream is default_rng([ORACLE_TAG, seed]), not default_rng(seed)


def dirichlet_weights(K: int, alpha: float, numiters: int, seed: int) -> np.ndarray:
    """The package's default weights: numiters × K draws of Dirichlet(K, alpha) from their own stream."""
    return np.random.default_rng([ORACLE_TAG, int(seed)]).dirichlet(np.full(K, float(alpha)), size=int(numiters))


def logits(points, K, radius, sigma):
    return float(radius) * np.asarray(points, dtype=np.float64)[:, :K] / float(sigma) ** 2


def posterior(B, w):
    """P_t (N × K) for one weight row w."""
    with np.errstate(divide="ignore"):
        z = np.log(np.asarray(w, dtype=np.float64))[None, :] + B
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=1, keepdims=True)


def oracle(points, K, weights, radius=1.0, sigma=0.1, rows=None, block=256):
    """(1/T)·Σ_t P_t P_tᵀ, or only the given rows of it; summed `block` iterations at a time through one matmul."""
    B = logits(points, K, radius, sigma)
    W = np.asarray(weights, dtype=np.float64)
    T = W.shape[0]
    idx = np.arange(B.shape[0]) if rows is None else np.asarray(rows)
    S = np.zeros((len(idx), B.shape[0]))
    for t0 in range(0, T, block):
        Q = np.concatenate([posterior(B, W[t]) for t in range(t0, min(T, t0 + block))], axis=1)
        S += Q[idx] @ Q.T
    return S / T


def literal_posterior(points, K, w, radius=1.0, sigma=0.1):
    """P_t as the reference computes it: w_j·pdf(MvNormal(radius·e_j, σ²I), x_i), normalised over j (NaN where every
    term over- or underflows, as Inf/Inf or 0/0 there)."""
    X = np.asarray(points, dtype=np.float64)
    dim = X.shape[1]
    C = np.zeros((K, dim))
    C[np.arange(K), np.arange(K)] = radius
    d2 = ((X[:, None, :] - C[None, :, :]) ** 2).sum(axis=2)
    logpdf = -0.5 * dim * np.log(2 * np.pi * sigma ** 2) - d2 / (2 * sigma ** 2)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(w, dtype=np.float64)[None, :] * np.exp(logpdf)
        return p / p.sum(axis=1, keepdims=True)
