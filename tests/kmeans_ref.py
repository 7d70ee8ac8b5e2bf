"""NumPy restatement of the device k-means (csrc/kmeans.inc.hip; algorithm: DESIGN.md §8 "k-means (built)") — TEST
INFRASTRUCTURE.

Clustering.jl's kmeans(X, k; maxiter, tol) with :kmpp seeding on f64 points (one per row), with every order the device
fixes restated literally: squared distances summed over ascending coordinates (a subtraction, a multiplication, an
addition), centres as the sum of the members in ascending point index and one division, the objective as 256 strided
partials and a halving tree, the weighted draws in integers on the same Philox stream.  The device must agree bit for bit."""
from __future__ import annotations

import math

import numpy as np

from np_transcription import M32, philox4x32_10

KMNS_TAG = 0x4B4D4E53


def u53(seed: int, k: int, draw: int) -> int:
    c = philox4x32_10((draw, k, 0, 0), (seed & M32, ((seed >> 32) & M32) ^ KMNS_TAG))
    return ((c[0] << 32) | c[1]) >> 11


def draw_shift(X: np.ndarray) -> int:
    """s of the integer weights floor(w · 2^s): 61 - ceil(log2 n) - ex with B < 2^ex the squared diagonal of the bounding
    box (summed over ascending coordinates), clamped to ±2000; 0 when B is zero or not finite."""
    n = X.shape[0]
    B = 0.0
    for c in range(X.shape[1]):
        d = float(X[:, c].max()) - float(X[:, c].min())
        B = B + d * d
    if not (B > 0.0) or not math.isfinite(B):
        return 0
    ex = math.frexp(B)[1]
    clog = 0
    while (1 << clog) < n:
        clog += 1
    return max(-2000, min(2000, 61 - clog - ex))


def sqdist(X: np.ndarray, M: np.ndarray) -> np.ndarray:
    """n×k squared distances between the rows of X and the rows of M, summed over ascending coordinates."""
    acc = np.zeros((X.shape[0], M.shape[0]))
    for c in range(X.shape[1]):
        d = X[:, c, None] - M[None, :, c]
        acc += d * d
    return acc


def draw_weights(w: np.ndarray, shift: int) -> np.ndarray:
    """q = floor(w · 2^shift), the integer weights of a draw."""
    return np.floor(np.ldexp(w, shift)).astype(np.int64)


def weighted_draw(w: np.ndarray, shift: int, u: int) -> int:
    """The first index whose inclusive prefix sum of q = floor(w · 2^shift) exceeds (u · W) >> 53, W = Σ q."""
    q = draw_weights(w, shift)
    W = int(q.sum(dtype=np.int64))
    if W <= 0:
        raise ValueError("every weight of the draw is zero")
    thr = (u * W) >> 53
    return int(np.argmax(np.cumsum(q, dtype=np.int64) > thr))


def objective(costs: np.ndarray) -> float:
    p = np.zeros(256)
    for b in range(0, len(costs), 256):
        seg = costs[b:b + 256]
        p[:len(seg)] += seg
    h = 128
    while h:
        p[:h] += p[h:2 * h]
        h //= 2
    return float(p[0])


def assign(X: np.ndarray, M: np.ndarray) -> tuple:
    """(0-based assignments with ties to the lowest centre, costs, counts, objv)"""
    d = sqdist(X, M)
    a = np.argmin(d, axis=1)
    costs = d[np.arange(X.shape[0]), a]
    return a, costs, np.bincount(a, minlength=M.shape[0]).astype(np.int64), objective(costs)


def ordered_mean(X: np.ndarray, members: np.ndarray) -> np.ndarray:
    """Σ of the member rows in ascending point index (cumsum adds row after row), then one division."""
    return np.cumsum(X[members], axis=0)[-1] / float(len(members))


def kmpp_seeds(X: np.ndarray, k: int, seed: int) -> list:
    """The k-means++ seeds (0-based point indices) in the order they are drawn."""
    n = X.shape[0]
    shift = draw_shift(X)
    p = (u53(seed, k, 0) * n) >> 53
    seeds = [p]
    mincost = sqdist(X, X[p:p + 1])[:, 0]
    mincost[p] = 0.0
    for s in range(1, k):
        p = weighted_draw(mincost, shift, u53(seed, k, s))
        seeds.append(p)
        mincost = np.minimum(mincost, sqdist(X, X[p:p + 1])[:, 0])
        mincost[p] = 0.0
    return seeds


def kmeans(X, k: int, maxiter: int = 100, tol: float = 1e-6, seed: int = 0, init=None) -> dict:
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    shift = draw_shift(X)
    ndraw = 0
    if init is not None:
        M = X[np.asarray(init, dtype=np.int64) - 1].copy()
    else:
        M = X[np.asarray(kmpp_seeds(X, k, seed))].copy()
        ndraw = k
    a, costs, counts, objv = assign(X, M)
    t, conv, repicks = 0, False, 0
    while not conv and t < maxiter:
        t += 1
        empty = []
        for g in range(k):
            members = np.flatnonzero(a == g)
            if len(members):
                M[g] = ordered_mean(X, members)
            else:
                empty.append(g)
        if empty:
            w = costs.copy()
            for g in empty:
                j = weighted_draw(w, shift, u53(seed, k, ndraw))
                ndraw += 1
                repicks += 1
                M[g] = X[j]
                w = np.minimum(w, sqdist(X, X[j:j + 1])[:, 0])
        prev = objv
        a, costs, counts, objv = assign(X, M)
        change = objv - prev
        if change > tol:
            pass   # the reference warns that the objective went up, and goes on
        elif k == 1 or abs(change) < tol:
            conv = True
    return dict(centers=M, assignments=a.astype(np.int64) + 1, costs=costs, counts=counts, totalcost=objv, iterations=t,
                converged=conv, repicks=repicks)
