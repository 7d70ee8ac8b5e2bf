"""NumPy restatement of the device k-medoids (csrc/kmedoids.inc.hip; algorithm: DESIGN.md §8) — TEST INFRASTRUCTURE.

Clustering.jl's kmedoids(D, k; maxiter, tol) with k-medoids++ seeding by costs, on the fixed-point matrix the device
holds: Dq = rint(D·2^eD) as int64 (D from Context.get_matrix(0), eD from Context.debug_rowsums after a set_state).
Integer sums, the same tie rules and the same Philox stream, so the device must agree exactly."""
from __future__ import annotations

import numpy as np

from np_transcription import M32, philox4x32_10

KMED_TAG = 0x4B4D4544


def u53(seed: int, k: int, step: int) -> int:
    c = philox4x32_10((step, k, 0, 0), (seed & M32, ((seed >> 32) & M32) ^ KMED_TAG))
    return ((c[0] << 32) | c[1]) >> 11


def draw(weights: np.ndarray, u: int) -> int:
    """The first index whose inclusive prefix sum exceeds (u·W) >> 53, W = Σ weights (integers throughout)."""
    W = int(weights.sum())
    if W <= 0:
        raise ValueError("every seeding weight is zero")
    thr = (u * W) >> 53
    return int(np.argmax(np.cumsum(weights) > thr))


def kmpp_seeds(Dq: np.ndarray, k: int, seed: int) -> list:
    n = Dq.shape[0]
    p = (u53(seed, k, 0) * n) >> 53
    med = [p]
    mincost = Dq[p].astype(np.int64).copy()
    mincost[p] = 0
    for s in range(1, k):
        p = draw(mincost, u53(seed, k, s))
        med.append(p)
        np.minimum(mincost, Dq[p], out=mincost)
        mincost[p] = 0
    return med


def assign(Dq: np.ndarray, med) -> tuple:
    """Nearest medoid per point, ties to the first medoid in medoid order; (0-based assignments, integer total cost)."""
    costs = Dq[np.asarray(med)]
    a = np.argmin(costs, axis=0)
    return a, int(costs[a, np.arange(Dq.shape[0])].sum())


def find_medoid(Dq: np.ndarray, grp: np.ndarray) -> int:
    """The member with the smallest sum of distances to its group, ties to the lowest point index (grp ascending)."""
    return int(grp[np.argmin(Dq[np.ix_(grp, grp)].sum(axis=0))])


def update_medoids(Dq: np.ndarray, a: np.ndarray, k: int) -> list:
    med = []
    for g in range(k):
        grp = np.flatnonzero(a == g)
        if len(grp) == 0:
            raise ValueError("empty k-medoids group")
        med.append(find_medoid(Dq, grp))
    return med


def kmedoids(Dq: np.ndarray, eD: int, k: int, maxiter: int = 200, tol: float = 1e-8, seed: int = 0) -> dict:
    Dq = np.asarray(Dq, dtype=np.int64)
    med = kmpp_seeds(Dq, k, seed)
    a, tc = assign(Dq, med)
    t, conv = 0, False
    while not conv and t < maxiter:
        t += 1
        med = update_medoids(Dq, a, k)
        prev = tc
        a, tc = assign(Dq, med)
        conv = float(abs(tc - prev)) * 2.0 ** -eD < tol
    return dict(medoids=np.asarray(med, np.int64) + 1, assignments=a.astype(np.int64) + 1, totalcost=float(tc) * 2.0 ** -eD,
                totalcost_q=tc, iterations=t, converged=conv)


def device_matrix(ctx) -> tuple:
    """(Dq int64, eD) of a Context: a state is set first if it has none (eD comes with rc_debug_rowsums)."""
    try:
        _, _, eD, _ = ctx.debug_rowsums(1)
    except Exception:
        ctx.set_state(np.ones(ctx.n, np.int64))
        _, _, eD, _ = ctx.debug_rowsums(1)
    D = ctx.get_matrix(0)
    return np.rint(np.ldexp(D, eD)).astype(np.int64), eD
