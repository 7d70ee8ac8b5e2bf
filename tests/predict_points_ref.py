"""Restatement of rc_predict_points' distance (include/redclust_hip.h, DESIGN.md §8 "Predict from points") — TEST
INFRASTRUCTURE — and the fixed inputs of its tests.

d_ij = sqrt(Σ_k (y_ik − x_jk)²), coordinates ascending: acc = +0; per coordinate t = y − x (one rounding) and
acc = fma(t, t, acc) (one rounding); one correctly rounded square root.  Python 3.10 has no math.fma, so the fused step is
float(Fraction(t)·Fraction(t) + Fraction(acc)): exact rational arithmetic, and Fraction.__float__ rounds correctly (to nearest
even).  math.sqrt is the correctly rounded IEEE square root.  Slow, which is fine at the shapes of the tests."""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

import predict_ref as PR

DIST_SHAPES = [(1, 1, 1), (63, 1, 1), (64, 16, 64), (65, 17, 65), (129, 33, 3), (200, 5, 70)]     # (n, dim, q)


def fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def distance(y, x) -> float:
    acc = 0.0
    for yk, xk in zip(y, x):
        t = float(yk) - float(xk)
        acc = fma(t, t, acc)
    return math.sqrt(acc)


def distances(Y, X) -> np.ndarray:
    """q×n: row i the distances of new point i (row of Y) to every training point (row of X)"""
    Y, X = np.asarray(Y, np.float64), np.asarray(X, np.float64)
    return np.array([[distance(y, x) for x in X] for y in Y], np.float64).reshape(len(Y), len(X))


def exact_distance_sq(y, x) -> Fraction:
    return sum(((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(y, x)), Fraction(0))


def coordinates(n, dim, q, seed=None):
    """(X, Y): n training and q new points around a few centres, full 53-bit mantissas, no new point on a training point"""
    rng = np.random.default_rng(1000003 * n + 1009 * dim + q if seed is None else seed)
    K = min(4, n)
    centres = 3.0 * rng.standard_normal((K, dim))
    X = centres[rng.integers(0, K, n)] + 0.5 * rng.standard_normal((n, dim))
    Y = centres[rng.integers(0, K, q)] + 0.5 * rng.standard_normal((q, dim))
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


@functools.lru_cache(maxsize=None)
def dist_case(n, dim, q):
    """(X, Y, the restated q×n distances) — computed once, shared by the tests, never written to"""
    X, Y = coordinates(n, dim, q)
    D = distances(Y, X)
    for a in (X, Y, D):
        a.setflags(write=False)
    return X, Y, D


@functools.lru_cache(maxsize=None)
def predict_case(repulsion=True):
    """n = 200 training points in dim 5, q = 70 new points, m = 12 samples: sample 0 one cluster (named 7), sample 1 all
    singletons, the rest 2..6 clusters whose names have gaps; maxK = 4, so the samples of 4 and more clusters offer no new
    cluster and the others do; r, p per sample; non-zero offsets."""
    n, dim, q, m = 200, 5, 70, 12
    X, Y = coordinates(n, dim, q, seed=20070)
    rng = np.random.default_rng(12)
    names = np.array([3, 9, 17, 40, 100, 200], np.int64)
    S = np.empty((m, n), np.int64)
    S[0] = 7
    S[1] = rng.permutation(n) + 1
    for s in range(2, m):
        k = 2 + (s - 2) % 5
        z = names[rng.integers(0, k, n)]
        z[:k] = names[:k]                                           # every one of the k names is used
        S[s] = z
    r = rng.uniform(0.5, 3.0, m)
    p = rng.uniform(0.2, 0.8, m)
    P = dict(PR.PARAMS, maxK=4, repulsion=bool(repulsion))
    K = np.array([len(np.unique(z)) for z in S])
    assert K.min() == 1 and K.max() == n and np.any(K < 4) and np.any((K >= 4) & (K < n))
    for a in (X, Y, S, r, p):
        a.setflags(write=False)
    return dict(X=X, Y=Y, samples=S, r=r, p=p, P=P, seed=0xC0FFEE12345, sample_offset=(1 << 33) + 5, point_offset=(1 << 32) + 77,
                Kmax=int(K.max()), K=K, n=n, dim=dim, q=q, m=m)


def pivot_of_case():
    """a pivot of three clusters (names with gaps): fewer than most samples have, so column 0 of the counts is populated"""
    n = predict_case()["n"]
    return np.array([5, 50, 120], np.int64)[np.arange(n) % 3]
