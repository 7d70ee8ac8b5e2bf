"""Restatement of the metrics' arithmetic (include/redclust_hip.h "Metrics from coordinates") in Python floats —
TEST INFRASTRUCTURE — and the fixed inputs of its tests.

Python's + − * / on floats and math.sqrt are the IEEE-754 binary64 operations, rounded to nearest even; only the fused
multiply-add is missing (Python 3.10), and it is predict_points_ref.fma: exact rational arithmetic, rounded once.  For a pair
(y, x) the coordinates are walked in ascending order and every accumulator starts at +0.0:

  euclidean    t = y_k − x_k; acc = fma(t, t, acc); d = sqrt(acc)
  sqeuclidean  the same chain; d = acc
  cityblock    t = y_k − x_k; acc = acc + |t|
  chebyshev    t = y_k − x_k; acc = max(acc, |t|)
  cosine       per point: nn = fma(x_k, x_k, nn), norm = sqrt(nn); per pair: dot = fma(y_k, x_k, dot); s = norm_y·norm_x;
               c = dot / s; d = max(1 − c, 0)
  correlation  cosine on centred coordinates: sum = sum + x_k; mu = sum / dim; x'_k = x_k − mu

Slow, which is fine at the shapes of the tests; the cases are cached and never written to."""
from __future__ import annotations

import functools
import math

import numpy as np

import predict_points_ref as PR

fma = PR.fma

METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev", "cosine", "correlation")
ANGULAR = ("cosine", "correlation")
# (n, dim, q), at the tile edges of both kernels: 64 pairs and 16 coordinates per tile of the symmetric kernel, 256 training
# points per strip and 8 new points per block of the q×n kernel
SHAPES = [(2, 3, 1), (63, 3, 1), (64, 16, 64), (65, 17, 65), (129, 33, 3), (200, 5, 70), (257, 3, 9)]
DIM1_SHAPE = (63, 1, 1)     # the four non-angular metrics only: in one dimension every cosine distance is 0 or 2


def shapes(metric):
    return SHAPES + ([] if metric in ANGULAR else [DIM1_SHAPE])


def prepared(metric, x):
    """(the coordinates the pair chain sees, the point's norm): centred for correlation; the norm is 1.0 where unused"""
    x = [float(v) for v in x]
    if metric not in ANGULAR:
        return x, 1.0
    if metric == "correlation":
        total = 0.0
        for v in x:
            total = total + v
        mu = total / float(len(x))
        x = [v - mu for v in x]
    nn = 0.0
    for v in x:
        nn = fma(v, v, nn)
    return x, math.sqrt(nn)


def pair(metric, y, ny, x, nx) -> float:
    """the distance of two prepared points"""
    acc = 0.0
    if metric in ANGULAR:
        for yk, xk in zip(y, x):
            acc = fma(yk, xk, acc)
        s = ny * nx
        c = acc / s
        return max(1.0 - c, 0.0)
    for yk, xk in zip(y, x):
        t = yk - xk
        if metric in ("euclidean", "sqeuclidean"):
            acc = fma(t, t, acc)
        elif metric == "cityblock":
            acc = acc + abs(t)
        else:
            acc = max(acc, abs(t))
    return math.sqrt(acc) if metric == "euclidean" else acc


def distance(metric, y, x) -> float:
    (yp, ny), (xp, nx) = prepared(metric, y), prepared(metric, x)
    return pair(metric, yp, ny, xp, nx)


def distances(metric, Y, X) -> np.ndarray:
    """q×n: row i the distances of new point i (row of Y) to every training point (row of X)"""
    PY, PX = [prepared(metric, y) for y in np.asarray(Y, np.float64)], [prepared(metric, x) for x in np.asarray(X, np.float64)]
    return np.array([[pair(metric, y, ny, x, nx) for x, nx in PX] for y, ny in PY], np.float64).reshape(len(PY), len(PX))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _euclid_family(n, dim, q):
    """the q×n squared chain of euclidean / sqeuclidean, walked once for both"""
    X, Y = PR.coordinates(n, dim, q)
    return distances("sqeuclidean", Y, X)


@functools.lru_cache(maxsize=None)
def case(metric, n, dim, q):
    """(X, Y, the restated q×n distances of Y against X)"""
    X, Y = PR.coordinates(n, dim, q)
    if metric in ("euclidean", "sqeuclidean"):
        sq = _euclid_family(n, dim, q)
        D = np.array([math.sqrt(v) for v in sq.ravel()]).reshape(sq.shape) if metric == "euclidean" else sq.copy()
    else:
        D = distances(metric, Y, X)
    return _frozen(X, Y, D)


@functools.lru_cache(maxsize=None)
def _euclid_family_self(n, dim, q):
    X, _ = PR.coordinates(n, dim, q)
    return _lower_mirrored("sqeuclidean", X)


def _lower_mirrored(metric, X):
    """X against X: the lower triangle by the restatement, mirrored (every metric is symmetric bit for bit, which
    test_metrics_cpu.py checks), the diagonal left at 0"""
    P = [prepared(metric, x) for x in X]
    n = len(P)
    D = np.zeros((n, n))
    for i in range(n):
        for j in range(i):
            D[i, j] = D[j, i] = pair(metric, P[i][0], P[i][1], P[j][0], P[j][1])
    return D


@functools.lru_cache(maxsize=None)
def self_case(metric, n, dim, q):
    """(X, the restated n×n distances of X against X off the diagonal; the diagonal holds 0)"""
    X, _ = PR.coordinates(n, dim, q)
    if metric in ("euclidean", "sqeuclidean"):
        sq = _euclid_family_self(n, dim, q)
        D = np.array([math.sqrt(v) for v in sq.ravel()]).reshape(sq.shape) if metric == "euclidean" else sq.copy()
    else:
        D = _lower_mirrored(metric, X)
    return _frozen(X, D)
