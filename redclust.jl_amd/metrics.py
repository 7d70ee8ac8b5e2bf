"""Metrics from coordinates: the names of include/redclust_hip.h's RC_METRIC_* (SciPy's and Distances.jl's), their checks
before the library is touched, the plain-NumPy evaluation the host uses, and pairwise(), the raw distances from the device
(rc_pairwise).  DESIGN.md §8 "Metrics from coordinates"."""
from __future__ import annotations

import numpy as np

from . import _lib

METRICS = _lib.METRICS
check_metric = _lib.check_metric


def _points(points, what="points"):
    X = np.ascontiguousarray(points, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"{what} must be a non-empty rows×dim array (one observation per row)")
    if not np.all(np.isfinite(X)):
        raise ValueError(f"{what} must be finite")
    return X


def host_pairwise(new_points, points, metric: str = "euclidean") -> np.ndarray:
    """The q×n distances of the rows of new_points to the rows of points in plain NumPy: direct differences, sums by
    np.sum — close to the device's values and not bit-equal to them (the device's arithmetic is the stated chain of the
    header; NumPy's sums are pairwise)."""
    check_metric(metric)
    Y, X = np.asarray(new_points, np.float64), np.asarray(points, np.float64)
    if metric in ("cosine", "correlation"):
        if metric == "correlation":
            Y = Y - (Y.sum(axis=1) / Y.shape[1])[:, None]
            X = X - (X.sum(axis=1) / X.shape[1])[:, None]
        ny, nx = np.sqrt(np.einsum("ij,ij->i", Y, Y)), np.sqrt(np.einsum("ij,ij->i", X, X))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.maximum(1.0 - (Y @ X.T) / (ny[:, None] * nx[None, :]), 0.0)
    out = np.empty((len(Y), len(X)))
    for i, y in enumerate(Y):                                         # a row at a time: q·n·dim doubles need not fit
        t = np.abs(y[None, :] - X)
        if metric == "cityblock":
            out[i] = t.sum(axis=1)
        elif metric == "chebyshev":
            out[i] = t.max(axis=1)
        else:
            sq = np.einsum("ij,ij->i", t, t)
            out[i] = np.sqrt(sq) if metric == "euclidean" else sq
    return out


def host_matrix(points, metric: str) -> np.ndarray:
    """The symmetric n×n matrix of host_pairwise(points, points) with a zero diagonal."""
    D = host_pairwise(points, points, metric)
    D = np.minimum(D, D.T)
    np.fill_diagonal(D, 0.0)
    return np.ascontiguousarray(D)


def pairwise(points, new_points=None, *, metric: str = "euclidean", device: int = 0) -> np.ndarray:
    """The raw distances as the device computes them (rc_pairwise), in the arithmetic include/redclust_hip.h states for
    each metric.  Without new_points: the symmetric n×n matrix of the n×dim points, zero diagonal — what
    Context.from_points(points, metric=metric) quantises.  With new_points (q×dim): the q×n matrix, new point against
    training point — what predict_points(..., metric=metric) uses.  Nothing about the values is refused: zero distances
    are legal here."""
    X = _points(points)
    check_metric(metric, X.shape[1])
    Y = None
    if new_points is not None:
        Y = _points(new_points, "new_points")
        if Y.shape[1] != X.shape[1]:
            raise ValueError("new_points must have the coordinates of points (q×dim)")
    return _lib.pairwise(X, Y, metric=metric, device=device)
