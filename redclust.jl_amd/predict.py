"""Predict: allocate observations that were not in the fit to the clusters of every posterior sample, on the GPU
(csrc/predict.inc.hip through rc_predict; include/redclust_hip.h has the contract, DESIGN.md §8 "Predict" the design).
Under one sample the allocation of a new observation is the Gibbs full conditional of an (n+1)-th point whose own cluster is
empty; predict allocates new observations independently of each other given a sample, predict_joint (rc_predict_joint,
csrc/predictjoint.inc.hip, DESIGN.md §8 "Joint predict") one after the other and then by Gibbs passes, so that new
observations may form clusters with each other.  There is no CPU fallback."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib

_DIST_CHUNK_BYTES = 64 << 20   # the difference tensor of one chunk of new points (rows × n × dim f64)


@dataclass
class Prediction:
    """labels[s, i]: the label new point i drew under sample s, in that sample's own label names; 0 = a cluster of its own.
    map_labels: the most probable label instead of a draw.  scores (optional, m×q×(Kmax+1)): the noise-free log weights —
    column t < K_s belongs to the t-th smallest label of sample s, the last column to a new cluster (-inf when maxK forbids
    it), NaN between.  kernel_ms: device time of the kernels.  From predict_points with a relabelling: counts and map_counts
    (q×(K_p+1) uint32: in how many samples the draw / the most probable label of each new point lands in each of the pivot's
    clusters, column 0 a cluster of its own or one without a counterpart) and pivot_labels (the K_p names of columns 1..K_p);
    labels and map_labels are then None unless kept."""
    labels: np.ndarray | None
    map_labels: np.ndarray | None
    scores: np.ndarray | None = None
    kernel_ms: float = 0.0
    counts: np.ndarray | None = None
    map_counts: np.ndarray | None = None
    pivot_labels: np.ndarray | None = None

    def allocation_counts(self) -> np.ndarray:
        """q×(K_p + 1) uint32: the samples in which each new observation's draw goes to each of the pivot's clusters (column
        k >= 1: pivot_labels[k - 1]; column 0: a cluster of its own or one the pivot has no counterpart for).  Every row sums
        to m.  Needs a prediction made by predict_points with a relabelling."""
        if self.counts is None:
            raise ValueError("this prediction holds no counts: use predict_points with a relabelling")
        return self.counts

    def probabilities(self) -> np.ndarray:
        """allocation_counts() / m: what allocation(relabelling, samples) returns, without the m×q labels."""
        c = self.allocation_counts()
        return c / float(c[0].sum())

    def hard_allocation(self) -> np.ndarray:
        """Per new observation the pivot label of largest count, the smaller column on a tie; 0 is possible."""
        c = self.allocation_counts()
        return np.concatenate([[0], self.pivot_labels]).astype(np.int64)[np.argmax(c, axis=1)]

    def new_cluster_frequency(self) -> np.ndarray:
        """Per new point: the share of samples in which it opened a cluster of its own."""
        return (self.labels == 0).mean(axis=0)

    def extended_samples(self, samples) -> np.ndarray:
        """The m×(n+q) label matrix of training and new points together.  Within a sample the a-th new point that drew 0
        gets the a-th smallest positive label the sample does not use, so independent singletons stay distinct; every
        label lies in 1..n+q, and posterior_counts, searchpointestimate, hclustpointestimate take the matrix as it is."""
        S = _label_matrix(samples)
        m, q = self.labels.shape
        if S.shape[0] != m:
            raise ValueError(f"samples must be the {m} samples of the prediction")
        n = S.shape[1]
        out = np.empty((m, n + q), np.int64)
        out[:, :n] = S
        out[:, n:] = self.labels
        every = np.arange(1, n + q + 1)
        for s in range(m):
            own = np.flatnonzero(self.labels[s] == 0)
            if len(own):
                out[s, n + own] = np.setdiff1d(every, S[s], assume_unique=False)[:len(own)]
        return out

    def allocation(self, relabelling, samples) -> np.ndarray:
        """q×(K_p + 1): the share of samples in which each new observation goes to each of the pivot's clusters, through a
        Relabelling of the same samples (pointestimate.relabel): the label a new point drew under sample s is one of that
        sample's names, its rank among them the column of relabelling.maps[s] that says which pivot cluster it became.
        Columns as relabelling.counts: column k >= 1 is the pivot's cluster pivot_labels[k - 1]; column 0 is a cluster of
        its own (label 0) or a cluster of the sample that the pivot has no counterpart for.  Every row sums to 1."""
        return _allocation(self.labels, relabelling, samples, unknown_raises=True)


@dataclass
class JointPrediction:
    """labels[s, i]: the label of new point i under sample s after the last pass, in that sample's own label names; a cluster
    that new points opened carries a label of 1..n+q that the sample did not use (there is no 0).  first_labels: the labels
    after pass 0, the sequential allocation.  K[s]: clusters of the extended sample.  moves[s, pass]: the visits of the pass
    whose draw differs from the point's previous label (pass 0 gives q).  kernel_ms: device time of the kernels."""
    labels: np.ndarray
    first_labels: np.ndarray
    K: np.ndarray
    moves: np.ndarray
    kernel_ms: float = 0.0

    def extended_samples(self, samples) -> np.ndarray:
        """The m×(n+q) label matrix of training and new points together: a plain concatenation, because the labels are
        already names in 1..n+q that are distinct where the clusters are.  posterior_counts, searchpointestimate,
        hclustpointestimate, relabel and credibleball take the matrix as it is."""
        S = _label_matrix(samples)
        if S.shape[0] != self.labels.shape[0]:
            raise ValueError(f"samples must be the {self.labels.shape[0]} samples of the prediction")
        return np.concatenate([S, self.labels], axis=1)

    def new_cluster_frequency(self, samples) -> np.ndarray:
        """Per new point: the share of samples in which its cluster holds no training point."""
        S = _label_matrix(samples)
        if S.shape[0] != self.labels.shape[0]:
            raise ValueError(f"samples must be the {self.labels.shape[0]} samples of the prediction")
        return np.stack([~np.isin(lab, z) for lab, z in zip(self.labels, S)]).mean(axis=0)

    def allocation(self, relabelling, samples) -> np.ndarray:
        """As Prediction.allocation, except that a label that is not one of the sample's training names (a cluster that new
        points opened) counts in column 0."""
        return _allocation(self.labels, relabelling, samples, unknown_raises=False)


def _allocation(labels, relabelling, samples, unknown_raises: bool) -> np.ndarray:
    """Prediction.allocation and JointPrediction.allocation: label 0 always counts in column 0; a positive label that is not a
    name of the sample raises or counts there too."""
    S = _label_matrix(samples)
    m, q = labels.shape
    if S.shape[0] != m or relabelling.maps.shape[0] != m:
        raise ValueError(f"samples and the relabelling must be of the {m} samples of the prediction")
    names = np.asarray(relabelling.pivot_labels, dtype=np.int64)
    counts = np.zeros((q, len(names) + 1), np.int64)
    for s in range(m):
        own = np.unique(S[s])
        lab = labels[s]
        t = np.searchsorted(own, lab)
        known = (lab > 0) & (t < len(own))
        known &= own[np.minimum(t, len(own) - 1)] == lab
        if unknown_raises and not np.all(known | (lab == 0)):
            raise ValueError(f"a label of the prediction is not a label of sample {s + 1}")
        to = np.where(known, relabelling.maps[s][np.where(known, t, 0)], 0)
        col = np.where(to > 0, np.searchsorted(names, np.maximum(to, 1)) + 1, 0)
        counts[np.arange(q), col] += 1
    return counts / float(m)


def _label_matrix(samples) -> np.ndarray:
    clusts = samples.clusts if hasattr(samples, "clusts") else samples
    if len(clusts) == 0:
        raise ValueError("no samples")
    S = np.asarray(clusts if isinstance(clusts, np.ndarray) else np.stack([np.asarray(c) for c in clusts]))
    if S.ndim != 2 or not np.issubdtype(S.dtype, np.integer):
        raise ValueError("samples must be an m×n matrix of integer labels")
    S = np.ascontiguousarray(S, dtype=np.int64)
    if S.shape[1] < 1 or S.min() < 1 or S.max() > S.shape[1]:
        raise ValueError("sample labels must lie in 1..n")
    return S


def _params_dict(params) -> dict:
    P = params.as_dict() if hasattr(params, "as_dict") else dict(params)
    for k in ("delta1", "delta2", "alpha", "beta", "zeta", "gamma"):
        if k not in P or not float(P[k]) > 0:
            raise ValueError(f"params: {k} must be given and positive")
    if int(P.get("maxK", 0)) < 0:
        raise ValueError("params: maxK must be >= 0")
    return P


def _sample_inputs(result_or_samples, r, p, params):
    """(S, r, p, P) of an MCMCResult or of a label matrix with r, p and params given, checked"""
    S = _label_matrix(result_or_samples)
    m = S.shape[0]
    res = result_or_samples
    r = getattr(res, "r", None) if r is None else r
    p = getattr(res, "p", None) if p is None else p
    params = getattr(res, "params", None) if params is None else params
    if r is None or p is None or params is None:
        raise ValueError("r, p and params are needed with a plain label matrix")
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
    if r.shape != (m,) or p.shape != (m,):
        raise ValueError(f"r and p must hold one value per sample ({m})")
    if not (np.all(np.isfinite(r)) and np.all(r > 0)):
        raise ValueError("r must be positive and finite")
    if not (np.all(p > 0) and np.all(p < 1)):
        raise ValueError("p must lie in (0, 1)")
    return S, r, p, _params_dict(params)


def _dim(points):
    """the number of coordinates of points given as rows, None when they are not (their own check says so)"""
    return int(np.shape(points)[1]) if points is not None and np.ndim(points) == 2 else None


def _host_distances(Y, X, metric):
    """the host's q×n distances: the Euclidean ones as they always were here, the other metrics by metrics.host_pairwise"""
    if metric == "euclidean":
        return np.sqrt(((Y[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    from .metrics import host_pairwise
    return host_pairwise(Y, X, metric)


def predict(result_or_samples, Dnew=None, *, new_points=None, points=None, r=None, p=None, params=None, seed: int = 0,
            scores: bool = False, device: int = 0, metric: str = "euclidean") -> Prediction:
    """Allocate new observations to the clusters of every posterior sample.

    result_or_samples: an MCMCResult (its clusts, r, p and params are used) or an m×n label matrix with r, p (one per
    sample) and params (a PriorHyperparamsList or a dict of the likelihood hyperparameters) given.  The new data: Dnew
    (q×n, distances of every new observation to every training observation) or new_points with the training points, one
    observation per row — the distances are then computed on the host in row chunks, so q×n never exists at once; every new
    point is quantised by itself and keyed by its own index, so the chunked result equals the unchunked one.  For many new
    points given by coordinates use predict_points, which takes the distances and their logarithms on the device.  metric (with
    new_points; a name of METRICS): the distance the host evaluates, the one the training matrix was made in."""
    _lib.check_metric(metric, _dim(points))
    S, r, p, P = _sample_inputs(result_or_samples, r, p, params)
    m, n = S.shape
    if (Dnew is None) == (new_points is None):
        raise ValueError("give either Dnew or new_points (with points)")
    Kmax = int(max(len(np.unique(row)) for row in S)) if scores else 0
    if Dnew is not None:
        if points is not None:
            raise ValueError("points goes with new_points, not with Dnew")
        Dnew = np.ascontiguousarray(Dnew, dtype=np.float64)
        if Dnew.ndim != 2 or Dnew.shape[1] != n or Dnew.shape[0] < 1:
            raise ValueError(f"Dnew must be a q×n matrix with n = {n} columns and q >= 1")
        if not (np.all(np.isfinite(Dnew)) and np.all(Dnew > 0)):
            raise ValueError("Dnew must be finite and positive")
        out = _lib.predict(Dnew, S, r, p, P, seed=seed, Kmax=Kmax, want_scores=scores, device=device)
        return Prediction(out["labels"], out["map"], out.get("scores"), out["kernel_ms"])
    if points is None:
        raise ValueError("new_points needs the training points")
    X = np.ascontiguousarray(points, dtype=np.float64)
    Y = np.ascontiguousarray(new_points, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != n:
        raise ValueError(f"points must hold the n = {n} training observations, one per row")
    if Y.ndim != 2 or Y.shape[1] != X.shape[1] or Y.shape[0] < 1:
        raise ValueError("new_points must hold q >= 1 observations of the training points' dimension, one per row")
    if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))):
        raise ValueError("points must be finite")
    q = Y.shape[0]
    step = max(1, _DIST_CHUNK_BYTES // (8 * n * max(X.shape[1], 1)))
    labels, maps = np.empty((m, q), np.int64), np.empty((m, q), np.int64)
    sc = np.empty((m, q, Kmax + 1)) if scores else None
    ms = 0.0
    for i0 in range(0, q, step):
        Yc = Y[i0:i0 + step]
        Dc = _host_distances(Yc, X, metric)
        if not np.all(Dc > 0):
            raise ValueError("a new point coincides with a training point: the distances must be positive" if metric == "euclidean" else
                             f"a {metric} distance of a new point to a training point is not positive (coincident or parallel points, "
                             "a zero or constant vector): the distances must be positive")
        out = _lib.predict(Dc, S, r, p, P, seed=seed, point_offset=i0, Kmax=Kmax, want_scores=scores, device=device)
        labels[:, i0:i0 + step], maps[:, i0:i0 + step] = out["labels"], out["map"]
        if scores:
            sc[:, i0:i0 + step] = out["scores"]
        ms += out["kernel_ms"]
    return Prediction(labels, maps, sc, ms)


def predict_points(result_or_samples, points, new_points, *, relabelling=None, keep_labels=None, r=None, p=None, params=None,
                   seed: int = 0, scores: bool = False, device: int = 0, metric: str = "euclidean") -> Prediction:
    """Allocate any number of new observations, given by their coordinates, to the clusters of every posterior sample
    (rc_predict_points): the distances to the n training points (one observation per row of `points`), their logarithms, the
    quantisation and the draws never leave the device, and the samples are uploaded once.  The distance is the Euclidean one,
    accumulated coordinate by coordinate with fused multiply-adds (include/redclust_hip.h has the exact arithmetic), so the
    labels are those of predict on those distances with the device's logarithm — not bit for bit those of
    predict(new_points=…, points=…), whose distances and logarithms are NumPy's and libm's.

    result_or_samples, r, p, params, seed, scores as for predict.  relabelling (pointestimate.relabel of the same samples onto
    a point estimate): the prediction then carries counts and map_counts, q×(K_p+1), per new observation the number of samples
    in which it lands in each of the pivot's clusters — Prediction.allocation without the m×q labels.  keep_labels (default:
    relabelling is None): whether labels and map_labels come back; without them only the counts cross the bus, which is what
    makes q in the millions practical.  scores needs keep_labels.  metric (a name of METRICS): the distance, in the arithmetic
    the header states for it — use the one the training matrix was made in (MCMCData(points, metric=...)); the default is the
    Euclidean call as before (rc_predict_points), any other name goes through rc_predict_points_metric."""
    _lib.check_metric(metric, _dim(points))
    S, r, p, P = _sample_inputs(result_or_samples, r, p, params)
    m, n = S.shape
    keep = (relabelling is None) if keep_labels is None else bool(keep_labels)
    if not keep and relabelling is None:
        raise ValueError("keep_labels=False needs a relabelling: nothing would come back")
    if scores and not keep:
        raise ValueError("scores come with the labels: keep_labels must be true")
    X = np.ascontiguousarray(points, dtype=np.float64)
    Y = np.ascontiguousarray(new_points, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != n or X.shape[1] < 1:
        raise ValueError(f"points must hold the n = {n} training observations, one per row")
    if Y.ndim != 2 or Y.shape[1] != X.shape[1] or Y.shape[0] < 1:
        raise ValueError("new_points must hold q >= 1 observations of the training points' dimension, one per row")
    if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))):
        raise ValueError("points must be finite")
    maps = names = cols = None
    if relabelling is not None:
        names = np.asarray(relabelling.pivot_labels, dtype=np.int64).reshape(-1)
        maps = np.asarray(relabelling.maps)
        if maps.ndim != 2 or maps.shape[0] != m:
            raise ValueError(f"the relabelling must be of the {m} samples")
        if len(names) < 1 or np.any(np.diff(names) <= 0):
            raise ValueError("the relabelling's pivot_labels must be ascending")
        at = np.searchsorted(names, np.maximum(maps, 1))
        if not np.all((maps <= 0) | (names[np.minimum(at, len(names) - 1)] == maps)):
            raise ValueError("the relabelling's maps must hold pivot labels")
        # the library wants pivot labels in 1..n; a pivot may carry any names: pass the columns 1..K_p instead
        maps = np.where(maps > 0, at + 1, maps).astype(np.int64)
        cols = np.arange(1, len(names) + 1, dtype=np.int64)
    Kmax = int(max(len(np.unique(row)) for row in S)) if scores else 0
    out = _lib.predict_points(X, Y, S, r, p, P, seed=seed, want_labels=keep, want_map=keep, maps=maps, pivot_labels=cols,
                              want_counts=maps is not None, want_mapcounts=maps is not None, Kmax=Kmax, want_scores=scores,
                              device=device, **({} if metric == "euclidean" else dict(metric=metric)))
    return Prediction(out["labels"], out["map"], out.get("scores"), out["kernel_ms"], out["counts"], out["mapcounts"], names)


def predict_joint(result_or_samples, Dnew=None, Dnn=None, *, new_points=None, points=None, sweeps: int = 2, r=None, p=None,
                  params=None, seed: int = 0, device: int = 0, metric: str = "euclidean") -> JointPrediction:
    """Allocate new observations to the clusters of every posterior sample jointly: under every sample the new observations
    are allocated one after the other in the order given, each seeing the training labels and the new observations before
    it, and then visited again in `sweeps` Gibbs passes with every other new observation allocated — so a group that the
    training data missed ends up as one new cluster instead of as many singletons as it has members.

    result_or_samples, r, p, params as for predict.  The new data: Dnew (q×n, new to training observations) with Dnn (q×q,
    symmetric, distances among the new observations; the diagonal is ignored), or new_points with the training points, one
    observation per row — both blocks are then computed on the host.  A sample's clusters and the new observations must fit
    4096 slots together (K_s + q <= 4096); allocate more observations in blocks, each block's extended_samples being the
    next block's training samples (with its Dnew extended by the earlier blocks).  metric (with new_points; a name of METRICS):
    the distance the host evaluates for both blocks."""
    _lib.check_metric(metric, _dim(points))
    S, r, p, P = _sample_inputs(result_or_samples, r, p, params)
    m, n = S.shape
    if int(sweeps) != sweeps or sweeps < 0:
        raise ValueError("sweeps must be an integer >= 0")
    if (Dnew is None) == (new_points is None):
        raise ValueError("give either Dnew with Dnn or new_points (with points)")
    if Dnew is not None:
        if points is not None:
            raise ValueError("points goes with new_points, not with Dnew")
        if Dnn is None:
            raise ValueError("Dnew needs Dnn, the distances among the new observations")
        Dnew = np.ascontiguousarray(Dnew, dtype=np.float64)
        if Dnew.ndim != 2 or Dnew.shape[1] != n or Dnew.shape[0] < 1:
            raise ValueError(f"Dnew must be a q×n matrix with n = {n} columns and q >= 1")
        if not (np.all(np.isfinite(Dnew)) and np.all(Dnew > 0)):
            raise ValueError("Dnew must be finite and positive")
        Dnn = np.ascontiguousarray(Dnn, dtype=np.float64)
        q = Dnew.shape[0]
        if Dnn.shape != (q, q):
            raise ValueError(f"Dnn must be a q×q matrix with q = {q}")
        off = ~np.eye(q, dtype=bool)
        if not (np.all(np.isfinite(Dnn[off])) and np.all(Dnn[off] > 0)):
            raise ValueError("Dnn must be finite and positive off the diagonal")
        if not np.array_equal(Dnn[off], Dnn.T[off]):
            raise ValueError("Dnn must be symmetric")
    else:
        if Dnn is not None:
            raise ValueError("Dnn goes with Dnew, not with new_points")
        if points is None:
            raise ValueError("new_points needs the training points")
        X = np.ascontiguousarray(points, dtype=np.float64)
        Y = np.ascontiguousarray(new_points, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] != n:
            raise ValueError(f"points must hold the n = {n} training observations, one per row")
        if Y.ndim != 2 or Y.shape[1] != X.shape[1] or Y.shape[0] < 1:
            raise ValueError("new_points must hold q >= 1 observations of the training points' dimension, one per row")
        if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))):
            raise ValueError("points must be finite")
        q = Y.shape[0]
        Dnew, Dnn = _host_distances(Y, X, metric), _host_distances(Y, Y, metric)
        if not np.all(Dnew > 0):
            raise ValueError("a new point coincides with a training point: the distances must be positive")
        if not np.all(Dnn[~np.eye(q, dtype=bool)] > 0):
            raise ValueError("two new points coincide: the distances must be positive")
    out = _lib.predict_joint(Dnew, Dnn, S, r, p, P, sweeps=int(sweeps), seed=seed, device=device)
    return JointPrediction(out["labels"], out["first"], out["K"], out["moves"], out["kernel_ms"])
