"""Cluster profiles on the GPU (csrc/profile.inc.hip through rc_cluster_profiles; include/redclust_hip.h has the contract,
DESIGN.md §8 "Cluster profiles" the design): what describes the clusters of a labelling in terms of the data when the model has
no cluster parameters to print — the medoid (exemplar) of every cluster, every point's silhouette width and every point's
neighbour cluster, the best alternative to its own — for any batch of labellings: point estimates, dendrogram cuts, the
samples of a chain.

The device returns exact integers of Dq = D·2^eD, the diagonal never counted.  With the clusters of a labelling in ascending
label order, sizes n_k, and A(i) the cluster of point i:
    within[i]  = Σ_{j in A(i), j != i} Dq[i][j]
    nearest[i] = Σ_{j in t} Dq[i][j] for the neighbour cluster t != A(i): the one of least mean distance to i, means compared
                 exactly as cross-products, ties to the smaller label; neighbour[i] is its label; both 0 with one cluster
    medoid of a cluster: its member of least within, ties to the smallest point index (reported 1-based).
The silhouette (Rousseeuw 1987) is float64 arithmetic on those, here on the host:
    ā = within/(n_A − 1),  b̄ = nearest/n_neighbour,  s = (b̄ − ā)/max(ā, b̄),
and s = 0 for a singleton, for one cluster and when max(ā, b̄) = 0.  The scale 2^-eD cancels.  There is no CPU fallback for
the device pass."""
from __future__ import annotations

import numpy as np

from .score import _context, _labellings


def _sizes_of(labels_row, neighbour_row, n):
    """(size of every point's own cluster, size of its neighbour cluster — 0 where there is none)"""
    cnt = np.bincount(labels_row, minlength=n + 1)
    nb = cnt[neighbour_row]
    return cnt[labels_row], np.where(neighbour_row > 0, nb, 0)


def silhouettes_from_sums(within, nearest, neighbour, labels) -> np.ndarray:
    """The silhouette widths of L labellings (or of one) from what rc_cluster_profiles returns, host only, float64:
    s = (b̄ − ā)/max(ā, b̄) with ā = within/(n_A − 1) and b̄ = nearest/n_neighbour, the sizes counted from labels; 0 for a
    singleton, where neighbour is 0 (one cluster) and where max(ā, b̄) = 0.  All four arguments have the shape of labels."""
    lab = np.asarray(labels)
    one = lab.ndim == 1
    lab, w, b, nb = (np.atleast_2d(np.asarray(x)) for x in (lab, within, nearest, neighbour))
    if not (lab.shape == w.shape == b.shape == nb.shape) or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError("within, nearest, neighbour and labels must have one shape, the labels integer")
    L, n = lab.shape
    out = np.zeros((L, n))
    for l in range(L):
        own, other = _sizes_of(lab[l].astype(np.int64), nb[l].astype(np.int64), n)
        ok = (own > 1) & (other > 0)
        a = w[l][ok].astype(np.float64) / (own[ok] - 1)
        bb = b[l][ok].astype(np.float64) / other[ok]
        hi = np.maximum(a, bb)
        s = np.zeros(len(a))
        pos = hi > 0
        s[pos] = (bb[pos] - a[pos]) / hi[pos]
        out[l][ok] = s
    return out[0] if one else out


class ClusterProfiles:
    """The profiles of L labellings of n points (clusterprofiles).  labellings: the L×n labels.  Per labelling l, with its
    clusters in ascending label order: labels[l] (their names), sizes[l], medoids[l] (1-based point indices),
    cluster_silhouette[l] (the mean silhouette of each cluster's points), within_mean[l] (each cluster's mean distance between
    two distinct members, in D's units; 0 for a singleton).  Per point: silhouette (L×n float64), neighbour (L×n labels, 0 with
    one cluster).  mean_silhouette (L): the mean over the points.  raw: the dict of Context.profiles."""

    def __init__(self, labellings, raw):
        self.labellings, self.raw = labellings, raw
        self.labels, self.sizes, self.medoids = raw["labels"], raw["sizes"], raw["medoids"]
        self.neighbour = raw["neighbour"]
        self.silhouette = silhouettes_from_sums(raw["within"], raw["nearest"], raw["neighbour"], labellings)
        self.mean_silhouette = self.silhouette.mean(axis=1)
        scale = np.ldexp(1.0, -raw["eD"])
        self.cluster_silhouette, self.within_mean = [], []
        for l, z in enumerate(labellings):
            ids = np.searchsorted(self.labels[l], z)
            sz = self.sizes[l].astype(np.float64)
            self.cluster_silhouette.append(np.bincount(ids, weights=self.silhouette[l], minlength=len(sz)) / sz)
            tot = np.bincount(ids, weights=raw["within"][l].astype(np.float64), minlength=len(sz))      # every pair twice
            self.within_mean.append(np.where(sz > 1, tot / np.maximum(sz * (sz - 1), 1), 0.0) * scale)

    def __len__(self):
        return len(self.labellings)

    def worst(self, k: int, labelling: int = 0):
        """The k points of lowest silhouette in one labelling, the lowest first (the smaller index on ties): (their 0-based
        indices, their silhouettes, the labels of their neighbour clusters — where they would rather go)."""
        s = self.silhouette[labelling]
        idx = np.argsort(s, kind="stable")[:max(int(k), 0)]
        return idx, s[idx], self.neighbour[labelling][idx]


def clusterprofiles(data, labellings, device: int = 0) -> ClusterProfiles:
    """The medoids, silhouettes and neighbour clusters of every labelling (module docstring).  data: a Context (used as it
    is: its state, layout and counts are untouched; it needs no parameters), an MCMCData or a dissimilarity matrix (a context
    is made for the call).  labellings: one labelling, an L×n label matrix, a list of vectors or an MCMCResult (its clusts)."""
    S = _labellings(labellings)
    ctx, own = _context(data, device)
    try:
        return ClusterProfiles(S, ctx.profiles(S, points=True))
    finally:
        if own:
            ctx.close()


def exemplars(data, samples, device: int = 0) -> dict:
    """The posterior view of the profiles, over the samples of a chain (an MCMCResult or an m×n label matrix): frequency (n:
    how often every point is the medoid of its cluster, a bincount of the medoids of all samples — it sums to Σ K),
    probability (frequency / m), silhouette (n: every point's posterior mean silhouette), mean_silhouette (the posterior mean
    of the samples' mean silhouettes), K (m) and kernel_ms."""
    prof = clusterprofiles(data, samples, device=device)
    m, n = prof.labellings.shape
    freq = np.bincount(np.concatenate(prof.medoids) - 1, minlength=n).astype(np.int64)
    return dict(frequency=freq, probability=freq / m, silhouette=prof.silhouette.mean(axis=0),
                mean_silhouette=float(prof.mean_silhouette.mean()), K=prof.raw["K"], kernel_ms=prof.raw["kernel_ms"])
