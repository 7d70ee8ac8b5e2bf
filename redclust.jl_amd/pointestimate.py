"""Point estimates and clustering comparison — host mirror of /root/reference/src/pointestimate.jl and
src/summaries.jl.  The pairwise loss matrix of the MPEL search and every pair measure are computed on the GPU
(csrc/pointestimate.inc.hip) through the C ABI; there is no CPU fallback."""
from __future__ import annotations

import sys
from dataclasses import dataclass

import numpy as np

from . import _lib

_LOSSES = {"binder": 0, "omARI": 1, "VI": 2, "ID": 3}  # pointestimate.jl:21, 38-47


def _check_lengths(a, b, msg):
    if len(a) != len(b):
        raise ValueError(msg)  # ArgumentError in the reference


def _labels(x):
    """Labels as the reference types them (ClustLabelVector = Vector{Int}); any positive integers are accepted by
    Clustering.jl's counts-based measures, so values above n are compacted first."""
    x = np.asarray(x)
    if x.ndim != 1 or not np.issubdtype(x.dtype, np.integer):
        raise TypeError("cluster labels must be a vector of integers")
    x = x.astype(np.int64)
    if len(x) and (x.min() < 1 or x.max() > len(x)):
        x = np.unique(x, return_inverse=True)[1].astype(np.int64) + 1
    return x


def getpointestimate(samples, method: str = "MAP", loss="VI", device: int = 0):
    """pointestimate.jl:18-60.  Returns (clust, i): a clustering among `samples.clusts` and its sample index —
    1-based as in the reference's return value (samples.clusts[i-1] in Python)."""
    if method == "MPEL" and isinstance(loss, str) and loss not in _LOSSES:
        raise ValueError("Invalid loss function specifier.")
    if method not in ("MAP", "MLE", "MPEL"):
        raise ValueError("Invalid method specifier.")
    if method == "MAP":
        i = int(np.argmax(samples.logposterior))
        return samples.clusts[i], i + 1
    if method == "MLE":
        i = int(np.argmax(samples.loglik))
        return samples.clusts[i], i + 1
    clusts = samples.clusts
    if callable(loss):
        # a user-supplied loss runs where the user's code runs: on the host, pair by pair (pointestimate.jl:36-37,49-58)
        m = len(clusts)
        L = np.zeros((m, m))
        for a in range(m):
            for b in range(a + 1, m):
                L[a, b] = loss(clusts[a], clusts[b])
        L = L + L.T
        i = int(np.argmin(L.sum(axis=0)))
        return clusts[i], i + 1
    S = np.stack([_labels(c) for c in clusts])
    _, _, i, _ = _lib.loss_matrix(S, _LOSSES[loss], device=device, want_matrix=False)
    return clusts[i], i + 1


_PSM_LOSSES = {"binder": 0, "VI": 1}   # RC_PSM_BINDER, RC_PSM_VILB


def cocluster_counts(clusts) -> np.ndarray:
    """Σ_s adjacencymatrix(clusts[s]) (utils.jl:59-63) as exact uint32 counts, on the host."""
    S = np.stack([_labels(c) for c in clusts])
    m, n = S.shape
    counts = np.zeros((n, n), np.uint32)
    for s in range(m):
        onehot = np.zeros((n, int(S[s].max()) + 1), np.float32)
        onehot[np.arange(n), S[s]] = 1.0
        counts += (onehot @ onehot.T).astype(np.uint32)
    return counts


def _sample_matrix(samples) -> np.ndarray:
    """The m×n int64 label matrix of an MCMCResult, anything with `.clusts`, or an m×n label matrix (every sample through
    _labels)."""
    clusts = samples.clusts if hasattr(samples, "clusts") else samples
    if len(clusts) == 0:
        raise ValueError("no samples")
    return np.stack([_labels(c) for c in clusts])


def posterior_counts(samples, device: int = 0) -> np.ndarray:
    """cocluster_counts built on the GPU (csrc/samplecounts.inc.hip): the exact n×n uint32 matrix whose entry (i, j) is the
    number of samples in which i and j share a cluster.  samples: an MCMCResult, anything with `.clusts`, or an m×n label
    matrix — a stored result, several chains' samples stacked, another sampler's draws.  There is no CPU fallback."""
    return _lib.samples_counts(_sample_matrix(samples), device=device)[0]


def posterior_coclustering(samples, device: int = 0) -> np.ndarray:
    """The posterior co-clustering matrix of the samples, posterior_counts / m in f64 (./ numsamples, mcmc.jl:560) — equal
    bit for bit to the `posterior_coclustering` runsampler returns for the same samples."""
    S = _sample_matrix(samples)
    return _lib.samples_counts(S, device=device)[0].astype(np.float64) / float(S.shape[0])


def expectedloss(clust, counts, numsamples: int, loss="VI") -> float:
    """The criterion searchpointestimate minimises, evaluated on the host in NumPy for any labelling `clust`, from the n×n
    co-clustering counts C (C_ii = numsamples = m):
      "binder": [Σ_{i<j} C_ij + Σ_{i<j, c_i=c_j} (m − 2·C_ij)] / (m·n(n−1)/2) — the mean over the samples of
                binderloss(clust, sample; normalised = true) (pointestimate.jl:68-76), exact in integers (0 for n = 1);
      "VI":     (1/n)·Σ_i [log n_{c_i} − 2·log T_i] + 2·log m with T_i = Σ_{j: c_j=c_i} C_ij — Wade & Ghahramani's
                lower bound of the expected VI without its partition-independent constant (natural logs)."""
    if loss not in _PSM_LOSSES:
        raise ValueError("Invalid loss function specifier.")
    c = _labels(clust)
    C = np.asarray(counts)
    n, m = len(c), int(numsamples)
    if C.shape != (n, n):
        raise ValueError("counts must be an n×n matrix matching clust")
    same = c[:, None] == c[None, :]
    Ci = C.astype(np.int64)
    if loss == "binder":
        if n < 2:
            return 0.0
        iu = np.triu_indices(n, 1)
        num = int(Ci[iu].sum()) + int((m - 2 * Ci[iu][same[iu]]).sum())
        return num / (m * (n * (n - 1) // 2))
    T = (Ci * same).sum(axis=1)
    return float(np.sum(np.log(same.sum(axis=1)) - 2.0 * np.log(T))) / n + 2.0 * float(np.log(m))


def expectedvi(clust, samples) -> float:
    """The posterior expected Variation of Information of `clust`: the mean over the samples (an MCMCResult, anything with
    `.clusts`, or an m×n label matrix) of VI(clust, sample) = [φ(n_k) and φ(n_l) summed − 2·Σ_kl φ(N_kl)] / n with
    φ(x) = x·log x, natural logs — what searchpointestimate(exact=True) minimises, in plain NumPy on the host."""
    c = np.unique(_labels(clust), return_inverse=True)[1].astype(np.int64)      # 0..K−1: K·L bins per sample below
    clusts = samples.clusts if hasattr(samples, "clusts") else samples
    n = len(c)
    if len(clusts) == 0:
        raise ValueError("no samples")

    def phi(x):
        x = x[x > 0].astype(np.float64)
        return float(np.sum(x * np.log(x)))

    base = phi(np.bincount(c))
    total = 0.0
    for s in clusts:
        s = np.asarray(s)
        if len(s) != n:
            raise ValueError("every sample must have as many labels as clust")
        s = np.unique(_labels(s), return_inverse=True)[1].astype(np.int64)
        total += base + phi(np.bincount(s)) - 2.0 * phi(np.bincount(c * (int(s.max()) + 1) + s))
    return total / (n * len(clusts))


def expectedid(clust, samples) -> float:
    """The posterior expected information distance of `clust`: the mean over the samples (an MCMCResult, anything with
    `.clusts`, or an m×n label matrix) of infodist(clust, sample; normalised = false) = max(H(c), H(s)) − I(c, s) =
    [max(Σ_k φ(n_k), Σ_l φ(n_l)) − Σ_kl φ(N_kl)] / n with φ(x) = x·log x, natural logs — what searchpointestimate(loss="ID")
    minimises, in plain NumPy on the host.  evaluateclustering's `nid` is this divided by log n."""
    c = np.unique(_labels(clust), return_inverse=True)[1].astype(np.int64)      # 0..K−1: K·L bins per sample below
    clusts = samples.clusts if hasattr(samples, "clusts") else samples
    n = len(c)
    if len(clusts) == 0:
        raise ValueError("no samples")

    def phi(x):
        x = x[x > 0].astype(np.float64)
        return float(np.sum(x * np.log(x)))

    base = phi(np.bincount(c))
    total = 0.0
    for s in clusts:
        s = np.asarray(s)
        if len(s) != n:
            raise ValueError("every sample must have as many labels as clust")
        s = np.unique(_labels(s), return_inverse=True)[1].astype(np.int64)
        total += max(base, phi(np.bincount(s))) - phi(np.bincount(c * (int(s.max()) + 1) + s))
    return total / (n * len(clusts))


def _counts_input(samples_or_counts, numsamples, ctx):
    """The three input forms of searchpointestimate as (samples matrix or None, counts or None, numsamples, n)."""
    if ctx is not None:
        if numsamples is None:
            raise ValueError("numsamples is required with ctx=")
        return None, None, int(numsamples), ctx.n
    if hasattr(samples_or_counts, "clusts"):
        S = _sample_matrix(samples_or_counts)
        return S, None, S.shape[0], S.shape[1]
    if samples_or_counts is None:
        raise ValueError("need an MCMCResult, a count matrix or ctx=")
    if numsamples is None:
        raise ValueError("numsamples is required with a count matrix")
    counts = np.asarray(samples_or_counts)
    if counts.ndim != 2 or counts.shape[0] != counts.shape[1] or not np.issubdtype(counts.dtype, np.integer):
        raise ValueError("counts must be a square matrix of integer counts")
    return None, np.ascontiguousarray(counts, dtype=np.uint32), int(numsamples), counts.shape[0]


def _search_starts(n, nruns, seed, init, samples=None, mpel_loss=None, extra=None, device=0):
    """The runs of every search as (inits, orders): nruns Philox orders from empty labels, drawn in run order; one run per init
    labelling; given the samples, one from their MPEL sample under mpel_loss; and one from `extra` if there is one — the last
    three kinds in the identity order.  The count-matrix and ctx forms have neither samples nor extra."""
    inits = [np.zeros(n, np.int64)] * int(nruns)
    rng = np.random.Generator(np.random.Philox(key=int(seed)))
    ident = np.arange(1, n + 1, dtype=np.int32)
    orders = [rng.permutation(n).astype(np.int32) + 1 for _ in range(int(nruns))]
    for lab in ([] if init is None else (np.atleast_2d(np.asarray(init)))):
        if len(lab) != n:
            raise ValueError("every labelling in init must have n entries")
        inits.append(np.asarray(lab, np.int64))
    if samples is not None:
        inits.append(_labels(getpointestimate(samples, "MPEL", mpel_loss, device=device)[0]))
    if extra is not None:
        inits.append(extra)
    if not inits:
        raise ValueError("no run: nruns = 0 and no init")
    return np.stack(inits), np.stack(orders + [ident] * (len(inits) - len(orders)))


_INFO_KEYS = ("loss", "sweeps", "converged", "moves", "K", "labels", "best", "kernel_ms", "loss_num")


def _exact_search(samples, loss, nruns, maxK, maxsweeps, seed, init, device):
    """searchpointestimate(loss="VI", exact=True) and searchpointestimate(loss="ID"): see there.  Two things differ: the
    library's search, and the call whose result is the last start — the bound's search for VI, the exact VI search for ID —
    with the key its info is kept under."""
    search, key = (_lib.id_search, "vi") if loss == "ID" else (_lib.vi_search, "lower_bound")
    S = _sample_matrix(samples)
    start, prior = searchpointestimate(samples, "VI", nruns=nruns, maxK=maxK, maxsweeps=maxsweeps, seed=seed, init=init, device=device,
                                       exact=loss == "ID")
    inits, orders = _search_starts(S.shape[1], nruns, seed, init, samples, loss, start, device)
    if not maxK:
        # the library's default cap is the samples' largest cluster count, which a start with more clusters widens
        lmax = max(len(np.unique(s)) for s in S)
        need = max(len(np.unique(x[x > 0])) for x in inits)
        maxK = need if need > lmax else 0
    res = search(S, inits, orders, maxK=maxK, maxsweeps=maxsweeps, device=device)
    info = {k: res[k] for k in _INFO_KEYS}
    info[key] = prior
    return res["labels"][res["best"]].copy(), info


def searchpointestimate(samples_or_counts=None, loss="VI", *, nruns: int = 16, maxK: int = 0, maxsweeps: int = 100,
                        seed: int = 0, init=None, numsamples=None, ctx=None, device: int = 0, exact: bool = False):
    """Search ALL partitions for the clustering of minimum expected loss under the posterior co-clustering counts (the
    reference's docs send its users to R's SALSO for this; getpointestimate(method="MPEL") only looks at the sampled
    clusterings).  Runs on the GPU (csrc/pointsearch.inc.hip), every run one workgroup; there is no CPU fallback.

    samples_or_counts: an MCMCResult (its counts are rebuilt exactly from `clusts` on the device and stay there:
    rc_psm_search_samples; info["counts_ms"] is that kernel's time), or an n×n uint32 count matrix together
    with numsamples; or pass a live Context as ctx= (with numsamples): its device counts are searched in place.
    loss: "binder", "VI" — see expectedloss; "VI" is the lower bound, not the exact posterior expected VI — or "ID", below.  When the
    samples are given, the partition-independent constant (1/n)·Σ_i mean_s log n^(s)_{c_i} that turns the bound's value into
    Wade & Ghahramani's is returned as info["vi_constant"]; the losses themselves leave it out.
    Runs: nruns runs from empty labels (sequential allocation, then improving sweeps) in the orders
    np.random.Generator(np.random.Philox(key=seed)).permutation(n), drawn in run order; one more run per labelling in init
    (identity order); and, for an MCMCResult, one run started at getpointestimate(samples, "MPEL", loss), so that the result is
    never worse under the searched criterion than that sample.  maxK: cap on the number of clusters (0 = none).
    Returns (clust, info): the best labelling (sortlabels'd) and a dict with the per-run loss, sweeps, converged, moves, K,
    all labellings (labels), best (index of the first minimal run), kernel_ms.

    exact=True (loss="VI" and an MCMCResult, or anything with `.clusts`, only): minimise the posterior expected VI itself
    (expectedvi; SALSO's "VI") instead of its lower bound — csrc/visearch.inc.hip, in fixed point, so a run is an exact
    integer function of its inputs.  Runs: the same nruns Philox orders from empty labels, one per init labelling, one from the
    MPEL VI sample and one from the result of the same call with exact=False (info["lower_bound"] is that call's info), so the
    result is never worse than either in the searched integer criterion info["loss_num"] (runs, and the choice of best, are
    exact in it).  info["loss"] is the expected VI as the library returns it, (Q + constant)/(2^32·n·m): within
    2·2^-32 ≈ 4.7e-10 of expectedvi's f64 value, so allow that much when comparing it with expectedvi of another labelling.
    Besides the search the call costs the exact=False search (with its counts kernel) and the MPEL loss matrix.  maxK = 0 caps the clusters at the largest cluster count among the samples (or a start's, if larger).

    loss="ID" (an MCMCResult, or anything with `.clusts`, only; `exact` may be either value, there is no bound variant):
    minimise the posterior expected information distance (expectedid; the `id` of evaluateclustering, SALSO's "ID") — the
    same kernel and fixed point as exact=True (rc_id_search), so a run is again an exact integer function of its inputs.
    Runs: the nruns Philox orders from empty labels, one per init labelling, one from the MPEL ID sample and one from the
    result of searchpointestimate(samples, "VI", exact=True) with the same arguments (info["vi"] is that call's info), so the
    result is never worse in the integer criterion info["loss_num"] than either.  info["loss"] = Q_ID/(2^32·n·m) is within
    2^-32 ≈ 2.3e-10 of expectedid's f64 value.  maxK = 0 is widened as for exact=True."""
    if loss == "ID":
        if ctx is not None:
            raise ValueError('loss="ID" needs the samples; a Context keeps only their counts')
        if not hasattr(samples_or_counts, "clusts"):
            raise ValueError('loss="ID" needs the samples (an MCMCResult), not a count matrix')
        return _exact_search(samples_or_counts, "ID", nruns, maxK, maxsweeps, seed, init, device)
    if loss not in _PSM_LOSSES:
        raise ValueError("Invalid loss function specifier.")
    if exact:
        if loss != "VI":
            raise ValueError('exact=True needs loss="VI"')
        if ctx is not None:
            raise ValueError("exact=True needs the samples; a Context keeps only their counts")
        if not hasattr(samples_or_counts, "clusts"):
            raise ValueError("exact=True needs the samples (an MCMCResult), not a count matrix")
        return _exact_search(samples_or_counts, "VI", nruns, maxK, maxsweeps, seed, init, device)
    S, counts, numsamples, n = _counts_input(samples_or_counts, numsamples, ctx)
    samples = None if S is None else samples_or_counts                  # the counts are built from S on the device
    inits, orders = _search_starts(n, nruns, seed, init, samples, "binder" if loss == "binder" else "VI", device=device)
    if samples is not None:
        res = _lib.psm_search_samples(S, _PSM_LOSSES[loss], inits, orders, maxK=maxK, maxsweeps=maxsweeps, device=device)
    else:
        res = _lib.psm_search(counts, numsamples, _PSM_LOSSES[loss], inits, orders, maxK=maxK, maxsweeps=maxsweeps, device=device, ctx=ctx)
    info = {k: res[k] for k in _INFO_KEYS}
    if samples is not None:
        info["counts_ms"] = res["counts_ms"]
        if loss == "VI":
            sizes = np.stack([np.bincount(s, minlength=n + 1)[s] for s in S])
            info["vi_constant"] = float(np.mean(np.log(sizes)))
    return res["labels"][res["best"]].copy(), info


_LINKAGES = {"average": 0, "complete": 1, "single": 2}   # RC_HCLUST_AVERAGE, _COMPLETE, _SINGLE


def linkage_matrix(merges, numsamples: int, linkage: str = "average") -> np.ndarray:
    """SciPy's (n−1)×4 linkage matrix of a merge sequence of hclust: SciPy's node numbering (leaves 0..n−1, step t makes
    node n + t; the smaller id first), height = 1 − similarity/m (similarity: S_ab/(|a|·|b|) for average, M_ab otherwise),
    size of the new cluster.  Host only."""
    if linkage not in _LINKAGES:
        raise ValueError("Invalid linkage specifier.")
    n = len(merges) + 1
    Z = np.zeros((n - 1, 4))
    node, size = np.arange(n + 1), np.ones(n + 1, np.int64)           # by cluster name (1-based)
    for t, g in enumerate(merges):
        a, b = int(g["a"]), int(g["b"])
        sim = int(g["s_ab"]) / (int(size[a]) * int(size[b])) if linkage == "average" else int(g["m_ab"])
        Z[t] = (min(node[a], node[b]) - 1, max(node[a], node[b]) - 1, 1.0 - sim / int(numsamples), int(g["size"]))
        node[a], size[a] = n + t + 1, int(g["size"])
    return Z


def leaf_order(Z) -> np.ndarray:
    """The leaves of a linkage matrix from left to right (first child first) — scipy.cluster.hierarchy.leaves_list's order,
    the one co-clustering heatmaps are drawn in.  0-based."""
    n = len(Z) + 1
    out, stack = [], [2 * n - 2] if n > 1 else [0]
    while stack:
        v = stack.pop()
        if v < n:
            out.append(v)
        else:
            stack += [int(Z[v - n, 1]), int(Z[v - n, 0])]
    return np.array(out, np.int64)


def hclust(samples_or_counts=None, linkage="average", *, numsamples=None, ctx=None, device: int = 0):
    """Agglomerative clustering of the posterior co-clustering counts on the GPU (csrc/hclust.inc.hip): the classical
    hierarchical point estimate's dendrogram (Medvedovic; mcclust's minbinder / mcclust.ext's minVI with method "avg" /
    "comp").  Input forms as searchpointestimate: an MCMCResult (the counts are built on the device and stay there), an n×n
    count matrix with numsamples, or ctx= with numsamples.  linkage: "average", "complete" or "single", on similarities —
    the pair of largest average / minimum / maximum count merges first; ties go to the smallest cluster name (smallest
    member), then the smallest partner; everything is exact integer arithmetic, so a run is reproducible bit for bit.
    Returns a dict: merges (records a, b, size, m_ab, s_ab per step, names 1-based), binder_num (the exact Binder numerator
    of the partition after t merges, t = 0..n−1), Z (linkage_matrix: usable with scipy.cluster.hierarchy.dendrogram),
    order (leaf_order(Z)), kernel_ms.  There is no CPU fallback."""
    if linkage not in _LINKAGES:
        raise ValueError("Invalid linkage specifier.")
    S, counts, m, _ = _counts_input(samples_or_counts, numsamples, ctx)
    res = _lib.hclust(counts, m, _LINKAGES[linkage], device=device, ctx=ctx, samples=S)
    Z = linkage_matrix(res["merges"], m, linkage)
    out = dict(merges=res["merges"], binder_num=res["binder_num"], Z=Z, order=leaf_order(Z), kernel_ms=res["kernel_ms"])
    if "counts_ms" in res:
        out["counts_ms"] = res["counts_ms"]
    return out


def _hclust_cuts(samples_or_counts, linkage, maxK, numsamples, ctx, device, *, lo=1, exact=False, vilb=False, cuts=True):
    """What the criteria of hclustpointestimate share: the linkage and the input checked (exact: the samples only), maxK
    defaulted to ⌈n/8⌉ (at least lo, n permitting) and checked to lie in lo..n, the dendrogram (vilb: with the VI bound of the
    cuts 1..maxK) and, unless cuts=False, the stacked cuts of lo..maxK clusters.  Returns (res, cuts, S, m, n, maxK)."""
    if linkage not in _LINKAGES:
        raise ValueError("Invalid linkage specifier.")
    if exact and ctx is not None:
        raise ValueError("exact=True needs the samples; a Context keeps only their counts")
    if exact and not hasattr(samples_or_counts, "clusts"):
        raise ValueError("exact=True needs the samples (an MCMCResult), not a count matrix")
    S, counts, m, n = _counts_input(samples_or_counts, numsamples, ctx)
    maxK = int(maxK) if maxK else max(-(-n // 8), min(n, lo))
    if not lo <= maxK <= n:
        raise ValueError("maxK must lie in 1..n" if lo == 1 else "maxK must lie in 2..n with criterion='silhouette'")
    res = _lib.hclust(counts, m, _LINKAGES[linkage], maxcut=maxK if vilb else 0, device=device, ctx=ctx, samples=S)
    stacked = np.stack([_lib.hclust_cut(res["merges"], n, K) for K in range(lo, maxK + 1)]) if cuts else None
    return res, stacked, S, m, n, maxK


def hclustpointestimate(samples_or_counts=None, loss="VI", linkage="average", *, maxK: int = 0, numsamples=None, ctx=None,
                        device: int = 0, exact: bool = False, criterion: str = "loss", data=None, params=None, r=None, p=None,
                        polish: bool = False):
    """The hierarchical point estimate: hclust's dendrogram cut at the number of clusters K in 1..maxK of minimum expected
    loss (ties: the smaller K).  loss: "binder" — from the exact curve binder_num — or "VI", the lower bound expectedloss(…,
    "VI") evaluates, computed for every cut on the device.  maxK = 0 means ⌈n/8⌉.  Returns (clust, info): the cut
    (sortlabels'd) and a dict with loss (per K = 1..maxK), K, merges, binder_num, kernel_ms, and loss_num (per K) for
    "binder".  A deterministic start for searchpointestimate(init=[clust]).

    exact=True (samples only: an MCMCResult or anything with `.clusts`): the cut is chosen by the exact posterior expected
    loss of every cut — expecteddistances on the maxK cuts, one call of rc_partition_distances — instead of the VI's lower
    bound; loss may then also be "ID".  info["loss"] and info["loss_num"] (per K; Python integers) are the exact expected
    loss and its integer numerator, and the choice is exact in loss_num.

    criterion="posterior": the cut of highest log-posterior under the model instead of lowest expected loss — mapestimate
    (score.py) over the maxK cuts, one device pass over the matrices of data (a Context, an MCMCData or a dissimilarity
    matrix) with params and r, p (scalars or one per cut; None: the posterior means of an MCMCResult's r and p).  info has K,
    loglik, logprior, logposterior (per K = 1..maxK), merges, binder_num, kernel_ms, score_ms.  polish=True (this criterion
    only; the default is off) passes the chosen cut through searchmapestimate under its r and p — a climb over all partitions
    from the cut and from empty labels; the result is never worse than the cut, and info["polish"] is that search's info.

    criterion="silhouette": the best separated cut — the one of highest mean silhouette width (profiles.py: exact integer
    sums of D on the device, the quotients on the host) among the cuts of 2..maxK clusters (one cluster has silhouette 0 by
    convention and is not a candidate; maxK >= 2), the fewest clusters on a float tie.  One device pass over the matrix of
    data (as above) for all cuts; it needs no params, r or p.  info has K, mean_silhouette (per K = 2..maxK), merges,
    binder_num, kernel_ms, profile_ms."""
    if criterion not in ("loss", "posterior", "silhouette"):
        raise ValueError("criterion must be 'loss', 'posterior' or 'silhouette'")
    if polish and criterion != "posterior":
        raise ValueError("polish=True goes with criterion='posterior'")
    source = (samples_or_counts, linkage, maxK, numsamples, ctx, device)
    if criterion != "loss":
        if exact:
            raise ValueError(f"exact=True chooses by expected loss; it does not go with criterion='{criterion}'")
        if linkage not in _LINKAGES:
            raise ValueError("Invalid linkage specifier.")
        if data is None:
            raise ValueError(f"criterion='{criterion}' needs data= (a Context, an MCMCData or a dissimilarity matrix)")
    if criterion == "silhouette":
        from .profiles import clusterprofiles
        res, cuts, _, _, _, _ = _hclust_cuts(*source, lo=2)
        prof = clusterprofiles(data, cuts, device=device)
        best = int(np.argmax(prof.mean_silhouette))                 # numpy's argmax is the first maximum: the fewest clusters
        info = dict(merges=res["merges"], binder_num=res["binder_num"], kernel_ms=res["kernel_ms"],
                    profile_ms=prof.raw["kernel_ms"], mean_silhouette=prof.mean_silhouette, K=best + 2)
        return cuts[best].copy(), info
    if criterion == "posterior":
        from .score import mapestimate
        if r is None and p is None and hasattr(samples_or_counts, "r"):
            r, p = float(np.mean(samples_or_counts.r)), float(np.mean(samples_or_counts.p))
        if params is None and not isinstance(data, _lib.Context):
            params = getattr(samples_or_counts, "params", None)
        if r is None or p is None:
            raise ValueError("criterion='posterior' needs r and p")
        res, cuts, _, _, _, _ = _hclust_cuts(*source)
        clust, sc = mapestimate(data, cuts, params, r, p, device=device)
        info = dict(merges=res["merges"], binder_num=res["binder_num"], kernel_ms=res["kernel_ms"], score_ms=sc["kernel_ms"],
                    loglik=sc["loglik"], logprior=sc["logprior"], logposterior=sc["logposterior"], K=sc["index"] + 1)
        if polish:
            from .score import searchmapestimate
            rk, pk = (np.broadcast_to(np.asarray(x, dtype=np.float64).reshape(-1), (len(cuts),))[sc["index"]] for x in (r, p))
            clust, info["polish"] = searchmapestimate(data, [clust], params, float(rk), float(pk), nruns=1, device=device)
        return clust, info
    if loss not in (_DIST_LOSSES if exact else _PSM_LOSSES):
        raise ValueError("Invalid loss function specifier.")
    if exact:
        res, cuts, S, _, n, maxK = _hclust_cuts(*source, exact=True)
        dist = _lib.partition_distances(cuts, S, want_sq=loss == "binder", want_phi=loss != "binder", device=device)
        losses, num = _expected_from_parts(dist, loss, n)
        K = min(range(maxK), key=lambda k: (num[k], k)) + 1
        info = dict(merges=res["merges"], binder_num=res["binder_num"], kernel_ms=res["kernel_ms"], counts_ms=res["counts_ms"],
                    distances_ms=dist["kernel_ms"], loss=losses, loss_num=num, K=K)
        return cuts[K - 1].copy(), info
    res, _, _, m, n, maxK = _hclust_cuts(*source, vilb=loss == "VI", cuts=False)    # one cut, for the chosen K
    info = dict(merges=res["merges"], binder_num=res["binder_num"], kernel_ms=res["kernel_ms"])
    if loss == "binder":
        pairs = n * (n - 1) // 2
        info["loss_num"] = res["binder_num"][::-1][:maxK].copy()       # K clusters = n − K merges
        info["loss"] = np.array([int(x) / (m * pairs) if pairs else 0.0 for x in info["loss_num"]])
        K = int(np.argmin(info["loss_num"])) + 1
    else:
        info["loss"] = res["vilb"]
        K = int(np.argmin(info["loss"])) + 1
    info["K"] = K
    return _lib.hclust_cut(res["merges"], n, K), info


def expectedlosses(labellings, counts_or_samples=None, numsamples=None, loss="VI", *, ctx=None, device: int = 0):
    """expectedloss for a batch of labellings (L×n, or one labelling) on the GPU: against an n×n count matrix with numsamples
    (copied to the device once for the batch), against ctx= with numsamples (its device counts, in place, no copy), or against an
    MCMCResult — its counts are built on the device, but come back to the host and go in again as a count matrix: there is no
    samples entry point for this call, so hold the counts (posterior_counts) when evaluating several batches.
    Returns (loss[L], num[L]): num is the exact Binder numerator (0 for "VI")."""
    if loss not in _PSM_LOSSES:
        raise ValueError("Invalid loss function specifier.")
    labs = np.stack([_labels(c) for c in np.atleast_2d(np.asarray(labellings))])
    S, counts, m, n = _counts_input(counts_or_samples, numsamples, ctx)
    if labs.shape[1] != n:
        raise ValueError("every labelling must have n entries")
    if S is not None:
        counts = _lib.samples_counts(S, device=device)[0]
    out_loss, num, _ = _lib.psm_expected_loss(labs, counts, m, _PSM_LOSSES[loss], device=device, ctx=ctx)
    return out_loss, num


def _pear_fraction(X, A, P, m, n):
    """(num, den) of PEAR from X = Σ_{i<j, same cluster} C_ij, A = Σ_k n_k(n_k−1)/2, P = Σ_{i<j} C_ij in Python integers:
    num = 2·(T·X − A·P), den = T·(m·A + P) − 2·A·P with T = n(n−1)/2 (include/redclust_hip.h); (0, 1) where den = 0."""
    X, A, P, m, T = int(X), int(A), int(P), int(m), int(n) * (int(n) - 1) // 2
    den = T * (m * A + P) - 2 * A * P
    return (2 * (T * X - A * P), den) if den else (0, 1)


def _within_pairs(c):
    s = np.bincount(c).astype(np.int64)
    return int((s * (s - 1) // 2).sum())


def pearfraction(clust, counts, numsamples: int):
    """expectedpear's exact value as the pair of Python integers (num, den), den > 0 — compare two labellings with
    fractions.Fraction(num, den), or by cross-multiplication, as searchmaxpear does."""
    c = _labels(clust)
    C = np.asarray(counts)
    n = len(c)
    if C.shape != (n, n):
        raise ValueError("counts must be an n×n matrix matching clust")
    iu = np.triu_indices(n, 1)
    upper = C[iu].astype(np.int64)
    same = (c[:, None] == c[None, :])[iu]
    return _pear_fraction(upper[same].sum(), _within_pairs(c), upper.sum(), numsamples, n)


def expectedpear(clust, counts, numsamples: int) -> float:
    """The posterior expected adjusted Rand index of `clust` in Fritsch & Ickstadt's form (mcclust's pear, SALSO's omARI.approx)
    from the n×n co-clustering counts C (C_ii = numsamples = m): the adjusted Rand index with each sample's pair indicators
    replaced by π_ij = C_ij/m,
        [Σ I_ij·π_ij − Σ I_ij·Σ π_ij / T] / [½(Σ I_ij + Σ π_ij) − Σ I_ij·Σ π_ij / T],  sums over i < j, T = n(n−1)/2,
    evaluated exactly as one ratio of two integers (pearfraction) and divided once; 0 where the denominator is 0 (n = 1, or
    every sample and clust all singletons or all one cluster).  What searchmaxpear maximises.  Host only."""
    num, den = pearfraction(clust, counts, numsamples)
    return num / den


def expectedpears(labellings, counts_or_samples=None, numsamples=None, *, ctx=None, device: int = 0):
    """expectedpear for a batch of labellings (L×n, or one labelling) from the exact Binder numerators the GPU returns
    (rc_psm_expected_loss, as expectedlosses — the input forms are its): a Binder numerator is P + m·A − 2·X, the all-singletons
    labelling (evaluated with the batch) gives P, and A comes from the cluster sizes, so X and with it the fraction follow in
    integers.  Returns (pear[L] f64, num[L], den[L]); num and den are int64 arrays, or object arrays of Python integers where
    a value passes 2^63 (only beyond searchmaxpear's capacity m·T² < 2^62)."""
    labs = np.stack([_labels(c) for c in np.atleast_2d(np.asarray(labellings))])
    S, counts, m, n = _counts_input(counts_or_samples, numsamples, ctx)
    if labs.shape[1] != n:
        raise ValueError("every labelling must have n entries")
    if S is not None:
        counts = _lib.samples_counts(S, device=device)[0]
    singletons = np.arange(1, n + 1, dtype=np.int64)[None, :]
    _, binder, _ = _lib.psm_expected_loss(np.concatenate([labs, singletons]), counts, m, _PSM_LOSSES["binder"], device=device, ctx=ctx)
    return _pears_from_binder(binder[:-1], [_within_pairs(c) for c in labs], binder[-1], m, n)


def _pears_from_binder(binder, within, P, m, n):
    """(pear, num, den) per labelling from its Binder numerator P + m·A − 2·X, its A and P"""
    fr = [_pear_fraction((int(P) + int(m) * A - int(b)) // 2, A, P, m, n) for b, A in zip(binder, within)]
    fits = all(abs(x) < 2 ** 63 for f in fr for x in f)
    num, den = (np.array([f[k] for f in fr], dtype=np.int64 if fits else object) for k in (0, 1))
    return np.array([f[0] / f[1] for f in fr]), num, den


def _first_max_fraction(num, den):
    """index of the first largest num/den (den > 0), compared exactly"""
    best = 0
    for k in range(1, len(num)):
        if int(num[k]) * int(den[best]) > int(num[best]) * int(den[k]):
            best = k
    return best


_PEAR_INFO = ("pear", "num", "den", "sweeps", "converged", "moves", "K", "labels", "best", "kernel_ms")


def _pear_cuts(samples_or_counts, linkage, maxK, numsamples, ctx, device):
    """The cuts of 1..maxK clusters (maxK = 0: ⌈n/8⌉) of hclust's dendrogram and their (pear, num, den), from the exact Binder
    numerators of the dendrogram: binder_num[0] is P.  Returns (cuts, pear, num, den)."""
    res, cuts, _, m, n, maxK = _hclust_cuts(samples_or_counts, linkage, maxK, numsamples, ctx, device)
    binder = res["binder_num"][::-1][:maxK]                             # K clusters = n − K merges
    return (cuts,) + _pears_from_binder(binder, [_within_pairs(c) for c in cuts], res["binder_num"][0], m, n)


def _pear_draws(samples, device):
    """(the samples as a matrix, pear, num, den of every sample)"""
    S = _sample_matrix(samples)
    return (S,) + expectedpears(S, samples, device=device)


def searchmaxpear(samples_or_counts=None, *, nruns: int = 16, maxK: int = 0, maxsweeps: int = 100, seed: int = 0, init=None,
                  numsamples=None, ctx=None, device: int = 0):
    """Search ALL partitions for the clustering of maximum posterior expected adjusted Rand index (expectedpear; mcclust's
    maxpear and SALSO's omARI.approx look for the same optimum) under the posterior co-clustering counts, on the GPU
    (csrc/pointsearch.inc.hip, rc_pear_search*): searchpointestimate's greedy search with the exact fraction as the criterion.
    Every comparison is an exact cross-multiplication of integers, so a run is a pure function of its inputs; there is no CPU
    fallback.  getpointestimate(method="MPEL", loss="omARI") only looks at the sampled clusterings.

    Inputs as searchpointestimate: an MCMCResult (anything with `.clusts`; the counts are built on the device), an n×n count
    matrix with numsamples, or ctx= with numsamples.  Capacity: n <= 8192, m·n < 2^31 and m·T² < 2^62 with T = n(n−1)/2.
    Runs: nruns runs from empty labels in the Philox orders of searchpointestimate; one per labelling in init; given the
    samples, one from the sample of highest PEAR (mcclust's method="draws"); and always one from the average-linkage cut of
    highest PEAR among 1..⌈n/8⌉ clusters (method="avg") — the last three kinds in the identity order, with maxK widened to a
    start's cluster count where that is larger.  So the result is never below any of those starts in the exact fraction.
    Returns (clust, info): the best labelling (sortlabels'd) and a dict with the per-run pear, num, den, sweeps, converged,
    moves, K, all labellings (labels), best (the first run of maximal num/den), kernel_ms, and counts_ms for an MCMCResult."""
    S, counts, m, n = _counts_input(samples_or_counts, numsamples, ctx)
    starts = [] if init is None else list(np.atleast_2d(np.asarray(init)))
    if S is not None:
        _, _, dnum, dden = _pear_draws(samples_or_counts, device)
        starts.append(S[_first_max_fraction(dnum, dden)])
    cuts, _, cnum, cden = _pear_cuts(samples_or_counts, "average", 0, numsamples, ctx, device)
    starts.append(cuts[_first_max_fraction(cnum, cden)])
    inits, orders = _search_starts(n, nruns, seed, starts)
    if maxK:
        maxK = max(int(maxK), max(len(np.unique(x[x > 0])) for x in inits))
    if S is not None:
        res = _lib.pear_search_samples(S, inits, orders, maxK=maxK, maxsweeps=maxsweeps, device=device)
    else:
        res = _lib.pear_search(counts, m, inits, orders, maxK=maxK, maxsweeps=maxsweeps, device=device, ctx=ctx)
    info = {k: res[k] for k in _PEAR_INFO}
    if S is not None:
        info["counts_ms"] = res["counts_ms"]
    return res["labels"][res["best"]].copy(), info


_MAXPEAR_METHODS = ("avg", "comp", "draws", "search")


def maxpear(samples_or_counts=None, method: str = "avg", *, maxK: int = 0, numsamples=None, ctx=None, device: int = 0, **search):
    """mcclust's maxpear: the clustering of highest PEAR (expectedpear) among the candidates of `method` —
      "avg" / "comp":  the cuts of 1..maxK clusters (maxK = 0: ⌈n/8⌉, mcclust's max.k) of hclust's average / complete linkage;
      "draws":         the samples themselves (an MCMCResult or anything with `.clusts` only);
      "search":        searchmaxpear over all partitions (keywords in **search: nruns, maxsweeps, seed, init; maxK is not a cap
                       of the search) — not in mcclust;
      "all":           every method the input admits ("draws" needs the samples); the best of them.
    The PEAR of every cut comes from the exact Binder numerators of the dendrogram and every choice is made on the exact
    fraction, the first maximum winning (the fewest clusters; the earliest sample; for "all" the order above).
    Returns (clust, info): the labelling (sortlabels'd) and a dict with pear, num, den, method (the one that won) and, per
    method that ran, info[method] = dict(pear, num, den, and K / index / the search's info)."""
    if method not in _MAXPEAR_METHODS + ("all",):
        raise ValueError("Invalid method specifier.")
    has_samples = ctx is None and hasattr(samples_or_counts, "clusts")
    if method == "draws" and not has_samples:
        raise ValueError('method="draws" needs the samples (an MCMCResult), not a count matrix')
    if search and method not in ("search", "all"):
        raise ValueError('search keywords go with method="search" or "all"')
    source = dict(numsamples=numsamples, ctx=ctx, device=device)
    found, per = [], {}
    for meth in [x for x in _MAXPEAR_METHODS if method in (x, "all")]:
        if meth in ("avg", "comp"):
            cuts, pear, num, den = _pear_cuts(samples_or_counts, "average" if meth == "avg" else "complete", maxK, numsamples, ctx, device)
            k = _first_max_fraction(num, den)
            clust, per[meth] = cuts[k].copy(), dict(pear=pear, num=num, den=den, K=k + 1)
        elif meth == "draws":
            if not has_samples:
                continue
            S, pear, num, den = _pear_draws(samples_or_counts, device)
            k = _first_max_fraction(num, den)
            clust, per[meth] = _sortlabels(S[k]), dict(pear=pear, num=num, den=den, index=k)
        else:
            clust, sinfo = searchmaxpear(samples_or_counts, **source, **search)
            k = sinfo["best"]
            num, den = sinfo["num"], sinfo["den"]
            per[meth] = dict(pear=sinfo["pear"], num=num, den=den, info=sinfo)
        found.append((meth, clust, int(num[k]), int(den[k])))
    b = _first_max_fraction([f[2] for f in found], [f[3] for f in found])
    meth, clust, num, den = found[b]
    return clust, dict(pear=num / den, num=num, den=den, method=meth, **per)


def _ari_from_sums(sq, lab_sq, smp_sq, n):
    """The L×m adjusted Rand indices (Hubert & Arabie) in f64 from the integer sums sq[l, s] = Σ_kl N_kl², lab_sq[l] = Σ_k n_k²,
    smp_sq[s] = Σ_l n_l²; 0 where the denominator is 0"""
    both = (np.asarray(sq) - n).astype(np.float64) / 2.0                                # Σ_kl C(N_kl, 2)
    a = ((np.asarray(lab_sq) - n).astype(np.float64) / 2.0)[:, None]
    b = ((np.asarray(smp_sq) - n).astype(np.float64) / 2.0)[None, :]
    pairs = n * (n - 1) / 2.0
    chance = a * b / pairs if pairs else np.zeros_like(both)
    den = 0.5 * (a + b) - chance
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0.0, (both - chance) / den, 0.0)


def expectedari(labellings, samples, device: int = 0):
    """The posterior mean of the adjusted Rand index itself — the mean over the samples (an MCMCResult, anything with `.clusts`,
    or an m×n label matrix) of ARI(labelling, sample), Hubert & Arabie's as evaluateclustering's `ari` — for each of L
    labellings (L×n, or one): the quantity PEAR approximates.  The integer sums Σ_kl N_kl² and the marginals Σ n_k², Σ n_l² of
    every pair come from the GPU (rc_partition_distances, as partitiondistances(…, "binder")); the index is formed from them in
    f64 on the host, 0 for a pair whose denominator is 0 (n = 1; both partitions all singletons or all one cluster).
    Returns ari[L]."""
    labs, S = _distance_inputs(labellings, samples)
    dist = _lib.partition_distances(labs, S, want_sq=True, want_phi=False, device=device)
    return _ari_from_sums(dist["sq"], dist["lab_marg"][:, 0], dist["smp_marg"][:, 0], S.shape[1]).mean(axis=1)


_DIST_LOSSES = ("binder", "VI", "ID")


def _numerators(dist, loss):
    """The L×m int64 numerators of a loss from rc_partition_distances' outputs (include/redclust_hip.h): Binder
    (A₂ + B₂ − 2P)/2, VI_q = A_q + B_q − 2T, ID_q = max(A_q, B_q) − T.  Each is below 2^52 (A_q, B_q <= Phiq(n) < n·log n·2^32
    + n with n <= 32767), so int64 holds them with room."""
    A, B = dist["lab_marg"], dist["smp_marg"]
    if loss == "binder":
        return (A[:, 0][:, None] + B[:, 0][None, :] - 2 * dist["sq"]) // 2
    if loss == "VI":
        return A[:, 1][:, None] + B[:, 1][None, :] - 2 * dist["phi"]
    return np.maximum(A[:, 1][:, None], B[:, 1][None, :]) - dist["phi"]


def _denominator(loss, n):
    """What a numerator is divided by: n(n−1)/2 pairs for Binder (normalised as binderloss does it), 2^32·n for VI and ID (nats)."""
    return float(n * (n - 1) // 2) if loss == "binder" else 2.0 ** 32 * n


def _divide(num, den):
    return num / den if den else np.zeros(np.shape(num))                 # Binder at n = 1: no pairs, loss 0


def _expected_from_parts(dist, loss, n):
    """(loss[L] f64, num[L]) from rc_partition_distances' outputs: num = Σ_s numerator, exact.
    Range: a VI numerator is below 2·Phiq(n) <= 2·(n·log n·2^32 + n), so Σ_s stays below 2^63 while m·n·log n < 2^30 — always
    within the exact searches' capacity m·n <= 2^26 (log n < 16), but not for every call this entry accepts (m·n < 2^31).  The
    rows are therefore summed in two 32-bit halves, each of which fits int64 (m < 2^31 terms below 2^32, and terms below
    2^20), and joined as Python integers; num is an int64 array when every sum fits and an object array of Python integers
    otherwise."""
    numer = _numerators(dist, loss)
    m = numer.shape[1]
    lo, hi = (numer & 0xFFFFFFFF).sum(axis=1), (numer >> 32).sum(axis=1)
    sums = [(int(h) << 32) + int(l) for h, l in zip(hi, lo)]
    den = _denominator(loss, n) * m
    losses = np.array([x / den if den else 0.0 for x in sums])
    fits = all(x < 2 ** 63 for x in sums)
    return losses, np.array(sums, dtype=np.int64 if fits else object)


def _distance_inputs(labellings, samples):
    labs = np.stack([_labels(c) for c in np.atleast_2d(np.asarray(labellings))])
    S = _sample_matrix(samples)
    if labs.shape[1] != S.shape[1]:
        raise ValueError("every labelling must have as many labels as the samples")
    return labs, S


def partitiondistances(labellings, samples, loss="VI", device: int = 0):
    """The distance from each of L labellings (L×n, or one labelling) to each of the m samples (an MCMCResult, anything with
    `.clusts`, or an m×n label matrix), on the GPU in exact integers (rc_partition_distances, csrc/partdist.inc.hip); there is
    no CPU fallback.  loss: "binder" — normalised as binderloss does it — or "VI" / "ID" in nats, as varinfo and
    infodist(normalised=False) give them.  Returns (dist, info): dist is L×m f64; info["num"] the L×m int64 numerators dist was
    divided from once (Binder: disagreeing pairs; VI, ID: units of 2^-32/n nats, in the fixed point of the exact searches, so
    equal distances compare equal), info["K_labellings"], info["K_samples"] the cluster counts, info["kernel_ms"]."""
    if loss not in _DIST_LOSSES:
        raise ValueError("Invalid loss function specifier.")
    labs, S = _distance_inputs(labellings, samples)
    dist = _lib.partition_distances(labs, S, want_sq=loss == "binder", want_phi=loss != "binder", device=device)
    num = _numerators(dist, loss)
    info = dict(num=num, K_labellings=dist["lab_marg"][:, 2].copy(), K_samples=dist["smp_marg"][:, 2].copy(), kernel_ms=dist["kernel_ms"])
    return _divide(num, _denominator(loss, S.shape[1])), info


def expecteddistances(labellings, samples, loss="VI", device: int = 0):
    """The posterior expected Binder loss, VI or ID of each of L labellings: the mean over the samples of partitiondistances'
    rows, summed in integers on the host and divided once.  Returns (loss[L], num[L]): num = Σ_s numerator, exact (int64, or
    Python integers in an object array where a sum passes 2^63 — possible only beyond the exact searches' capacity).  For "VI",
    num is rc_vi_search's loss_num plus its constant; expectedvi / expectedid / expectedloss(…, "binder") give the same
    values in f64 on the host, one labelling at a time."""
    if loss not in _DIST_LOSSES:
        raise ValueError("Invalid loss function specifier.")
    labs, S = _distance_inputs(labellings, samples)
    dist = _lib.partition_distances(labs, S, want_sq=loss == "binder", want_phi=loss != "binder", device=device)
    return _expected_from_parts(dist, loss, S.shape[1])


@dataclass
class Relabelling:
    """Posterior samples renamed onto a pivot labelling.  labels[s, j]: the label of point j in sample s in the pivot's names, 0
    where the sample's cluster has no counterpart (only when the sample has more clusters than the pivot).  maps[s, t]: the pivot
    label that the t-th smallest label of sample s is sent to, 0 unmatched, -1 for t >= K_s.  overlap[s]: the points on which
    the renamed sample and the pivot agree.  counts[j, k], k = 0..K_p: the samples in which point j lands in the pivot's cluster
    pivot_labels[k - 1]; column 0 counts unmatched.  kernel_ms: device time of the kernels."""
    labels: np.ndarray
    maps: np.ndarray
    overlap: np.ndarray
    counts: np.ndarray
    pivot_labels: np.ndarray
    kernel_ms: float = 0.0

    def probabilities(self) -> np.ndarray:
        """counts / m, n×(K_p + 1): the share of samples in which each point belongs to each of the pivot's clusters."""
        return self.counts / float(len(self.overlap))

    def allocation(self) -> np.ndarray:
        """Per point the pivot label of largest count, the smaller column on a tie; 0 (unmatched) is possible."""
        return np.concatenate([[0], self.pivot_labels]).astype(np.int64)[np.argmax(self.counts, axis=1)]

    def uncertainty(self) -> np.ndarray:
        """Per point 1 − its largest allocation probability."""
        return 1.0 - self.counts.max(axis=1) / float(len(self.overlap))


def relabel(result_or_samples, pivot, *, device: int = 0) -> Relabelling:
    """Rename every sample (an MCMCResult, anything with `.clusts`, or an m×n label matrix) onto the labelling `pivot` — a point
    estimate, say — on the GPU in exact integers (rc_relabel, csrc/relabel.inc.hip); there is no CPU fallback.  Each sample's
    clusters are matched to the pivot's so that the number of points on which the two agree is largest (a linear assignment on
    their contingency table; among optimal matchings the one the fixed tie rule of DESIGN.md §8 "Relabelling" finds), and
    counts says per point how often it then lands in each of the pivot's clusters."""
    S = _sample_matrix(result_or_samples)
    c = _labels(pivot)
    if c.shape[0] != S.shape[1]:
        raise ValueError("the pivot must have as many labels as the samples")
    out = _lib.relabel(S, c, device=device)
    names = np.unique(np.asarray(pivot).astype(np.int64))
    if not np.array_equal(names, out["pivot_labels"]):              # _labels compacted a pivot with names above n: give them back
        back = np.concatenate([[0], names])
        for key in ("labels", "maps"):
            a = out[key]
            out[key] = np.where(a > 0, back[np.maximum(a, 0)], a)
    return Relabelling(out["labels"], out["maps"], out["overlap"], out["counts"], names, out["kernel_ms"])


def _sortlabels(x):
    """utils.jl:69-74: relabel by order of first appearance"""
    _, first, inv = np.unique(x, return_index=True, return_inverse=True)
    return (np.argsort(np.argsort(first))[inv] + 1).astype(np.int64)


def credibleball_from_distances(num, K, alpha: float = 0.05) -> dict:
    """The selection behind credibleball, on the host, for callers that hold the distances already (rc_partition_distances
    through the C ABI): num[s] is the integer distance of sample s from the point estimate, K[s] its number of clusters.
      k = m − ⌊α·m + 1e-9⌋;  ε = the k-th smallest distance;  the ball is every sample with distance <= ε — ties at ε are in,
      so it may hold more than k samples (a ball is defined by its radius);
      horizontal: the ball's samples at distance ε;  upper: among the ball's samples with the fewest clusters, those of greatest
      distance;  lower: among the ball's samples with the most clusters, those of greatest distance
    (Wade & Ghahramani's vertical upper / lower and horizontal bounds; mcclust.ext's credibleball).  Returns a dict: epsilon_num,
    level = |ball|/m, ball (bool[m]) and horizontal_index, upper_index, lower_index (ascending 0-based sample indices)."""
    if not 0.0 <= alpha < 1.0:
        raise ValueError("alpha must lie in [0, 1)")
    num, K = np.asarray(num), np.asarray(K)
    if num.ndim != 1 or num.shape != K.shape or len(num) == 0:
        raise ValueError("num and K must be vectors of the same positive length")
    m = len(num)
    k = m - int(np.floor(alpha * m + 1e-9))
    eps = np.sort(num)[k - 1]
    ball = num <= eps

    def farthest(mask):
        return np.flatnonzero(mask & (num == num[mask].max()))

    return dict(epsilon_num=int(eps), level=int(ball.sum()) / m, ball=ball, horizontal_index=np.flatnonzero(ball & (num == eps)),
                upper_index=farthest(ball & (K == K[ball].min())), lower_index=farthest(ball & (K == K[ball].max())))


def credibleball(clust, samples, loss="VI", alpha: float = 0.05, device: int = 0) -> dict:
    """The (1 − alpha) credible ball around the point estimate `clust` (Wade & Ghahramani 2018; mcclust.ext's credibleball):
    the smallest ball in the metric `loss` ("binder", "VI" or "ID") that holds at least 1 − alpha of the samples (an
    MCMCResult, anything with `.clusts`, or an m×n label matrix), and its three bounds — see credibleball_from_distances for
    the definition.  The distances come from the GPU in exact integers (partitiondistances), so ties are ties.
    Returns that function's dict and: epsilon (the radius in the units of partitiondistances), distances and distances_num (m),
    K (m, the samples' cluster counts), and horizontal, upper, lower: the distinct partitions among the samples of each bound,
    sortlabels'd, in order of first occurrence."""
    if loss not in _DIST_LOSSES:
        raise ValueError("Invalid loss function specifier.")
    if not 0.0 <= alpha < 1.0:
        raise ValueError("alpha must lie in [0, 1)")
    labs, S = _distance_inputs(clust, samples)
    if labs.shape[0] != 1:
        raise ValueError("clust must be one labelling")
    dist, info = partitiondistances(labs, S, loss, device=device)
    out = credibleball_from_distances(info["num"][0], info["K_samples"], alpha)
    out.update(epsilon=float(_divide(out["epsilon_num"], _denominator(loss, S.shape[1]))), distances=dist[0], distances_num=info["num"][0],
               K=info["K_samples"], kernel_ms=info["kernel_ms"])
    for name in ("horizontal", "upper", "lower"):
        parts, seen = [], set()
        for i in out[name + "_index"]:
            c = _sortlabels(S[i])
            if c.tobytes() not in seen:
                seen.add(c.tobytes())
                parts.append(c)
        out[name] = np.stack(parts)
    return out


def lossmatrix(samples, loss: str = "VI", device: int = 0):
    """The symmetrised matrix of pairwise losses that getpointestimate(method="MPEL") searches (pointestimate.jl:49-56)
    and its column sums."""
    clusts = samples.clusts if hasattr(samples, "clusts") else samples
    if loss not in _LOSSES:
        raise ValueError("Invalid loss function specifier.")
    S = np.stack([_labels(c) for c in clusts])
    M, cs, _, _ = _lib.loss_matrix(S, _LOSSES[loss], device=device)
    return M, cs


def binderloss(a, b, normalised: bool = True, device: int = 0) -> float:
    """pointestimate.jl:68-76"""
    _check_lengths(a, b, "Length of the input vectors must be equal.")
    n = len(a)
    pm = _lib.pair_measures(_labels(a), _labels(b), device)
    return pm["mirkin"] * (1 if normalised else n * (n - 1) // 2)


def infodist(a, b, normalised: bool = True, device: int = 0) -> float:
    """pointestimate.jl:89-99"""
    _check_lengths(a, b, "Length of the input vectors must be equal.")
    pm = _lib.pair_measures(_labels(a), _labels(b), device)
    return pm["nid"] if normalised else pm["id"]


def varinfo(a, b, device: int = 0) -> float:
    """Clustering.jl's varinfo, as getpointestimate(loss=varinfo) uses it (test_pointestimates.jl:15)."""
    _check_lengths(a, b, "Length of the input vectors must be equal.")
    return _lib.pair_measures(_labels(a), _labels(b), device)["vi"]


def evaluateclustering(clusts, truth, device: int = 0) -> dict:
    """summaries.jl:12-23 — keys as the reference's named tuple."""
    _check_lengths(clusts, truth, "Length of inputs must be equal.")
    n = len(clusts)
    pm = _lib.pair_measures(_labels(clusts), _labels(truth), device)
    return dict(nbloss=pm["mirkin"], ari=pm["ari"], vi=pm["vi"], nvi=pm["vi"] / np.log(n), id=pm["id"],
                nid=pm["id"] / np.log(n), nmi=pm["nmi"])


def summarise(*args, io=None, device: int = 0) -> None:
    """summaries.jl:32-45: summarise([io], clusts, truth)."""
    if len(args) == 3:
        io, clusts, truth = args
    else:
        clusts, truth = args
    io = io or sys.stdout
    t = evaluateclustering(clusts, truth, device=device)
    print("Clustering summary", file=io)
    print(f"Number of clusters : {len(np.unique(clusts))}", file=io)
    print(f"Normalised Binder loss : {t['nbloss']}", file=io)
    print(f"Adjusted Rand Index : {t['ari']}", file=io)
    print(f"Normalised Variation of Information (NVI) distance : {t['nvi']}", file=io)
    print(f"Normalised Information Distance (NID) : {t['nid']}", file=io)
    print(f"Normalised Mutual Information : {t['nmi']}", file=io)
