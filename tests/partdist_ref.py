"""NumPy restatement of the partition distances (DESIGN.md §8 "Partition distances", include/redclust_hip.h
rc_partition_distances) and of the credible ball built on them: plain loops over bincount tables and Python integers, test
infrastructure only.  Everything is integer arithmetic on a given table G (the library's rc_vi_gtable), so the device has to
reproduce every number bit for bit."""
import numpy as np

import psm_search_ref as R
from vi_search_ref import phi_table


def _dense(x):
    return np.unique(np.asarray(x), return_inverse=True)[1].astype(np.int64)


def marginals(rows, Phi):
    """(Σ n_k², Σ Φ(n_k), K) of every row, int64"""
    out = np.zeros((len(rows), 3), np.int64)
    for r, x in enumerate(rows):
        sizes = np.bincount(_dense(x))
        out[r] = (sum(int(v) ** 2 for v in sizes), sum(Phi[int(v)] for v in sizes), len(sizes))
    return out


def distances_ref(labels, samples, G):
    """P[l][s] = Σ_kl N_kl², T[l][s] = Σ_kl Φ(N_kl) from every pair's contingency table, and the marginals (Σ n_k², Σ Φ(n_k), K)
    of the labellings and of the samples — four int64 arrays (every value is below 2^52)."""
    labels, samples = np.atleast_2d(np.asarray(labels)), np.atleast_2d(np.asarray(samples))
    Phi = phi_table(G)
    P = np.zeros((len(labels), len(samples)), np.int64)
    T = np.zeros_like(P)
    dense = [_dense(s) for s in samples]
    for l, c in enumerate(labels):
        c = _dense(c)
        for s, z in enumerate(dense):
            cells = np.bincount(c * (int(z.max()) + 1) + z)
            cells = cells[cells > 0]
            P[l, s] = sum(int(v) ** 2 for v in cells)
            T[l, s] = sum(Phi[int(v)] for v in cells)
    return P, T, marginals(labels, Phi), marginals(samples, Phi)


def numerators(P, T, A, B, loss):
    """the L×m integer distances of include/redclust_hip.h from distances_ref's outputs"""
    if loss == "binder":
        num = A[:, 0][:, None] + B[:, 0][None, :] - 2 * P
        assert not (num & 1).any()
        return num // 2
    if loss == "VI":
        return A[:, 1][:, None] + B[:, 1][None, :] - 2 * T
    assert loss == "ID"
    return np.maximum(A[:, 1][:, None], B[:, 1][None, :]) - T


def denominator(loss, n):
    return n * (n - 1) // 2 if loss == "binder" else 2 ** 32 * n


def credibleball_ref(num, K, alpha):
    """The definition, one step at a time: k = m − ⌊α·m + 1e-9⌋, ε the k-th smallest distance, the ball every sample within ε;
    horizontal: the ball's samples at ε; upper / lower: of the ball's samples with the fewest / most clusters, the farthest."""
    num, K = [int(x) for x in num], [int(x) for x in K]
    m = len(num)
    k = m - int(np.floor(alpha * m + 1e-9))
    eps = sorted(num)[k - 1]
    ball = [s for s in range(m) if num[s] <= eps]

    def farthest(members):
        far = max(num[s] for s in members)
        return [s for s in members if num[s] == far]

    kmin, kmax = min(K[s] for s in ball), max(K[s] for s in ball)
    return dict(epsilon_num=eps, level=len(ball) / m, ball=np.array([s in ball for s in range(m)]),
                horizontal_index=[s for s in ball if num[s] == eps],
                upper_index=farthest([s for s in ball if K[s] == kmin]),
                lower_index=farthest([s for s in ball if K[s] == kmax]))


def distinct_partitions(samples, index):
    """the distinct partitions among samples[index], sortlabels'd, in order of first occurrence"""
    out = []
    for i in index:
        c = R.sortlabels(samples[i])
        if not any(np.array_equal(c, o) for o in out):
            out.append(c)
    return np.stack(out)


def varied_samples(n, m, K, noise, seed):
    """psm_search_ref.planted_counts' samples with their cluster counts varied: in sample s ≡ 1 (mod 3) every second member of
    its largest cluster (ties: the smallest label) moves to the smallest unused label; in sample s ≡ 2 (mod 3) its two
    smallest-named clusters are merged."""
    S, _ = R.planted_counts(n, m, K, noise, seed)
    S = S.copy()
    for s in range(m):
        names, sizes = np.unique(S[s], return_counts=True)
        if s % 3 == 1:
            members = np.flatnonzero(S[s] == names[np.argmax(sizes)])
            S[s, members[1::2]] = min(set(range(1, n + 1)) - set(names.tolist()))
        elif s % 3 == 2 and len(names) > 1:
            S[s, S[s] == names[1]] = names[0]
    S.setflags(write=False)
    return S
