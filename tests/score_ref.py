"""Reference for the scoring of labellings (csrc/score.inc.hip): the K×K block sums of a labelling against the quantised
matrices, in Python integers, and the (hi, lo) halves the library carries them in.  Not product code.

For a labelling with clusters in ascending label order k = 0..K−1 and k <= t:  B_X[k][t] = Σ_{i in k} Σ_{j in t} Xq[i][j]
for X = D and logD (rows in the smaller label, columns in the larger).  Blocks are listed in row-major (k, t >= k) order."""
import numpy as np

LO_BITS = 24


def clusters(z):
    """(ascending labels, dense id 0..K−1 of every point, sizes in that order)"""
    names, ids, sizes = np.unique(np.asarray(z, dtype=np.int64), return_inverse=True, return_counts=True)
    return names, ids.reshape(-1), sizes.astype(np.int64)


def block_sums(Dq, Lq, z):
    """[(B_D, B_L)] as Python integers.  The row sums to a cluster fit int64 (that is how the matrices are quantised), their
    sums over the rows of a cluster need not: those are Python integers."""
    _, ids, sizes = clusters(z)
    K = len(sizes)
    M = (ids[:, None] == np.arange(K)[None, :]).astype(np.int64)
    RD, RL = np.asarray(Dq, dtype=np.int64) @ M, np.asarray(Lq, dtype=np.int64) @ M      # [i][t]
    out = []
    for k in range(K):
        rows = np.flatnonzero(ids == k)
        for t in range(k, K):
            out.append((sum(int(x) for x in RD[rows, t]), sum(int(x) for x in RL[rows, t])))
    return out


def block_sums_bruteforce(Dq, Lq, z):
    """the same by the definition: a double loop over the entries"""
    names = sorted(set(int(x) for x in z))
    n = len(z)
    out = []
    for a, k in enumerate(names):
        for t in names[a:]:
            bd = bl = 0
            for i in range(n):
                for j in range(n):
                    if int(z[i]) == k and int(z[j]) == t:
                        bd += int(Dq[i][j]); bl += int(Lq[i][j])
            out.append((bd, bl))
    return out


def halves(Dq, Lq, z):
    """the blocks as the K(K+1)/2 × 4 int64 (D_hi, D_lo, L_hi, L_lo) the library returns: every per-row sum Σ_{j in t} Xq[i][j]
    split into v >> 24 and v & (2^24 − 1), the halves summed over the rows of cluster k"""
    _, ids, sizes = clusters(z)
    K = len(sizes)
    M = (ids[:, None] == np.arange(K)[None, :]).astype(np.int64)
    mask = (1 << LO_BITS) - 1
    out = np.zeros((K * (K + 1) // 2, 4), np.int64)
    parts = []
    for X in (Dq, Lq):
        R = np.asarray(X, dtype=np.int64) @ M
        parts += [M.T @ (R >> LO_BITS), M.T @ (R & mask)]          # [k][t]
    b = 0
    for k in range(K):
        for t in range(k, K):
            out[b] = [parts[0][k, t], parts[1][k, t], parts[2][k, t], parts[3][k, t]]
            b += 1
    return out


def values(blocks):
    """[(B_D, B_L)] as Python integers from the library's K(K+1)/2 × 4 halves"""
    return [(int(b[0]) * (1 << LO_BITS) + int(b[1]), int(b[2]) * (1 << LO_BITS) + int(b[3])) for b in np.asarray(blocks).reshape(-1, 4)]


def quantised(M, e):
    """the integers behind a matrix of Context.get_matrix (value = q·2^-e exactly)"""
    q = np.ldexp(np.asarray(M, dtype=np.float64), int(e))
    assert np.array_equal(q, np.rint(q))
    return q.astype(np.int64)
