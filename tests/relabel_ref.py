"""NumPy restatement of rc_relabel (csrc/relabel.inc.hip; DESIGN.md §8 "Relabelling"), in int64 throughout: the contingency
table of a sample with the pivot, the assignment by shortest augmenting paths with the library's tie rule, and labels, maps,
overlap and counts as the device returns them.  The assignment is written out from the definition — rows the side with fewer
clusters (the pivot on a tie) inserted in ascending dense id from zero potentials, every step to the unused column of minimum
reduced cost, the smallest column id among equals — vectorised over the columns, one Python step per step of the algorithm."""
import numpy as np

INF = np.int64(0x3fffffff)


def table(c, z):
    """(N, pivot names, sample names): N[k][l] = #{j : c_j has dense id k, z_j has dense id l}, dense ids in ascending label order"""
    cn, ci = np.unique(np.asarray(c), return_inverse=True)
    zn, zi = np.unique(np.asarray(z), return_inverse=True)
    N = np.zeros((len(cn), len(zn)), np.int64)
    np.add.at(N, (ci.reshape(-1), zi.reshape(-1)), 1)
    return N, cn.astype(np.int64), zn.astype(np.int64)


def assign_rows(T):
    """T: R×C int64 with R <= C.  Returns col_of_row (R, 0-based): the maximum-weight matching of every row to a distinct
    column, by shortest augmenting paths on cost = −T (columns 1..C, column 0 the root of every path)."""
    T = np.asarray(T, np.int64)
    R, C = T.shape
    assert 1 <= R <= C
    u = np.zeros(R + 1, np.int64)
    v = np.zeros(C + 1, np.int64)
    p = np.zeros(C + 1, np.int64)                    # p[j]: the row of column j, 0 = free
    way = np.zeros(C + 1, np.int64)
    cost = np.zeros((R + 1, C + 1), np.int64)
    cost[1:, 1:] = -T
    cols = np.arange(C + 1)
    for i in range(1, R + 1):
        p[0] = i
        j0 = 0
        minv = np.full(C + 1, INF, np.int64)
        used = np.zeros(C + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used
            free[0] = False
            cur = cost[i0] - u[i0] - v
            better = free & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            cand = cols[free]
            delta = minv[cand].min()                 # may be negative in a row's first step: potentials start at zero
            j1 = cand[np.argmax(minv[cand] == delta)]        # the smallest column id among the minima
            u[p[used]] += delta                      # the rows of the used columns are distinct
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col_of_row = np.zeros(R, np.int64)
    for j in range(1, C + 1):
        if p[j]:
            col_of_row[p[j] - 1] = j - 1
    return col_of_row


def match(N):
    """N: K_p×K_s.  Returns to (K_s): the pivot's dense id each of the sample's clusters is sent to, −1 = unmatched."""
    Kp, Ks = N.shape
    to = np.full(Ks, -1, np.int64)
    if Kp <= Ks:                                     # the pivot's clusters are the rows
        col = assign_rows(N)
        to[col] = np.arange(Kp)
    else:
        to[:] = assign_rows(N.T)
    return to


def relabel_ref(samples, pivot):
    """dict(labels m×n int64, maps m×W int64, overlap m int64, counts n×(K_p+1) uint32, pivot_labels) as rc_relabel returns them"""
    S = np.asarray(samples, np.int64)
    c = np.asarray(pivot, np.int64)
    m, n = S.shape
    tabs = [table(c, z) for z in S]
    cn = tabs[0][1]
    cid = np.searchsorted(cn, c)
    Kp = len(cn)
    W = max(len(t[2]) for t in tabs)
    labels = np.zeros((m, n), np.int64)
    maps = np.full((m, W), -1, np.int64)
    overlap = np.zeros(m, np.int64)
    counts = np.zeros((n, Kp + 1), np.uint32)
    for s, (N, _, zn) in enumerate(tabs):
        to = match(N)
        Ks = len(zn)
        assert (to >= 0).sum() == min(Kp, Ks) and len(set(to[to >= 0])) == min(Kp, Ks)
        maps[s, :Ks] = np.where(to >= 0, cn[np.maximum(to, 0)], 0)
        zid = np.searchsorted(zn, S[s])
        k = to[zid] + 1                              # the column of counts: 0 = unmatched
        labels[s] = maps[s, zid]
        overlap[s] = sum(int(N[to[l], l]) for l in range(Ks) if to[l] >= 0)
        assert overlap[s] == int(np.sum((k - 1) == cid))
        counts[np.arange(n), k] += 1
    return dict(labels=labels, maps=maps, overlap=overlap, counts=counts, pivot_labels=cn)
