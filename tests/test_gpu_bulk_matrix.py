"""Every row-reduction kernel the product library can launch, at the shapes where tiled kernels go wrong (-m gpu).

bulk_choice chooses among fourteen kernels by storage width, by whether logD is derived, by RC_SYM_VARIANT and by the symmetric /
full-read choice (tests/bulk_rows.py lists them).  Each is put through
  * test_row_sums: rc_set_state, then the S table the kernel just wrote (rc_debug_rowsums) against plain integer sums of the
    fixed-point matrices, both matrices bit for bit, plus Σ_labels S == rc_debug_rowtotals — for every size of SIZES (tile edges:
    128-column blocks with 8- and 16-row units, 128/32 and 256/16 tiles, k_bulk's 512- and 1024-element chunks, two columns per
    lane), every labelling of labelings() and with the cluster-contiguous re-layout on and off (RC_NO_RELAYOUT=1: cluster
    boundaries inside a lane's column pair right after rc_set_state);
  * test_sweeps: at n = 1029 from perturbed labels, six sweeps against the oracle (labels, sizes, K, change counts exactly,
    loglik to 1e-9, the table after the last sweep bit for bit), the same sweeps enqueued without blocking and once in the
    incremental mode — where a variant that clears the wrong S generation or disagrees with the resolver's in-place corrections
    shows.
In every case rc_bulk_kernel_name must be the row's kernel: a case that ends up in another kernel fails.

Matrices: random symmetric, zero diagonal; `narrow` has entries in [0.5, 4) (three binades: folded log table), `wide` is
log-uniform over twelve binades (stays derived: every entry >= 2^32 quanta; not folded).  Both carry entries exactly on binade
edges (0.5, 1, 2, nextafter(2, 0)) and the maximum 4 - 2^-40, which quantises to 2^47 - 32: the top of the 47-bit packed range.
The derived rows 3-6 run on `wide` (rc_qlog has to derive every exponent), the stored rows on `narrow` (their logD is data).

Wall time of `pytest -m gpu` on one MI355X: 238 s with this file and tests/test_gpu_diagonal.py (454 tests), of which the two new
files take 78 s (68 s + 10 s by pytest's per-test durations) and the tests of the parent commit 157 s — the parent's own run, 272
tests, was not timed apart: its figure is what the same run spends outside the new files, about 160 s with collection.  The budget
was half of the parent's time, so one context serves all labellings of a (kernel, size, re-layout setting) and the reference sums
are computed once per (matrix, storage); no size, labelling or kernel row was dropped.
"""
import numpy as np
import pytest

import bulk_rows as B
import redclust_amd as rc

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 7, 8, 9, 31, 33, 127, 128, 129, 255, 256, 257, 513, 1023, 1025, 2047, 2056, 4097]
BIG = 8197                                                 # a full grid (n >= 8192, n % 8 != 0) for the kernels the headline tests never see
BIG_ROWS = ("03", "04", "05", "08", "09", "10", "13")
TOP = 4.0 - 2.0 ** -40


def matrix(kind, n):
    """symmetric, zero diagonal; see the module docstring"""
    rng = np.random.default_rng(1000 + n)
    U = rng.random((n, n))
    X = (0.5 + 3.5 * U) if kind == "narrow" else np.exp2(-10.0 + 12.0 * U)
    X = np.minimum(X, TOP)
    iu = np.triu_indices(n, 1)
    npairs = len(iu[0])
    edges = [TOP] + ([2.0 ** -10] if kind == "wide" else []) + [0.5, np.nextafter(2.0, 0.0), 2.0, 1.0]
    pos = rng.permutation(npairs)[:len(edges)]
    for q, v in zip(pos, edges):
        X[iu[0][q], iu[1][q]] = v
    D = np.triu(X, 1)
    return D + D.T


def labelings(n):
    rng = np.random.default_rng(2000 + n)
    out = {"one": np.ones(n, np.int64)}
    if n <= 4096:
        out["singletons"] = np.arange(1, n + 1, dtype=np.int64)
    # contiguous runs, every boundary at an odd position: the first run has odd length, the others even
    runs, pos, k = np.empty(n, np.int64), 0, 1
    while pos < n:
        ln = 2 * int(rng.integers(1, max(2, n // 12) + 1)) - (1 if pos == 0 else 0)
        runs[pos:pos + ln] = k
        pos += ln; k += 1
    out["odd_runs"] = runs
    out["alternating"] = 1 + (np.arange(n, dtype=np.int64) % 2)
    out["uniform9"] = rng.integers(1, min(9, n) + 1, n).astype(np.int64)           # (labels lie in 1..n)
    out["alternating"] = np.minimum(out["alternating"], n)
    # many clusters of 1..7 points next to three large ones, points in random order (the layout puts small clusters first)
    lab, pos, k = np.empty(n, np.int64), 0, 1
    while pos < (2 * n) // 5:
        ln = int(rng.integers(1, 8))
        lab[pos:pos + ln] = k
        pos += ln; k += 1
    lab[pos:] = k + rng.integers(0, 3, max(n - pos, 0))
    out["small_and_large"] = np.minimum(lab, n)[rng.permutation(n)]   # (labels lie in 1..n: the tiniest sizes merge a few)
    vals = np.arange(n, 0, -3, dtype=np.int64)[:12]        # sparse, high labels: n, n-3, ... so that slot != label
    out["sparse_high"] = vals[rng.integers(0, len(vals), n)]
    for v in out.values():
        assert v.shape == (n,) and v.min() >= 1 and v.max() <= n
    return out


_matrices, _references = {}, {}


def _matrix(kind, n):
    if (kind, n) not in _matrices:
        if n >= 4096:
            _matrices.clear()                              # (at most one large matrix is kept)
        _matrices[(kind, n)] = matrix(kind, n)
    return _matrices[(kind, n)]


def _reference(row, ctx, D, L_host, labs):
    """Reference sums of every labelling for this (matrix, storage, exponents): computed once, shared by the rows of a storage."""
    eD, eL = ctx.debug_rowsums(1)[2:4]
    key = (row.data, row.storage, len(D), eD, eL)
    if key not in _references:
        Dq, Lq, _, _ = B.reference_matrices(row, ctx, D, L_host)
        assert np.array_equal(Dq, Dq.T) and np.array_equal(Lq, Lq.T) and not Lq.diagonal().any()
        tot = (Dq.sum(axis=1), Lq.sum(axis=1))
        refs = {}
        for name, lab in labs.items():
            ks = B.pick_clusters(lab)
            refs[name] = (ks, B.cluster_rowsums(Dq, lab, ks), B.cluster_rowsums(Lq, lab, ks)) + tot
        _references[key] = (refs, B.expected_folded(row._replace(fold=1), Dq))
    refs, fold1 = _references[key]
    return refs, fold1 and row.fold == 1


def _run_size(row, n, relayout, kernel_by_env=False, env=None):
    D = _matrix(row.data, n)
    labs = labelings(n)
    ctx, L_host = B.make_context(row, D, relayout=relayout, kernel_by_env=kernel_by_env, env=env)
    try:
        ctx.set_state(labs["one"])
        refs, folded = _reference(row, ctx, D, L_host, labs)
        for name, lab in labs.items():
            what = (row.id, n, "relayout" if relayout else "RC_NO_RELAYOUT=1", name)
            ctx.set_state(lab)
            B.check_table(ctx, None, None, lab, what, ref=refs[name])
            assert ctx.bulk_kernel_name() == row.name, (what, ctx.bulk_kernel_name())
            if row.storage == "derived" and n > 1:
                assert ctx.log_table_folded() == folded, (what, ctx.log_table_folded())
    finally:
        ctx.close()
    return folded


@pytest.mark.parametrize("relayout", [True, False], ids=["relayout", "norelayout"])
@pytest.mark.parametrize("row", B.ROWS, ids=B.ROW_IDS)
def test_row_sums(row, relayout):
    folded = {n: _run_size(row, n, relayout) for n in SIZES + ([BIG] if row.id in BIG_ROWS else [])}
    if row.id == "01":
        assert all(folded[n] for n in SIZES if n > 1)       # what tells row 1 from row 2: the folded table
    if row.id.startswith("02"):
        assert not any(folded[n] for n in SIZES if n > 2)   # (n = 2 has one entry: one binade, whatever the distribution)


def test_stored_log_by_environment():
    """RC_STORED_LOG=1 with D alone: the stored form (row 7's kernel), logD computed by the library within one quantum of the
    host's log; the sums are those of the integers rc_get_matrix(1) reports.  Sizes: the quantum 2^-eL has to be a bound that two
    correct logarithms can meet.  The library's log and libm's are each within one ulp of log, i.e. within 2^-51 of each other for
    |log D| < 2, and the stored value is rounded to the quantum (half a quantum more): 2^-51 + 2^-(eL+1) <= 2^-eL needs eL <= 50,
    and eL = 62 - 1 - ceil(log2 n) is from n = 1025 on (at n = 129 the quantum, 2^-53, is finer than the spacing of the doubles)."""
    row7 = next(r for r in B.ROWS if r.id == "07")
    for n in (1029, 2056):
        D = matrix("narrow", n)
        lab = labelings(n)["uniform9"]
        with B.environment(RC_STORED_LOG="1"):
            ctx = rc.Context(D)
        ctx.set_bulk_kernel("sym")
        ctx.set_state(lab)
        eD, eL = ctx.debug_rowsums(1)[2:4]
        L = ctx.get_matrix(1)
        assert eL <= 50 and np.abs(L).max() < 2.0
        err = np.abs(L - B.host_log(D)).max()
        print("RC_STORED_LOG: n", n, "eL", eL, "largest |logD - log D|", err, "quantum", 2.0 ** -eL)
        assert err <= 2.0 ** -eL and not L.diagonal().any()
        B.check_table(ctx, B.quantise(D, eD), B.quantise(L, eL), lab, ("RC_STORED_LOG", n))
        assert ctx.bulk_kernel_name() == row7.name and not ctx.log_table_folded()
        ctx.close()


@pytest.mark.parametrize("row", [r for r in B.ROWS if r.id in ("01", "06", "07", "11", "12", "14")], ids=lambda r: f"{r.id}-{r.kernel}")
def test_kernel_choice_by_environment(row):
    """RC_BULK_KERNEL=sym / perm in place of rc_set_bulk_kernel"""
    for n in (129, 1029):
        _run_size(row, n, True, kernel_by_env=True)


@pytest.mark.parametrize("value", ["4", "-1", "17"])
def test_sym_variant_out_of_range_is_automatic(value):
    """RC_SYM_VARIANT outside 0..3 means "automatic", as if it were not set: the kernels of rows 1, 7 and 12, named truthfully."""
    for row in B.DEFAULT_ROWS:
        _run_size(row._replace(variant=value), 257, True)


def test_two_per_cu_lists_at_a_ragged_size():
    """k_bulk_syml2 reads its second set of unit lists (two blocks per CU) only for a launch enqueued while the last sweep changed
    more than 32 labels.  n = 135 is one full column block plus seven rows — the last block has 128 fast rows and one slow unit —
    and from uniformly random labels on a matrix without structure nearly every point moves in every sweep (the CPU oracle: 124 to
    135 changes per sweep of this chain), so every launch after the first sweep takes those lists.  The full-read kernel, which has
    no lists, runs the same chain: labels and the row sums of every live label must agree exactly after every sweep."""
    n, nsweeps, seed = 135, 6, 77
    D = matrix("narrow", n)
    init = np.random.default_rng(3000).integers(1, 21, n).astype(np.int64)
    P = rc.likelihood_hyperparams(D, init)
    row_sym, row_perm = (next(r for r in B.ROWS if r.id == i) for i in ("01", "06"))
    sym, _ = B.make_context(row_sym, D)
    perm, _ = B.make_context(row_perm, D)
    try:
        for ctx in (sym, perm):
            ctx.set_params(**P)
            ctx.set_state(init)
        changes = []
        for t in range(nsweeps):
            r, p = B.rp_schedule(t)
            for ctx in (sym, perm):
                ctx.gibbs_sweep(r, p, seed, t)
            assert sym.bulk_kernel_name() == row_sym.name and perm.bulk_kernel_name() == row_perm.name, t
            lab = sym.get_state()[0]
            assert np.array_equal(lab, perm.get_state()[0]), (t, int(np.sum(lab != perm.get_state()[0])))
            changes.append(sym.sweep_stats()["n_changes"])
            assert changes[-1] == perm.sweep_stats()["n_changes"], t
            for k in np.unique(lab):
                for a, b in zip(sym.debug_rowsums(int(k))[:2], perm.debug_rowsums(int(k))[:2]):
                    assert np.array_equal(a, b), (t, int(k), np.flatnonzero(a != b)[:8])
        print("label changes per sweep:", changes)
        assert max(changes[:-1]) > 32, changes                 # some sweep with that many changes was followed by another
    finally:
        sym.close()
        perm.close()


@pytest.fixture(scope="module")
def sweep_data():
    return B.sweep_data()


@pytest.mark.parametrize("row", B.ROWS, ids=B.ROW_IDS)
def test_sweeps(row, sweep_data):
    mats, truth, init = sweep_data
    D = mats[row.data]
    B.run_sweeps(row, D, rc.likelihood_hyperparams(D, truth), init)
