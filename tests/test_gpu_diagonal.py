"""A nonzero diagonal of D on the device (-m gpu).

The reference keeps D's diagonal as given (types.jl:155 zeroes only logD's) and loglik adds it: matsum(D, clust_k, clust_k)/2 of
mcmc.jl:32 includes D[i,i].  The library carries the diagonal apart in many places — added under `if (x)` in the symmetric row
reductions, taken off the point's own cluster in k_resolve and k_sweep_wide, removed again in rc_within_between and the k-medoids
split kernels, moved by k_gather_ll on a re-layout, masked away from rc_qlog in the derived kernels — none of which a zero
diagonal reaches.  tests/test_diagonal_cpu.py pins the CPU references (the sweep must not see the diagonal, loglik must); here
  * every kernel row of tests/bulk_rows.py: the matrices as stored, the row-sum table with Dq[i][i] in the point's own cluster,
    six sweeps against the oracle in both modes, blocking and not, and loglik — which must differ from the zero-diagonal value by
    far more than the tolerance, or the test could pass with the diagonal dropped;
  * the three default contexts (derived, stored 64-bit, 32-bit): rc_within_between, the k-medoids scan's split, split–merge with
    checkpoint / restore, an automatic re-layout, rc_run_chain; and a wide context (k_sweep_wide).
Diagonals: positive (uniform in [0.1, 3]), mixed sign (N(0, 2)), larger than every off-diagonal entry (constant 50).
"""
import os

import numpy as np
import pytest

import bulk_rows as B
import oracle_lib as O
import redclust_amd as rc
from helpers import cluster_terms_positive, golden_case, load_golden, rp_schedule, with_diagonal

pytestmark = pytest.mark.gpu

LL_RTOL = 1e-9
KINDS = ["positive", "mixed", "large"]
WB = ("count_within", "count_between", "sum_within", "sumlog_within", "sum_between", "sumlog_between")


@pytest.fixture(scope="module")
def synthetic():
    return B.sweep_data()


def _case(size, row, synthetic):
    if size == "paper100":
        g, d = load_golden()
        D0, P, init, _ = golden_case(g, d, "d2_random")
        return D0, P, init
    mats, truth, init = synthetic
    D0 = mats[row.data]
    return D0, rc.likelihood_hyperparams(D0, truth), init


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", ["paper100", "synthetic1029"])
@pytest.mark.parametrize("row", B.ROWS, ids=B.ROW_IDS)
def test_every_kernel_row_with_a_diagonal(row, size, kind, synthetic):
    D0, P, init = _case(size, row, synthetic)
    D = with_diagonal(D0, kind)
    ctx, L_host = B.make_context(row, D)
    try:
        ctx.set_params(**P)
        ctx.set_state(init)
        Dq, Lq, eD, eL = B.reference_matrices(row, ctx, D, L_host)
        assert np.array_equal(Dq.diagonal(), B.quantise(np.diag(D), eD)) and Dq.diagonal().any()
        G = ctx.get_matrix(0)
        assert np.array_equal(G, np.ldexp(Dq.astype(np.float64), -eD))                # D as stored, the diagonal included,
        assert np.abs(np.diag(G) - np.diag(D)).max() <= 2.0 ** -(eD + 1)              # to the quantum of D
        assert not ctx.get_matrix(1).diagonal().any()                                  # logD's diagonal is exactly 0
    finally:
        ctx.close()
    # the initial table (Dq[i][i] in the point's own cluster), sweeps in both modes, blocking and not, the table after them
    ll, orc = B.run_sweeps(row, D, P, init)
    assert cluster_terms_positive(D, orc.clusts, P["beta"])
    # the same partition on the zero-diagonal matrix: loglik must be far away, or a dropped diagonal would pass
    ctx0, _ = B.make_context(row, D0)
    try:
        ctx0.set_params(**P)
        ctx0.set_state(orc.clusts)
        ll0 = ctx0.loglik()
    finally:
        ctx0.close()
    assert abs(ll - ll0) > 1000 * LL_RTOL * abs(ll), (ll, ll0)


def _paper(d):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paper_datasets.npz"))
    return z[f"D{d}"], z[f"labels{d}"]


def _default_context(row, D, kcap=0):
    """as a caller creates it: no switch, no forced kernel"""
    with B.environment():
        if row.storage == "derived":
            return rc.Context(D, kcap=kcap), None
        L = B.host_log(D)
        return rc.Context(D, logD=L, kcap=kcap, storage_bits=32 if row.storage == "32" else 64), L


def _oracle(row, ctx, D, L_host, P):
    Dq, Lq, eD, eL = B.reference_matrices(row, ctx, D, L_host)
    orc = O.Oracle(D, P, logD=np.ldexp(Lq.astype(np.float64), -eL), eD=eD, eL=eL)
    assert np.array_equal(orc.Dq, Dq) and np.array_equal(orc.Lq, Lq)
    return orc, Dq, Lq


DEFAULT_IDS = [r.storage for r in B.DEFAULT_ROWS]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", B.DEFAULT_ROWS, ids=DEFAULT_IDS)
def test_within_between_leaves_the_diagonal_out(row, kind):
    """fitprior's A / B split is over the strict upper triangle (prior.jl:73-75)"""
    n = 700
    data = rc.generatemixture(n, 6, seed=12, sigma=0.3, dim=8)
    sh = np.random.default_rng(0).permutation(n)
    D = with_diagonal(np.ascontiguousarray(data["distancematrix"][np.ix_(sh, sh)]), kind)
    lab = data["clusts"][sh]
    ctx, _ = _default_context(row, D)
    try:
        ctx.set_state(lab)
        w = ctx.within_between()
        iu = np.triu_indices(n, 1)
        same = (lab[:, None] == lab[None, :])[iu]
        assert w["count_within"] == int(same.sum()) and w["count_between"] == int((~same).sum())
        # the matrices as the context stores them (rc_get_matrix: per-entry kernels); the derived context also against the host's
        # doubles, as tests/test_gpu_parity.py::test_within_between_split_from_block_sums
        mats = [(ctx.get_matrix(0), ctx.get_matrix(1))] + ([(D, B.host_log(D))] if row.storage == "derived" else [])
        for Dm, Lm in mats:
            assert np.isclose(w["sum_within"], Dm[iu][same].sum(), rtol=1e-12, atol=0)
            assert np.isclose(w["sum_between"], Dm[iu][~same].sum(), rtol=1e-12, atol=0)
            assert np.isclose(w["sumlog_within"], Lm[iu][same].sum(), rtol=1e-10, atol=0)
            assert np.isclose(w["sumlog_between"], Lm[iu][~same].sum(), rtol=1e-10, atol=0)
        with_diag = D[iu][same].sum() + np.diag(D).sum() / 2                           # what a diagonal left in would give
        assert not np.isclose(w["sum_within"], with_diag, rtol=1e-6, atol=0)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["small_positive", "negative"])
@pytest.mark.parametrize("row", B.DEFAULT_ROWS, ids=DEFAULT_IDS)
def test_kmedoids_split_equals_within_between(row, kind):
    """rc_kmedoids_scan_split == rc_within_between of the same labelling, bit for bit (as check_split of
    tests/test_gpu_fitprior2.py).  The diagonal lies below the smallest off-diagonal entry, so that every medoid stays in its
    own group (a larger one legitimately is RC_ERR_DOMAIN)."""
    n = 300
    D = rc.generatemixture(n, 8, seed=2)["distancematrix"].copy()
    lo = D[~np.eye(n, dtype=bool)].min()
    rng = np.random.default_rng(3)
    D[np.diag_indices(n)] = rng.uniform(0.05, 0.9, n) * lo if kind == "small_positive" else -rng.uniform(0.1, 2.0, n)
    ctx, _ = _default_context(row, D)
    try:
        kmin, kmax, seed = 1, 150, 5
        scan = ctx.kmedoids_scan(kmin, kmax, maxiter=1000, seed=seed, split=True)
        plain = ctx.kmedoids_scan(kmin, kmax, maxiter=1000, seed=seed)
        for f in ("totalcost", "iterations", "converged"):
            assert np.array_equal(scan[f], plain[f]), f
        for k in (150, 1, 2, 7, 40):
            ctx.set_state(ctx.kmedoids(k, maxiter=1000, seed=seed).assignments)
            wb = ctx.within_between()
            for f in WB:
                assert scan[f][k - kmin] == wb[f], (k, f, scan[f][k - kmin], wb[f])
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", B.DEFAULT_ROWS, ids=DEFAULT_IDS)
def test_splitmerge_checkpoint_restore(row, kind):
    """Split–merge proposals against the oracle (k_apply_moves at column i = x), then checkpoint / restore; the row-sum table
    after each, bit for bit."""
    D0, truth = _paper(1)
    D = with_diagonal(D0, kind)
    P = rc.likelihood_hyperparams(D0, truth)
    init = truth.copy(); init[init == 2] = 1; init[init == 4] = 3; init[init == 9] = 8   # merged clusters: splits get accepted
    seed = 4322
    ctx, L_host = _default_context(row, D, kcap=64)
    try:
        ctx.set_params(**P)
        ctx.set_state(init)
        orc, Dq, Lq = _oracle(row, ctx, D, L_host, P)
        orc.set_state(init)
        ctx.attach_host_matrices(D, np.ldexp(Lq.astype(np.float64), -orc.eL))
        accepted = 0
        for t in range(12):
            inf = orc.mh_proposal(1.0, 0.5, 5, seed, t, 0, mode=1)
            got = ctx.splitmerge(1.0, 0.5, 5, seed, t, 0)
            assert got == (bool(inf.accept), bool(inf.split)), (t, got, inf.accept, inf.split)
            accepted += got[0]
            lab, sizes, K = ctx.get_state()
            assert np.array_equal(lab, orc.clusts) and np.array_equal(sizes, orc.sizes) and K == orc.K, t
            B.check_table(ctx, Dq, Lq, orc.clusts, (row.id, kind, "proposal", t))
            if t % 4 == 3:
                ctx.gibbs_sweep(1.0, 0.5, seed, t)
                orc.sweep_stable(1.0, 0.5, seed, t)
                assert np.array_equal(ctx.get_state()[0], orc.clusts), t
        assert accepted >= 1
        ref = orc.loglik_stable()
        assert abs(ctx.loglik() - ref) <= LL_RTOL * abs(ref)
        kept, ll = orc.clusts.copy(), ctx.loglik()
        ctx.checkpoint()
        for t in range(12, 15):
            ctx.splitmerge(1.0, 0.5, 5, seed, t, 0)
            ctx.gibbs_sweep(1.0, 0.5, seed, t)
        ctx.restore()
        assert np.array_equal(ctx.get_state()[0], kept) and ctx.loglik() == ll
        B.check_table(ctx, Dq, Lq, kept, (row.id, kind, "restored"))
    finally:
        ctx.close()


@pytest.mark.parametrize("row", B.DEFAULT_ROWS, ids=DEFAULT_IDS)
def test_automatic_relayout_moves_the_diagonal(row):
    """As tests/test_gpu_parity.py::test_automatic_relayout_is_invisible, with a mixed-sign diagonal: k_gather_ll moves it."""
    n, K = 2048, 4
    data = rc.generatemixture(n, K, seed=5, sigma=0.6, dim=6)
    sh = np.random.default_rng(8).permutation(n)
    D0 = np.ascontiguousarray(data["distancematrix"][np.ix_(sh, sh)])
    truth = data["clusts"][sh]
    D = with_diagonal(D0, "mixed")
    P = dict(rc.likelihood_hyperparams(D0, truth), maxK=12)
    ctx, L_host = _default_context(row, D, kcap=64)
    ref, _ = _default_context(row, D, kcap=64)
    try:
        ctx.set_params(**P); ctx.set_state(truth)
        ref.set_params(**P); ref.set_bulk_kernel("perm"); ref.set_state(truth)     # forced kernel: never re-lays out after rc_set_state
        l0 = ctx.layout_info()[0]
        moved = 0
        for t in range(120):
            ctx.gibbs_sweep(1.0, 0.5, 3, t, blocking=False)
            ref.gibbs_sweep(1.0, 0.5, 3, t, blocking=False)
            if t % 10 == 9:
                a, b = ctx.get_state(), ref.get_state()
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (t, ctx.layout_info())
                moved += ctx.sweep_stats()["n_changes"]
        assert moved > 0
        assert ctx.loglik() == ref.loglik()
        assert ctx.layout_info()[0] > l0, "expected at least one automatic re-layout (runs=%d)" % ctx.layout_info()[1]
        lab = ctx.get_state()[0]
        Dq, Lq, _, _ = B.reference_matrices(row, ctx, D, L_host)
        B.check_table(ctx, Dq, Lq, lab, (row.id, "after the re-layout"))
        ctx0, _ = _default_context(row, D0, kcap=64)
        ctx0.set_params(**P); ctx0.set_state(lab)
        ll0 = ctx0.loglik()
        ctx0.close()
        assert abs(ctx.loglik() - ll0) > 1000 * LL_RTOL * abs(ll0)
    finally:
        ctx.close(); ref.close()


def test_wide_context_all_singletons():
    """n just above 4096, every point a cluster of its own: the context is wide (k_sweep_wide takes the diagonal off the point's
    own cluster)."""
    n, K = 4100, 25
    data = rc.generatemixture(n, K, seed=9, sigma=0.15)
    D0, truth = data["distancematrix"], data["clusts"]
    D = with_diagonal(D0, "positive")
    P = rc.likelihood_hyperparams(D0, truth)
    init = np.arange(1, n + 1, dtype=np.int64)
    row = B.DEFAULT_ROWS[0]
    ctx, L_host = _default_context(row, D)
    try:
        ctx.set_params(**P)
        ctx.set_state(init)
        assert ctx.capacity_info()["kcap"] >= n
        orc, Dq, Lq = _oracle(row, ctx, D, L_host, P)
        orc.set_state(init)
        B.check_table(ctx, Dq, Lq, init, "wide, installed state", ks=[1, 2050, n])
        ll, ref = ctx.loglik(), orc.loglik_stable()
        assert abs(ll - ref) <= LL_RTOL * abs(ref), (ll, ref)
        for t in range(2):
            r, p = rp_schedule(t)
            ctx.gibbs_sweep(r, p, 4242, t)
            orc.sweep_stable(r, p, 4242, t)
            lab, sizes, Kc = ctx.get_state()
            assert np.array_equal(lab, orc.clusts) and np.array_equal(sizes, orc.sizes) and Kc == orc.K, t
            assert ctx.sweep_stats()["n_changes"] == orc.last_changes
        ks = np.unique(orc.clusts)
        B.check_table(ctx, Dq, Lq, orc.clusts, "wide, after two sweeps", ks=ks[[0, len(ks) // 2, -1]])
        ll, ref = ctx.loglik(), orc.loglik_stable()
        assert abs(ll - ref) <= LL_RTOL * abs(ref), (ll, ref)
        ctx0, _ = _default_context(row, D0)
        ctx0.set_params(**P); ctx0.set_state(orc.clusts)
        ll0 = ctx0.loglik()
        ctx0.close()
        assert abs(ll - ll0) > 1000 * LL_RTOL * abs(ll)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", B.DEFAULT_ROWS, ids=DEFAULT_IDS)
def test_run_chain_records_loglik_with_the_diagonal(row, kind):
    """rc_run_chain with numMH = 1 against the oracle's loop, as tests/test_gpu_chain.py: recorded loglik and logposterior."""
    D0, truth = _paper(1)
    D = with_diagonal(D0, kind)
    P = rc.likelihood_hyperparams(D0, truth)
    init = truth.copy(); init[init == 2] = 1; init[init == 4] = 3; init[init == 9] = 8
    iters, seed = 16, 4322
    ctx, L_host = _default_context(row, D)
    try:
        ctx.set_params(**P)
        ctx.set_state(init)
        orc, Dq, Lq = _oracle(row, ctx, D, L_host, P)
        ctx.cocluster_reset()
        ctx.attach_host_matrices(D, np.ldexp(Lq.astype(np.float64), -orc.eL))
        ch = ctx.run_chain(iters, 2, 2, 5, 1, seed, 1.0, 0.5, 0.7)
        ref = O.run_chain(orc, init, 1.0, 0.5, iters, 2, 2, 5, 1, seed, proposalsd_r=0.7, stable=True)
        assert ch["num_samples"] == len(ref["K"]) == (iters - 2) // 2
        for got, want in ((ch["r_all"], ref["r_all"]), (ch["p_all"], ref["p_all"]), (ch["clusts"], ref["clusts"]), (ch["K"], ref["K"]),
                          (ch["splitmerge_acceptances"], ref["sm_acc"]), (ch["splitmerge_splits"], ref["sm_split"])):
            assert np.array_equal(got, want)
        assert np.all(np.isfinite(ref["loglik"]))
        assert np.allclose(ch["loglik"], ref["loglik"], rtol=LL_RTOL, atol=0)
        assert np.allclose(ch["logposterior"], ref["logposterior"], rtol=1e-6, atol=0)
        orc0 = O.Oracle(D0, P, logD=orc.logD, eD=orc.eD, eL=orc.eL)                 # the last recorded partition without the diagonal
        orc0.set_state(ref["clusts"][-1])
        assert abs(ch["loglik"][-1] - orc0.loglik_stable()) > 1000 * LL_RTOL * abs(ch["loglik"][-1])
    finally:
        ctx.close()
