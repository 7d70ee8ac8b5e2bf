"""Distance matrices in other units on the device (-m gpu): tests/units.py's family — D0 times 2^±20, 1e±6, 2^±60, every entry
below one, every entry within 6 % of one (and that matrix at 2^±60), small integers, all ones — through every kind of context
(derived logD, stored logD, 32-bit storage, and from points for the pure rescalings) at n = 333 and n = 1029.

Every exponent the library chooses from the magnitude of the matrix ("Units of D") is held against the formula, the
ingested matrices against the host's, the row-sum table, six sweeps in both modes, split–merge and one rc_run_chain leg against the
CPU oracle — which is handed the device's logD and exponents, as tests/test_gpu_derived_log.py does — and every consumer of the
context's matrices against the reference module it already has.  tests/test_units_cpu.py pins the references at these units: the
chains move, K stays below the contexts' slot capacity, the oracle's own two log-likelihoods agree far inside the tolerances here.

A member that is another one times 2^s (units.dyadic_pair) must hold the very same fixed-point integers with eD lower by s.
"""
import numpy as np
import pytest

import bulk_rows as B
import kmeans_ref as KM
import kmedoids_ref as KR
import oracle_lib as O
import predict_joint_ref as J
import predict_ref as R
import redclust_amd as rc
import score_ref as SR
import units as U
from helpers import assert_derived_log_close
from redclust_amd import _lib
from test_gpu_kmeans import assert_same as assert_same_kmeans
from test_gpu_kmedoids import assert_same as assert_same_kmedoids
from test_gpu_predict import _check_against_reference as check_predict
from test_gpu_profiles import check as check_profiles
from test_gpu_score import check as check_score

pytestmark = pytest.mark.gpu

KINDS = ("derived", "stored", "bits32")
POINT_NAMES = ("base",) + tuple(U.RESCALED)
SETUPS = [(name, kind, n) for n in U.SIZES for name in U.NAMES for kind in KINDS] + \
         [(name, "points", n) for n in U.SIZES for name in POINT_NAMES]
SMALL = U.SIZES[0]


def make_context(name, kind, n, kcap=U.KCAP):
    m = U.member(name, n)
    with B.environment():                                     # none of the library's switches
        if kind == "points":
            return rc.Context.from_points(U.base(n)["points"] * m["scale"], kcap=kcap)
        if kind == "derived":
            return rc.Context(m["D"], kcap=kcap)
        return rc.Context(m["D"], logD=U.host_log(m["D"]), kcap=kcap, storage_bits=32 if kind == "bits32" else 64)


def is_derived(kind):
    return kind in ("derived", "points")


class Setup:
    """one context with parameters and the perturbed start set, and the oracle on the device's logD and exponents"""

    def __init__(self, name, kind, n):
        m = U.member(name, n)
        self.name, self.kind, self.n, self.m, self.P, self.init = name, kind, n, m, m["P"], m["init"]
        self.ctx = make_context(name, kind, n)
        self.ctx.set_params(**self.P)
        self.ctx.set_state(self.init)
        self.Ddev, self.L = self.ctx.get_matrix(0), self.ctx.get_matrix(1)
        self.eD, self.eL = self.ctx.debug_rowsums(int(self.init[0]))[2:4]
        self.D = self.Ddev if kind == "points" else m["D"]     # (from points: the device's distances are the data)
        self.orc = O.Oracle(self.D, self.P, logD=self.L, bits=32 if kind == "bits32" else 64, eL=self.eL, eD=self.eD)
        self.orc.set_state(self.init)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module", params=SETUPS, ids=[f"{a}-{b}-{c}" for a, b, c in SETUPS])
def S(request):
    s = Setup(*request.param)
    yield s
    s.close()


def rowsum_table(ctx, labels):
    return [ctx.debug_rowsums(int(k))[:2] for k in np.unique(labels)]


def assert_tables_equal(a, b, what, side=(0, 1)):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        for w in side:
            assert np.array_equal(x[w], y[w]), what


# ---------------------------------------------------------------------------------------------------------------
# ingestion
# ---------------------------------------------------------------------------------------------------------------
def test_ingestion(S):
    n, D, hostD = S.n, S.D, S.m["D"]
    quantum = np.ldexp(1.0, -S.eD)
    assert np.all(np.abs(S.Ddev - D) <= quantum / 2), float(np.max(np.abs(S.Ddev - D)) / quantum)
    if S.kind == "points":
        # k_pairwise and the host both take |a|² + |b|² - 2 a·b: a dozen roundings of 2^-53 of the squared norms (below 4·scale²)
        # each, halved and divided by a distance of 0.1·scale at the least — far below 1e-12·scale
        assert np.all(np.abs(S.Ddev - hostD) <= 1e-12 * S.m["scale"]), float(np.max(np.abs(S.Ddev - hostD)))
    Dq = B.quantise(S.Ddev, S.eD)
    assert np.array_equal(Dq, S.orc.Dq) and np.array_equal(np.ldexp(Dq.astype(np.float64), -S.eD), S.Ddev)
    want = U.expected_exponents(D, n, "derived" if is_derived(S.kind) else S.kind)
    assert (S.eD, S.eL) == want, (S.eD, S.eL, want)
    assert (S.eD, S.eL) == (S.orc.eD, S.orc.eL)
    folded = S.ctx.log_table_folded()
    assert folded == (is_derived(S.kind) and B.binades(Dq) <= 4), (folded, B.binades(Dq))
    ratio = float("nan")
    if is_derived(S.kind):
        worst, ratio = assert_derived_log_close(S.L, D, S.eD, S.eL)
        assert np.array_equal(S.L, S.L.T)
    else:
        assert np.all(np.abs(S.L - U.host_log(D)) <= np.ldexp(1.0, -S.eL - 1))
        assert np.all(np.diag(S.L) == 0.0)
    if S.name == "all_ones":
        assert S.eL == 0 and not S.L.any() and not S.orc.Lq.any()
    if S.name == "below_one":
        assert S.orc.Lq.max() == 0 and S.orc.Lq[~np.eye(n, dtype=bool)].max() < 0
    print(f"UNITS {S.name!r} {S.kind} n={n} eD={S.eD} eL={S.eL} folded={folded} binades={B.binades(Dq)} "
          f"max|L-logD|/bound={ratio:.3g}")
    pair = U.dyadic_pair(S.name)
    if pair:
        other = Setup(pair[0], S.kind, n)
        try:
            assert S.eD == other.eD - pair[1]
            assert np.array_equal(S.orc.Dq, other.orc.Dq)
            assert_tables_equal(rowsum_table(S.ctx, S.init), rowsum_table(other.ctx, S.init), "D-side row sums of a dyadic pair", side=(0,))
        finally:
            other.close()


KERNELS = ("perm", "sym")      # rc_set_bulk_kernel: the full-read kernel and the context's symmetric one — for a derived context
#                                k_bulk_syml2, which at these sizes no automatic choice reaches and which alone reads the folded log table


def symmetric_kernel_of(kind):
    return {"derived": "k_bulk_syml2<true, true>", "points": "k_bulk_syml2<true, true>", "stored": "k_bulk_sym<false>", "bits32": "k_bulk_sym32"}[kind]


def test_row_sums_of_both_matrices_are_the_oracles_integers(S):
    S.ctx.set_mode("full")
    onehot = (S.init[:, None] == np.arange(1, U.K + 1)[None, :]).astype(np.int64)
    refD, refL = S.orc.Dq @ onehot, S.orc.Lq @ onehot
    for kernel in KERNELS + ("auto",):
        S.ctx.set_bulk_kernel(kernel)
        S.ctx.set_state(S.init)
        for k in range(1, U.K + 1):
            sd, sl, eD, eL = S.ctx.debug_rowsums(k)
            assert (eD, eL) == (S.eD, S.eL)
            assert np.array_equal(sd, refD[:, k - 1]), (kernel, k)
            assert np.array_equal(sl, refL[:, k - 1]), (kernel, k)
    td, tl = S.ctx.debug_rowtotals()
    assert np.array_equal(td, S.orc.Dq.sum(axis=1)) and np.array_equal(tl, S.orc.Lq.sum(axis=1))
    w = S.ctx.within_between()                                # rtol as tests/test_gpu_parity.py::test_within_between_split_from_block_sums
    iu = np.triu_indices(S.n, 1)
    same = (S.init[:, None] == S.init[None, :])[iu]
    assert w["count_within"] == int(same.sum()) and w["count_between"] == int((~same).sum())
    # the matrices as the context holds them, and the host's — which 32-bit storage rounds to half a quantum per entry
    qD, qL = (np.ldexp(0.5, -S.eD), np.ldexp(0.5, -S.eL)) if S.kind == "bits32" else (0.0, 0.0)
    for Dm, Lm, fD, fL in ((S.Ddev, S.L, 0.0, 0.0), (S.D, U.host_log(S.D), qD, qL)):
        for key, M, sel, rtol, f in (("sum_within", Dm, same, 1e-12, fD), ("sum_between", Dm, ~same, 1e-12, fD),
                                     ("sumlog_within", Lm, same, 1e-10, fL), ("sumlog_between", Lm, ~same, 1e-10, fL)):
            ref = M[iu][sel].sum()
            assert abs(w[key] - ref) <= rtol * abs(ref) + f * int(sel.sum()), (key, w[key], ref)


# ---------------------------------------------------------------------------------------------------------------
# sweeps
# ---------------------------------------------------------------------------------------------------------------
def run_sweeps(S, ctx, mode, kernel):
    orc = S.orc
    ctx.set_bulk_kernel(kernel)
    ctx.set_state(S.init)
    ctx.set_mode(mode)
    orc.set_state(S.init)
    moved, names = 0, set()
    for t in range(U.NSWEEPS):
        r, p = U.rp(t)
        ctx.gibbs_sweep(r, p, U.SEED, t)
        names.add(ctx.bulk_kernel_name())
        orc.sweep_stable(r, p, U.SEED, t)
        lab, sizes, K = ctx.get_state()
        assert np.array_equal(lab, orc.clusts), (mode, kernel, t, int(np.sum(lab != orc.clusts)))
        assert np.array_equal(sizes, orc.sizes) and K == orc.K, (mode, kernel, t)
        st = ctx.sweep_stats()
        assert st["n_changes"] == orc.last_changes and st["K"] == orc.K, (mode, kernel, t, st, orc.last_changes)
        moved += st["n_changes"]
    if kernel == "sym" and mode == "full":                    # (incremental mode launches no row reduction after the first)
        assert names == {symmetric_kernel_of(S.kind)}, names
    ll, ref, lit = ctx.loglik(), orc.loglik_stable(), orc.loglik_literal()
    print(f"{S.name!r} {S.kind} n={S.n} {mode} {kernel}: moved {moved}, K {orc.K}, loglik rel. to stable {abs(ll - ref) / abs(ref):.3g}, "
          f"to literal {abs(ll - lit) / abs(lit):.3g}")
    assert abs(ll - ref) <= 1e-9 * abs(ref), (ll, ref)
    assert abs(ll - lit) <= 1e-6 * abs(lit), (ll, lit)
    lit_host = O.lib().orc_loglik_literal(S.n, np.ascontiguousarray(S.D).reshape(-1), U.host_log(S.D).reshape(-1), orc.clusts, orc.sizes, orc.P)
    assert abs(ll - lit_host) <= 1e-6 * abs(lit_host), (ll, lit_host)
    lp = ctx.logprior(*U.rp(U.NSWEEPS - 1))
    assert abs(lp - orc.logprior(*U.rp(U.NSWEEPS - 1))) <= 1e-12 * abs(lp)
    assert S.name == "all_ones" or moved >= 20
    table = rowsum_table(ctx, orc.clusts)
    ref_table = [(orc.Dq[:, orc.clusts == k].sum(axis=1), orc.Lq[:, orc.clusts == k].sum(axis=1)) for k in np.unique(orc.clusts)]
    assert_tables_equal(table, ref_table, (mode, kernel, "row sums after the sweeps"))
    return ll, table


def test_six_sweeps_in_both_modes_against_the_oracle(S):
    """full and incremental mode, through the full-read and the symmetric row reduction; a derived context once more with
    "fold_log_table" 0 (k_bulk_syml2w, which derives the exponent per entry): the same integers"""
    try:
        runs = [run_sweeps(S, S.ctx, mode, kernel) for kernel in KERNELS for mode in ("full", "incremental")]
    finally:
        S.ctx.set_mode("full"); S.ctx.set_bulk_kernel("auto")
    if is_derived(S.kind):
        other = make_context(S.name, S.kind, S.n)
        try:
            other.set_option("fold_log_table", 0)
            other.set_params(**S.P)
            assert not other.log_table_folded()
            runs.append(run_sweeps(S, other, "full", "sym"))
        finally:
            other.close()
    for ll, table in runs[1:]:
        assert ll == runs[0][0]
        assert_tables_equal(table, runs[0][1], "row sums of two kernels / modes")


SM_CASES = [(name, kind, n) for n in U.SIZES for name in ("x1e-6", "x2^60", "near_one") for kind in KINDS]


@pytest.mark.parametrize("name,kind,n", SM_CASES, ids=[f"{a}-{b}-{c}" for a, b, c in SM_CASES])
def test_splitmerge_proposals_then_a_sweep(name, kind, n):
    """as tests/test_gpu_parity.py::test_incremental_mode_is_bit_identical: proposals against orc.mh_proposal(mode=1), then a
    sweep, from units.sm_start (tests/test_units_cpu.py: proposals of both kinds, at n = 333 accepted ones among them)"""
    s = Setup(name, kind, n)
    try:
        ctx, orc = s.ctx, s.orc
        start = U.sm_start(n)
        ctx.set_state(start); orc.set_state(start)
        ctx.set_mode("incremental")
        ctx.attach_host_matrices(s.D, s.L)
        accepted, splits = 0, 0
        for it in range(U.SM_PROPOSALS):
            inf = orc.mh_proposal(1.0, 0.5, 3, U.SM_SEED, it, 0, mode=1)
            got = ctx.splitmerge(1.0, 0.5, 3, U.SM_SEED, it, 0)
            assert got == (bool(inf.accept), bool(inf.split)), (it, got, inf.accept, inf.split)
            accepted += got[0]; splits += got[1]
            assert np.array_equal(ctx.get_state()[0], orc.clusts), it
        assert 0 < splits < U.SM_PROPOSALS and (accepted >= 1 or n != SMALL)
        ctx.gibbs_sweep(1.0, 0.5, U.SM_SEED, 100); orc.sweep_stable(1.0, 0.5, U.SM_SEED, 100)
        lab, sizes, K = ctx.get_state()
        assert np.array_equal(lab, orc.clusts) and np.array_equal(sizes, orc.sizes) and K == orc.K
        assert ctx.sweep_stats()["n_changes"] == orc.last_changes > 0
        table = rowsum_table(ctx, orc.clusts)                 # the table kept by corrections through proposals and the sweep
        ref_table = [(orc.Dq[:, orc.clusts == k].sum(axis=1), orc.Lq[:, orc.clusts == k].sum(axis=1)) for k in np.unique(orc.clusts)]
        assert_tables_equal(table, ref_table, "row sums after split-merge and a sweep")
        ref = orc.loglik_stable()
        assert abs(ctx.loglik() - ref) <= 1e-9 * abs(ref)
    finally:
        s.close()


@pytest.mark.parametrize("kind", ["derived", "stored"])
@pytest.mark.parametrize("name", ["x1e6", "near_one"])
def test_one_run_chain_leg(name, kind):
    """as tests/test_gpu_chain.py::test_free_running_chain_vs_oracle_and_golden: the native loop against oracle_lib.run_chain"""
    s = Setup(name, kind, SMALL)
    try:
        ctx, orc, init = s.ctx, s.orc, s.init
        ctx.cocluster_reset()
        ctx.attach_host_matrices(s.D, s.L)
        iters, burnin, thin, numMH, seed = 30, 4, 2, 1, 515
        ch = ctx.run_chain(iters, burnin, thin, 5, numMH, seed, 1.0, 0.5, 0.7)
        ref = O.run_chain(orc, init, 1.0, 0.5, iters, burnin, thin, 5, numMH, seed, proposalsd_r=0.7, stable=True)
        assert ch["num_samples"] == len(ref["K"]) == (iters - burnin) // thin
        for got, want in ((ch["r_all"], ref["r_all"]), (ch["p_all"], ref["p_all"]), (ch["r"], ref["r"]), (ch["p"], ref["p"]),
                          (ch["clusts"], ref["clusts"]), (ch["K"], ref["K"]), (ch["r_acceptances"], ref["r_acc"]),
                          (ch["splitmerge_acceptances"], ref["sm_acc"]), (ch["splitmerge_splits"], ref["sm_split"])):
            assert np.array_equal(got, want)
        assert np.allclose(ch["loglik"], ref["loglik"], rtol=1e-9, atol=0)
        assert np.allclose(ch["logposterior"], ref["logposterior"], rtol=1e-6, atol=0)
        assert len(np.unique(ch["clusts"], axis=0)) > 1                       # the chain moves
        lab, _, K = ctx.get_state()
        assert np.array_equal(lab, orc.clusts) and K == orc.K
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------
# consumers of the context's matrices (n = 333)
# ---------------------------------------------------------------------------------------------------------------
CONSUMER_CASES = [(name, "derived") for name in U.NAMES] + \
                 [(name, kind) for name in ("x2^-60", "x2^60", "below_one", "near_one") for kind in ("stored", "bits32")] + \
                 [(name, "points") for name in ("x2^-60", "x1e6")]
CONSUMER_IDS = [f"{a}-{b}" for a, b in CONSUMER_CASES]


def labellings(n):
    """the truth, the perturbed start, one cluster, all singletons, twelve sparse names"""
    b = U.base(n)
    rng = np.random.default_rng(5)
    return np.stack([b["truth"], b["init"], np.full(n, 7), rng.permutation(n) + 1,
                     (rng.choice(n, 12, replace=False) + 1)[rng.integers(0, 12, n)]]).astype(np.int64)


@pytest.mark.parametrize("name,kind", CONSUMER_CASES, ids=CONSUMER_IDS)
def test_kmedoids_default_and_scaled_tolerance(name, kind):
    """tol is in units of D: the default 1e-8 is binding at small units (the run stops while the cost still falls) and never at
    large ones; scaled along with D the run is the base's.  Both against the restatement; a dyadic member with the scaled tol has
    the base's medoids and assignments and its costs times 2^s exactly."""
    ctx = make_context(name, kind, SMALL)
    try:
        Dq, eD = KR.device_matrix(ctx)
        scale = float(U.member(name, SMALL)["D"].max() / U.member("base", SMALL)["D"].max())
        kmin, kmax, seed = 1, 17, 5
        for tol in (1e-8, 1e-8 * scale):
            scan = ctx.kmedoids_scan(kmin, kmax, tol=tol, seed=seed)
            for k in range(kmin, kmax + 1):
                ref = KR.kmedoids(Dq, eD, k, tol=tol, seed=seed)
                assert scan["totalcost"][k - kmin] == ref["totalcost"] and scan["iterations"][k - kmin] == ref["iterations"], (tol, k)
                assert bool(scan["converged"][k - kmin]) == ref["converged"], (tol, k)
                if k in (3, 17):
                    assert_same_kmedoids(ctx.kmedoids(k, tol=tol, seed=seed), ref)
        pair = U.dyadic_pair(name)
        if pair:
            other = make_context(pair[0], kind, SMALL)
            try:
                s = pair[1]
                for k in (3, 17):                                              # (tests/test_units_cpu.py: the same on the restatement)
                    a, b = other.kmedoids(k, seed=seed), ctx.kmedoids(k, tol=1e-8 * 2.0 ** s, seed=seed)
                    assert np.array_equal(a.medoids, b.medoids) and np.array_equal(a.assignments, b.assignments)
                    assert a.iterations == b.iterations > 1 and a.converged == b.converged
                    assert b.totalcost == a.totalcost * 2.0 ** s
                    d = ctx.kmedoids(k, seed=seed)                             # the default: binding at once, or never
                    if s == -60:
                        assert d.iterations == 1 and d.converged
                    if s > 0:
                        assert d.iterations == a.iterations
            finally:
                other.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", POINT_NAMES)
def test_kmeans_on_rescaled_points(name):
    c = U.member(name, SMALL)["scale"]
    X = U.base(SMALL)["points"] * c
    ctx = rc.Context.from_points(X)
    try:
        for k, seed in ((1, 7), (5, 7), (17, (1 << 32) + 12345678901)):
            for tol in (1e-6, 1e-6 * c * c):
                assert_same_kmeans(ctx.kmeans(k, tol=tol, seed=seed), KM.kmeans(X, k, tol=tol, seed=seed))
        scan = ctx.kmeans_scan(1, 9, tol=1e-6 * c * c, seed=3)
        for k in range(1, 10):
            ref = KM.kmeans(X, k, tol=1e-6 * c * c, seed=3)
            assert scan["totalcost"][k - 1] == ref["totalcost"] and scan["iterations"][k - 1] == ref["iterations"], k
    finally:
        ctx.close()


@pytest.mark.parametrize("name,kind", CONSUMER_CASES, ids=CONSUMER_IDS)
def test_score_blocks_and_loglik(name, kind):
    """tests/test_gpu_score.py's check: blocks equal score_ref's integers (below_one: every log block negative), loglik and
    logprior bit for bit what set_state + loglik / logprior return on a second context"""
    ctx, twin = make_context(name, kind, SMALL), make_context(name, kind, SMALL)
    try:
        P = U.member(name, SMALL)["P"]
        ctx.set_params(**P); twin.set_params(**P)
        labs = labellings(SMALL)
        out = check_score(ctx, twin, labs)
        assert np.all(np.isfinite(out["loglik"]))
        if name == "below_one":
            for l in range(len(labs)):
                assert all(v[1] < 0 for v in SR.values(out["blocks"][l]) if v[1] != 0)
            assert any(v[1] < 0 for v in SR.values(out["blocks"][0]))
        if name == "all_ones":
            assert all(v[1] == 0 for l in range(len(labs)) for v in SR.values(out["blocks"][l]))
    finally:
        ctx.close(); twin.close()


@pytest.mark.parametrize("name,kind", CONSUMER_CASES, ids=CONSUMER_IDS)
def test_profiles(name, kind):
    ctx = make_context(name, kind, SMALL)
    try:
        labs = labellings(SMALL)
        out, Dq = check_profiles(ctx, labs)
        assert int(out["nearest"][0].astype(object).max()) * SMALL < 1 << 127
        pair = U.dyadic_pair(name)
        if pair:
            other = make_context(pair[0], kind, SMALL)
            try:
                ref = other.profiles(labs)
                assert out["eD"] == ref["eD"] - pair[1]
                for f in ("K", "within", "nearest", "neighbour"):
                    assert np.array_equal(out[f], ref[f]), f
                for f in ("labels", "sizes", "medoids", "medoid_within"):
                    assert all(np.array_equal(x, y) for x, y in zip(out[f], ref[f])), f
                a, b = rc.clusterprofiles(ctx, labs), rc.clusterprofiles(other, labs)
                assert np.array_equal(a.silhouette, b.silhouette) and np.array_equal(a.mean_silhouette, b.mean_silhouette)
                assert all(np.array_equal(x * 2.0 ** -pair[1], y) for x, y in zip(a.within_mean, b.within_mean))
                assert np.count_nonzero(a.silhouette[0]) > SMALL // 2              # (not a comparison of zeros)
            finally:
                other.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# new observations: per-row exponents computed on the host
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predict_case():
    return U.predict_case()


@pytest.mark.parametrize("given_logs", [True, False])
def test_predict_rows_in_units_of_their_own(predict_case, given_logs):
    c = predict_case
    n = c["Dnew"].shape[1]
    ref = R.predict_ref(c["Dnew"], c["logDnew"], c["samples"], c["r"], c["p"], c["P"], c["seed"])
    out = _lib.predict(c["Dnew"], c["samples"], c["r"], c["p"], c["P"], seed=c["seed"], Kmax=ref["Kmax"], want_scores=True,
                       want_sums=True, logDnew=c["logDnew"] if given_logs else None)
    eD, eL = U.row_exponents(c["Dnew"], c["logDnew"], n)
    assert np.array_equal(out["eD"], eD) and np.array_equal(out["eL"], eL) and out["eL"][2] == 0
    if given_logs:
        check_predict(out, ref)
    else:
        # the library's own logarithms (libm) against NumPy's: each of the n addends of S_L may move by one quantum — the integers
        # of D, the row of ones (no logarithm to round) and, by the decision gaps tests/test_units_cpu.py keeps, the labels are equal
        assert np.array_equal(out["sums"][..., 0], ref["sums"][..., 0])
        assert np.array_equal(out["sums"][:, 2], ref["sums"][:, 2])
        assert np.max(np.abs(out["sums"][..., 1] - ref["sums"][..., 1])) <= n
        assert np.array_equal(out["labels"], ref["labels"]) and np.array_equal(out["map"], ref["map"])


@pytest.mark.parametrize("given_logs", [True, False])
def test_predict_joint_rows_in_units_of_their_own(predict_case, given_logs):
    c = predict_case
    q, n = c["Dnew"].shape
    ref = J.predict_joint_ref(c["Dnew"], c["Dnn"], c["logDnew"], c["logDnn"], c["samples"], c["r"], c["p"], c["P"], c["sweeps"], c["seed"])
    out = _lib.predict_joint(c["Dnew"], c["Dnn"], c["samples"], c["r"], c["p"], c["P"], sweeps=c["sweeps"], seed=c["seed"], want_sums=True,
                             logDnew=c["logDnew"] if given_logs else None, logDnn=c["logDnn"] if given_logs else None)
    eD, eL = U.row_exponents(np.concatenate([c["Dnew"], c["Dnn"]], axis=1), np.concatenate([c["logDnew"], c["logDnn"]], axis=1), n + q)
    assert np.array_equal(out["eD"], eD) and np.array_equal(out["eL"], eL) and out["eL"][2] == 0
    for k in ("labels", "first", "K", "moves") + (("sums",) if given_logs else ()):
        assert np.array_equal(out[k], ref[k]), k
    assert np.array_equal(out["sums"][..., 0], ref["sums"][..., 0])
    assert np.max(np.abs(out["sums"][..., 1] - ref["sums"][..., 1])) <= (0 if given_logs else n + q)
