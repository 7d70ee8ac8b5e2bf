"""The references at other units of D (-m "not gpu"): tests/units.py's family through the CPU oracle and the NumPy restatements
that tests/test_gpu_units.py compares the device with.  What the GPU tests rely on is pinned here, so that none of them can pass
vacuously: the oracle agrees with the independent transcription, its two log-likelihoods agree far inside the GPU tolerances, the
chains move and stay below the slot capacity the contexts are given, the quantisation is invariant under a power of two, and the
restatements of k-medoids, k-means, predict and predict_joint take every member."""
import numpy as np
import pytest

import kmeans_ref as KM
import kmedoids_ref as KR
import np_transcription as T
import oracle_lib as O
import predict_joint_ref as J
import predict_ref as R
import units as U

MEMBERS = [(name, n) for n in U.SIZES for name in U.NAMES]
IDS = [f"{name}-{n}" for name, n in MEMBERS]


@pytest.mark.parametrize("name", U.NAMES)
def test_family_is_what_it_says(name):
    n = U.SIZES[0]
    D = U.member(name, n)["D"]
    off = D[~np.eye(n, dtype=bool)]
    assert np.array_equal(D, D.T) and not D.diagonal().any() and off.min() > 0
    L = np.log(off)
    if name == "below_one":
        assert off.max() == 0.5 and L.max() < 0
    if name == "near_one":
        assert off.min() == U.NEAR_ONE[0] and off.max() == U.NEAR_ONE[1]
        assert (off < 1.0).sum() > n and (off > 1.0).sum() > n             # both binades around 1.0
        assert np.abs(L).max() < 0.25                                     # where 50 - ex(max |log D|) reaches 52
    if name == "integers":
        vals = np.unique(off)
        assert np.array_equal(vals, np.rint(vals)) and len(vals) <= 6 and {1.0, 2.0, 4.0} <= set(vals)
    if name == "all_ones":
        assert np.all(off == 1.0)
    if U.dyadic_pair(name):                                               # the same mantissas
        of, s = U.dyadic_pair(name)
        m0, e0 = np.frexp(U.member(of, n)["D"])
        m1, e1 = np.frexp(D)
        assert np.array_equal(m0, m1) and np.all((e1 - e0)[m0 > 0] == s)


@pytest.mark.parametrize("name", U.NAMES)
def test_oracle_sweeps_equal_the_transcription(name):
    """two literal sweeps of the C oracle and of np_transcription from the perturbed start, labels exact (n = 333: the
    transcription is a Python loop)"""
    m = U.member(name, U.SIZES[0])
    D, P = m["D"], m["P"]
    o = O.Oracle(D, P)
    o.set_state(m["init"])
    logD = T.make_logD(D)
    clusts = m["init"].copy()
    sizes, K = T.state_from_labels(clusts)
    for t in range(2):
        r, p = U.rp(t)
        K = T.sweep(D, logD, clusts, sizes, P, r, p, U.SEED, t)
        o.sweep_literal(r, p, U.SEED, t)
        assert np.array_equal(clusts, o.clusts) and K == o.K, t
    assert not np.array_equal(clusts, m["init"])


@pytest.mark.parametrize("name,n", MEMBERS, ids=IDS)
def test_chain_conditions_and_the_two_logliks(name, n):
    """Six stable sweeps from the perturbed start: at least 20 labels move and K stays below the contexts' slot capacity, after
    every sweep; loglik_stable and loglik_literal agree within 1e-7 relative (the GPU tests allow 1e-9 against the first and
    1e-6 against the second).  all_ones is exempt from "moves" by its nature — with every distance equal nothing tells two
    clusters apart — though it does move: every point ends in one cluster."""
    m = U.member(name, n)
    o = O.Oracle(m["D"], m["P"])
    o.set_state(m["init"])
    moved = 0
    for t in range(U.NSWEEPS):
        o.sweep_stable(*U.rp(t), U.SEED, t)
        moved += o.last_changes
        assert o.K < U.KCAP, (t, o.K)
        ls, ll = o.loglik_stable(), o.loglik_literal()
        print(name, n, "sweep", t, "K", o.K, "changes", o.last_changes, "|stable - literal| / |literal| =", abs(ls - ll) / abs(ll))
        assert abs(ls - ll) <= 1e-7 * abs(ll), (t, ls, ll)
    if name != "all_ones":
        assert moved >= 20, moved
    if name in U.RESCALED or U.dyadic_pair(name):           # the model is scale-free once the hyperparameters are refitted
        of = U.dyadic_pair(name)[0] if U.dyadic_pair(name) else "base"
        b = O.Oracle(U.member(of, n)["D"], U.member(of, n)["P"])
        b.set_state(m["init"])
        for t in range(U.NSWEEPS):
            b.sweep_stable(*U.rp(t), U.SEED, t)
        assert np.array_equal(b.clusts, o.clusts)


@pytest.mark.parametrize("n", U.SIZES)
@pytest.mark.parametrize("name", [x for x in U.NAMES if U.dyadic_pair(x)])
def test_quantisation_is_invariant_under_a_power_of_two(name, n):
    of, s = U.dyadic_pair(name)
    D0, D = U.member(of, n)["D"], U.member(name, n)["D"]
    a, b = O.Oracle(D0, U.member(of, n)["P"]), O.Oracle(D, U.member(name, n)["P"])
    assert b.eD == a.eD - s and np.array_equal(a.Dq, b.Dq)
    L = O.lib()
    for e in (a.eD, 47 - U.exponent(D0.max()), 30 - U.exponent(D0.max())):      # stored, derived and 32-bit exponents
        q0, q1 = np.empty(n * n, np.int64), np.empty(n * n, np.int64)
        L.orc_quantize(D0.ravel(), n * n, e, q0)
        L.orc_quantize(D.ravel(), n * n, e - s, q1)
        assert np.array_equal(q0, q1) and q0.max() > 2 ** 28
    assert (b.eD < 0) == (s == 60) and (b.eD > 100) == (s == -60)


SM_CASES = [(name, n) for n in U.SIZES for name in ("x1e-6", "x2^60", "near_one")]


@pytest.mark.parametrize("name,n", SM_CASES, ids=[f"{a}-{b}" for a, b in SM_CASES])
def test_splitmerge_leg_has_proposals_of_both_kinds_and_an_accepted_one(name, n):
    """the proposals tests/test_gpu_units.py::test_splitmerge_proposals_then_a_sweep replays, on the oracle with the exponents of
    a stored context (its own)"""
    m = U.member(name, n)
    o = O.Oracle(m["D"], m["P"])
    o.set_state(U.sm_start(n))
    acc, split = [], []
    for it in range(U.SM_PROPOSALS):
        inf = o.mh_proposal(1.0, 0.5, 3, U.SM_SEED, it, 0, mode=1)
        acc.append(bool(inf.accept)); split.append(bool(inf.split))
    o.sweep_stable(1.0, 0.5, U.SM_SEED, 100)
    assert o.K < U.KCAP and o.last_changes > 0
    print(name, n, "accepted", acc, "split", split)
    assert any(split) and not all(split)
    assert any(acc) or n != U.SIZES[0]                      # (at n = 1029 none of the ten is accepted: the ratios are still compared)


@pytest.mark.parametrize("name", U.NAMES)
def test_expected_exponents_are_the_oracles(name):
    """units.expected_exponents (what the GPU tests hold the contexts' exponents against) is the oracle's own rule for the
    stored kinds"""
    for n in U.SIZES:
        m = U.member(name, n)
        for kind, bits in (("stored", 64), ("bits32", 32)):
            o = O.Oracle(m["D"], m["P"], bits=bits)
            assert (o.eD, o.eL) == U.expected_exponents(m["D"], n, kind), (n, kind)
    if name == "all_ones":
        assert U.expected_exponents(m["D"], n, "derived")[1] == 0
    if name == "near_one":
        assert U.expected_exponents(m["D"], U.SIZES[0], "derived")[1] == 54      # log 2 · 2^54 + 1.5 · 2^52 > 2^53


@pytest.mark.parametrize("name", ["x2^-20", "x2^20", "x2^-60", "x2^60"])
def test_kmedoids_restatement_under_a_power_of_two(name):
    """With tol scaled along with D the run is the base's and the costs are exactly ·2^s; with the default tol = 1e-8 the small
    units stop at the first iteration whose cost changes by less than 1e-8 — at 2^-60 every change is — and the large ones
    never stop early."""
    n, s = U.SIZES[0], U.DYADIC[name]
    D0, D = U.member("base", n)["D"], U.member(name, n)["D"]
    e0 = 47 - U.exponent(D0.max())
    q = np.rint(np.ldexp(D0, e0)).astype(np.int64)
    assert np.array_equal(q, np.rint(np.ldexp(D, e0 - s)).astype(np.int64))
    for k in (3, 17):
        a = KR.kmedoids(q, e0, k, seed=5)
        b = KR.kmedoids(q, e0 - s, k, tol=1e-8 * 2.0 ** s, seed=5)
        assert a["iterations"] > 1 and a["converged"]
        for f in ("medoids", "assignments"):
            assert np.array_equal(a[f], b[f])
        assert a["iterations"] == b["iterations"] and b["totalcost"] == a["totalcost"] * 2.0 ** s
        d = KR.kmedoids(q, e0 - s, k, seed=5)
        if s == -60:
            assert d["iterations"] == 1 and d["converged"]
        if s > 0:
            assert d["iterations"] == a["iterations"]


@pytest.mark.parametrize("name", list(U.RESCALED))
def test_kmeans_restatement_on_rescaled_points(name):
    """k-means on points·c: for c a power of two every step is the base's, scaled exactly (tol scaled by c²)"""
    c = U.RESCALED[name]
    X = U.base(U.SIZES[0])["points"]
    a = KM.kmeans(X, 5, seed=7)
    b = KM.kmeans(X * c, 5, tol=1e-6 * c * c, seed=7)
    assert a["iterations"] > 1 and a["converged"] and b["converged"]
    if name in U.DYADIC:
        assert np.array_equal(a["assignments"], b["assignments"]) and a["iterations"] == b["iterations"]
        assert np.array_equal(a["centers"] * c, b["centers"]) and b["totalcost"] == a["totalcost"] * c * c
    d = KM.kmeans(X * c, 5, seed=7)                       # the default tol = 1e-6, in units of D²
    assert d["iterations"] >= 1 and np.all(d["counts"] > 0)
    if c < 1:
        assert d["iterations"] <= b["iterations"]


def test_predict_references_take_rows_of_every_unit():
    """predict_ref and predict_joint_ref on units.predict_case: the per-row exponents follow the formula (0 for the row of ones,
    negative for none), and the decision gaps stay above 1e-6 — the device's scores deviate by 2^-49 of their terms — so that
    the GPU tests may ask for equal labels."""
    c = U.predict_case()
    n, q = c["Dnew"].shape[1], c["Dnew"].shape[0]
    ref = R.predict_ref(c["Dnew"], c["logDnew"], c["samples"], c["r"], c["p"], c["P"], c["seed"])
    eD, eL = U.row_exponents(c["Dnew"], c["logDnew"], n)
    assert np.array_equal(ref["eD"], eD) and np.array_equal(ref["eL"], eL)
    assert eL[2] == 0 and eD[1] == eD[0] - 20 and eD[4] >= eD[0] + 59 and eL[3] >= 62 - U.ceil_log2(n) + 4
    print("predict gaps", ref["min_gap_noisy"], ref["min_gap_map"], "eD", eD, "eL", eL)
    assert ref["min_gap_noisy"] > 1e-6 and ref["min_gap_map"] > 1e-6
    assert len(np.unique(ref["labels"])) > 3                                   # the draws differ between points and samples
    jref = J.predict_joint_ref(c["Dnew"], c["Dnn"], c["logDnew"], c["logDnn"], c["samples"], c["r"], c["p"], c["P"], c["sweeps"], c["seed"])
    rows = np.concatenate([c["Dnew"], c["Dnn"]], axis=1)
    lrows = np.concatenate([c["logDnew"], c["logDnn"]], axis=1)
    eDj, eLj = U.row_exponents(rows, lrows, n + q)
    assert np.array_equal(jref["eD"], eDj) and np.array_equal(jref["eL"], eLj) and eLj[2] == 0
    print("joint gap", jref["min_gap_noisy"], "eD", eDj, "eL", eLj, "moves", jref["moves"].sum(axis=0))
    assert jref["min_gap_noisy"] > 1e-6
    assert eLj[3] >= 62 - U.ceil_log2(n + q) + 4 and eDj[1] == eDj[0] - 20
    assert jref["moves"][:, 0].min() == q and jref["moves"][:, 1:].sum() > 0 and len(np.unique(jref["labels"])) > 3
