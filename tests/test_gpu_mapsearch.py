"""The MAP search on the device (-m gpu): rc_map_search through Context.map_search, and searchmapestimate built on it.

Every fixed input of tests/map_search_ref.py runs on the three default kinds of context (derived log, stored 64-bit, 32-bit).
The reference is run on the integers that very context holds (score_ref.quantised of get_matrix), once per (input, kind) and
shared by the tests; tests/test_mapsearch_cpu.py holds its decision gaps above 1e-6 on the host's quantisation, and the same
guard is asserted here on the context's.  The kernel's floating point decides moves only, so labels and records are compared
exactly; the kernel's own block cells against rc_score_labellings' blocks as integers; the reported numbers against
scorelabellings bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import map_search_ref as R
import score_ref as SR

pytestmark = pytest.mark.gpu

KINDS = ("derived64", "stored64", "bits32")
ARG, STATE, CAP = -1, -5, -6


def make_context(kind, D):
    if kind == "derived64":
        return rc.Context(D)
    off = D.copy()
    np.fill_diagonal(off, 1.0)
    return rc.Context(D, logD=np.log(off), storage_bits=32 if kind == "bits32" else 64)


def integers(ctx):
    """(Dq, Lq, eD, eL) of a context, caller's order"""
    sc = ctx.score(np.ones(ctx.n, np.int64))
    return SR.quantised(ctx.get_matrix(0), sc["eD"]), SR.quantised(ctx.get_matrix(1), sc["eL"]), sc["eD"], sc["eL"]


def run_on(ctx, c, **kw):
    return ctx.map_search(c["init"], c["order"], c["r"], c["p"], maxK=c["maxK"], maxsweeps=c["maxsweeps"], want_state=True, **kw)


@pytest.fixture(scope="module")
def solved():
    """(case, context, the device's result, the reference's runs) per (input, kind): computed once, contexts closed at the end"""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            c = R.case(name)
            ctx = make_context(kind, c["D"])
            ctx.set_params(**c["P"])
            res = run_on(ctx, c)
            cache[name, kind] = (c, ctx, res, R.run_case(c, *integers(ctx)))
        return cache[name, kind]
    yield get
    for _, ctx, _, _ in cache.values():
        ctx.close()


def assert_equal_to_reference(res, refs):
    for q, ref in enumerate(refs):
        assert ref["min_gap"] > 1e-6, (q, ref["min_gap"])
        got = {k: int(res[k][q]) for k in ("sweeps", "moves", "K", "converged", "capped")}
        want = {k: int(ref[k]) for k in got}
        assert got == want, (q, got, want)
        assert np.array_equal(res["labels"][q], ref["labels"]), q
        assert np.array_equal(res["slots"][q], ref["slots"]), q


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", R.CASES)
def test_labels_and_records_equal_the_reference(solved, name, kind):
    c, _, res, refs = solved(name, kind)
    assert_equal_to_reference(res, refs)
    if name == "maxK3":
        assert np.all(res["K"] == 3) and np.all(res["capped"] == 0)      # an explicit cap is not counted
        assert solved("n130", kind)[2]["K"][0] > 3                       # ... and it is below what the free run wants
    if name == "capped":
        assert res["K"][0] == 1024 == res["Kcap"] and res["capped"][0] == 76
    if name == "n130":
        assert res["K"][4] < 64 < 130                                    # the singletons start crossed 64 slots and emptied most
    if name == "n1025":
        assert res["sweeps"][0] == 2 and not res["converged"][0]


def kernel_values(blocks):
    """the Kcap×Kcap×4 cells of one run as two Kcap×Kcap object arrays of Python integers (D, L)"""
    b = blocks.astype(object)
    return b[:, :, 0] * (1 << SR.LO_BITS) + b[:, :, 1], b[:, :, 2] * (1 << SR.LO_BITS) + b[:, :, 3]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", R.CASES)
def test_the_incremental_blocks_equal_the_scored_ones(solved, name, kind):
    """A wrong commit shows here even where the labels agree: the kernel's final cells, turned into integers, against the blocks
    rc_score_labellings reduces from scratch for labels_out, for every ordered pair of slots; the cells of empty slots are 0."""
    c, ctx, res, _ = solved(name, kind)
    sc = ctx.score(res["labels"], want_blocks=True)
    for q in range(len(res["labels"])):
        lab, slots, K = res["labels"][q], res["slots"][q], int(res["K"][q])
        slot_of = np.zeros(K + 1, np.int64)
        slot_of[lab] = slots                                             # label (1..K, ascending = score's order) -> kernel slot
        assert len(set(slot_of[1:])) == K and slot_of[1:].min() >= 1
        VD, VL = kernel_values(res["blocks"][q])
        want = SR.values(sc["blocks"][q])
        wD, wL = np.zeros((K, K), object), np.zeros((K, K), object)
        iu = np.triu_indices(K)
        wD[iu] = [v[0] for v in want]; wL[iu] = [v[1] for v in want]
        wD.T[iu] = wD[iu]; wL.T[iu] = wL[iu]
        s = slot_of[1:] - 1
        assert np.array_equal(VD[np.ix_(s, s)], wD) and np.array_equal(VL[np.ix_(s, s)], wL), q
        empty = np.setdiff1d(np.arange(res["Kcap"]), s)
        assert not VD[empty, :].any() and not VD[:, empty].any() and not VL[empty, :].any() and not VL[:, empty].any(), q


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", R.CASES)
def test_reported_numbers_are_those_of_scorelabellings(solved, name, kind):
    c, ctx, res, _ = solved(name, kind)
    for q in range(len(res["labels"])):
        sc = rc.scorelabellings(ctx, res["labels"][q], None, c["r"][q], c["p"][q])
        assert res["loglik"][q] == sc["loglik"][0] and res["logprior"][q] == sc["logprior"][0], q
        assert res["logposterior"][q] == sc["logposterior"][0], q
        if c["init"][q].all():
            st = rc.scorelabellings(ctx, c["init"][q], None, c["r"][q], c["p"][q])
            assert res["start_logposterior"][q] == st["logposterior"][0], q
            assert res["logposterior"][q] >= res["start_logposterior"][q], q
        else:
            assert math.isnan(res["start_logposterior"][q]), q
    assert res["best"] == int(np.argmax(res["logposterior"]))            # the first maximum
    assert res["kernel_ms"] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_search_is_never_worse_than_mapestimate(kind):
    c = R.case("n130")
    ctx = make_context(kind, c["D"])
    try:
        ctx.set_params(**c["P"])
        rng = np.random.default_rng(5)
        truth = c["init"][1]
        cands = np.stack([np.where(rng.random(130) < f, rng.integers(1, 8, 130), truth) for f in (0.0, 0.1, 0.3, 0.5, 0.1, 0.9)] + [truth])
        best, mi = rc.mapestimate(ctx, cands, None, 1.5, 0.1)
        clust, info = rc.searchmapestimate(ctx, cands, None, 1.5, 0.1, nruns=3, seed=2)
        assert len(info["runs"]) == 4 and not info["runs"][-1].any()     # the three best distinct candidates, then empty labels
        assert sum(np.array_equal(x, truth) for x in info["runs"]) <= 1  # the planted labelling is there twice: one start
        assert info["index"] == mi["index"] and np.array_equal(info["candidate_logposterior"], mi["logposterior"])
        assert np.array_equal(info["runs"][0], best)
        # the planted labelling is no mode under these parameters, so the climb gains; what comes back scores as reported
        assert info["best"] >= 0 and info["logposterior"][info["best"]] > mi["logposterior"][mi["index"]]
        assert np.all(info["logposterior"][:3] >= info["start_logposterior"][:3]) and math.isnan(info["start_logposterior"][3])
        top = rc.scorelabellings(ctx, clust, None, 1.5, 0.1)["logposterior"][0]
        assert top == info["logposterior"][info["best"]] == info["logposterior"].max()
        # a candidate that is a mode already: no run beats it, and it comes back as mapestimate returns it
        again, i2 = rc.searchmapestimate(ctx, [clust], None, 1.5, 0.1, nruns=1, seed=2)
        assert i2["logposterior"][0] == top == i2["start_logposterior"][0] and i2["moves"][0] == 0
        assert max(i2["logposterior"].max(), i2["candidate_logposterior"][0]) >= top
        if not i2["logposterior"].max() > top:
            assert i2["best"] == -1 and np.array_equal(again, clust)
        # no candidates: init rows and the empty start under the given pair
        only, i3 = rc.searchmapestimate(ctx, None, None, 1.5, 0.1, init=[truth], seed=2)
        assert len(i3["runs"]) == 2 and i3["index"] is None and i3["logposterior"][i3["best"]] >= i3["start_logposterior"][0]
        with pytest.raises(ValueError, match="r and p"):
            rc.searchmapestimate(ctx, None)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_the_same_bits_and_a_run_does_not_depend_on_its_company(solved, kind):
    c, ctx, first, _ = solved("n130", kind)
    again = run_on(ctx, c)
    for k in ("labels", "slots", "blocks", "loglik", "logprior", "logposterior", "sweeps", "moves", "K"):
        assert np.array_equal(first[k], again[k]), k
    # 16 runs: the five starts cycled under orders of their own; run 7 alone gives the bits it gives among them
    g = np.random.default_rng(16)
    init = np.stack([c["init"][q % 5] for q in range(16)])
    order = np.stack([g.permutation(130) + 1 for _ in range(16)]).astype(np.int32)
    r, p = 1.0 + 0.1 * np.arange(16), np.full(16, 0.1)
    many = ctx.map_search(init, order, r, p, want_state=True)
    alone = ctx.map_search(init[7:8], order[7:8], r[7:8], p[7:8], want_state=True)
    for k in ("labels", "slots", "blocks", "loglik", "logprior", "logposterior", "start_logposterior", "sweeps", "moves", "K", "converged"):
        assert np.array_equal(many[k][7:8], alone[k], equal_nan=True), k
    assert len({m for m in many["moves"]}) > 1


def mid_chain_context(kind, D, P):
    """20 sweeps with moving labels from a scattered start: the points have been re-laid out (pi is not the identity) and the
    row-sum pipeline is running"""
    ctx = make_context(kind, D)
    ctx.set_params(**P)
    ctx.set_state(np.random.default_rng(3).integers(1, 14, D.shape[0]).astype(np.int64))
    for t in range(20):
        ctx.gibbs_sweep(1.0 + 0.1 * (t % 3), 0.4, seed=11, sweep_index=t)
        ctx.record_sample(False)
    assert ctx.layout_info()[0] >= 1
    return ctx


@pytest.mark.parametrize("kind", KINDS)
def test_a_context_in_mid_chain_is_read_through_its_layout_and_left_as_it_was(kind):
    """With a stored log the kernel indexes Lq by the internal (row, column) itself — a derived log is recomputed from Dq and would
    hide a wrong index — so the re-laid-out context is held against the reference on every kind."""
    c = R.case("n130")
    ctx = mid_chain_context(kind, c["D"], c["P"])
    try:
        def snapshot():
            return ctx.get_state(), ctx.layout_info(), ctx.cocluster_counts(), ctx.bulk_kernel_name(), ctx.capacity_info(), ctx.loglik()
        before = snapshot()
        res = run_on(ctx, c)
        assert_equal_to_reference(res, R.run_case(c, *integers(ctx)))
        after = snapshot()
        assert all(np.array_equal(x, y) for x, y in zip(before[0][:2], after[0][:2])) and before[0][2] == after[0][2]
        assert before[1] == after[1] and np.array_equal(before[2], after[2]) and before[3:] == after[3:]
        plain = make_context(kind, c["D"])
        try:
            plain.set_params(**c["P"])
            same = run_on(plain, c)
            for k in ("labels", "blocks", "logposterior"):
                assert np.array_equal(res[k], same[k]), k
        finally:
            plain.close()
    finally:
        ctx.close()


def test_params_given_are_used_and_none_needs_the_contexts():
    c = R.case("n65")
    ctx = make_context("stored64", c["D"])
    try:
        with pytest.raises(rc.RedClustHIPError, match="RC_ERR_STATE"):
            run_on(ctx, c)
        res = run_on(ctx, c, params=c["P"])
        assert_equal_to_reference(res, R.run_case(c, *integers_with(ctx, c["P"])))
        other = dict(c["P"], repulsion=False, alpha=20.0)
        ctx.set_params(**c["P"])
        res2 = run_on(ctx, c, params=other)
        assert_equal_to_reference(res2, R.run_case(dict(c, P=other), *integers(ctx)))
        sc = rc.scorelabellings(ctx, res2["labels"][0], other, c["r"][0], c["p"][0])
        assert res2["logposterior"][0] == sc["logposterior"][0]
    finally:
        ctx.close()


def integers_with(ctx, P):
    sc = ctx.score(np.ones(ctx.n, np.int64), params=P)
    return SR.quantised(ctx.get_matrix(0), sc["eD"]), SR.quantised(ctx.get_matrix(1), sc["eL"]), sc["eD"], sc["eL"]


def test_argument_errors_come_before_any_device_work(solved):
    c, ctx, _, _ = solved("n65", "derived64")
    n, L = ctx.n, rc.lib()
    init, order = c["init"][:2].copy(), c["order"][:2].copy()
    labels, runs = np.zeros((2, n), np.int64), (_lib.RcMapRun * 2)()
    best = C.c_int32()

    def raw(nruns=2, init=init, order=order, r=(1.0, 1.5), p=(0.1, 0.2), params=None, maxK=0, maxsweeps=5, out=labels, rec=runs, bst=best, h=None):
        keep = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (r, p)]
        ptr = lambda a: None if a is None else a.ctypes.data
        prm = None if params is None else C.byref(_lib._params_struct(params))
        code = L.rc_map_search(ctx.h if h is None else h, nruns, ptr(init), ptr(order), ptr(keep[0]), ptr(keep[1]), prm, maxK, maxsweeps,
                               ptr(out), None if rec is None else rec, None, None, None if bst is None else C.byref(bst), None)
        return code, L.rc_last_error(ctx.h if h is None else h).decode()
    assert raw()[0] == 0
    bad = init.copy(); bad[1, 7] = n + 1
    neg = init.copy(); neg[0, 0] = -1
    twice = order.copy(); twice[0, 3] = twice[0, 4]
    zero = order.copy(); zero[1, 0] = 0
    singles = np.stack([np.arange(1, n + 1)] * 2)
    for kw, code, text in ((dict(init=None), ARG, "NULL argument"), (dict(order=None), ARG, "NULL argument"), (dict(r=None), ARG, "NULL argument"),
                           (dict(p=None), ARG, "NULL argument"), (dict(out=None), ARG, "NULL argument"), (dict(rec=None), ARG, "NULL argument"),
                           (dict(bst=None), ARG, "NULL argument"),
                           (dict(nruns=0), ARG, "nruns >= 1"), (dict(maxsweeps=0), ARG, "maxsweeps >= 1"), (dict(maxK=-1), ARG, "maxK >= 0"),
                           (dict(init=bad), ARG, f"label {n + 1} of run 2 outside 0..n"), (dict(init=neg), ARG, "label -1 of run 1 outside 0..n"),
                           (dict(order=twice), ARG, "the order of run 1 is not a permutation"), (dict(order=zero), ARG, "the order of run 2 is not a permutation"),
                           (dict(init=bad, order=twice), ARG, "the order of run 1"),                 # run 1's order before run 2's label
                           (dict(r=(1.0, 0.0)), ARG, "r of run 2 must be positive and finite"), (dict(r=(np.inf, 1.0)), ARG, "r of run 1"),
                           (dict(p=(0.1, 1.0)), ARG, "p of run 2 must lie in (0, 1)"), (dict(order=zero, r=(0.0, 1.0)), ARG, "the order of run 2"),
                           (dict(params=dict(c["P"], zeta=-1.0)), ARG, "must be positive"), (dict(p=(0.0, 0.5), params=dict(c["P"], zeta=-1.0)), ARG, "p of run 1"),
                           (dict(maxK=1025), CAP, "the slot cap 1025 (maxK) exceeds 1024"), (dict(maxK=1025, r=(-1.0, 1.0)), ARG, "r of run 1"),
                           (dict(init=singles, maxK=3), ARG, f"run 1 starts with {n} clusters, more than the slot cap 3")):
        code_, msg = raw(**kw)
        assert code_ == code and text in msg, (kw, code_, msg)
    bare = make_context("derived64", c["D"])
    try:
        code_, msg = raw(h=bare.h)
        assert code_ == STATE and "params is NULL and the context has no parameters set" in msg
        code_, msg = raw(h=bare.h, maxK=1025, params=dict(c["P"], zeta=-1.0))
        assert code_ == ARG and "must be positive" in msg                # the parameters before the capacity
    finally:
        bare.close()
    assert L.rc_map_search(None, 2, None, None, None, None, None, 0, 5, None, None, None, None, None, None) == ARG


def test_n_8193_is_beyond_the_capacity():
    X = np.random.default_rng(8).normal(0, 1, (8193, 2))
    ctx = rc.Context.from_points(X)
    try:
        ctx.set_params(**R.P0)
        with pytest.raises(rc.RedClustHIPError, match=r"RC_ERR_CAPACITY.*n = 8193 exceeds the 8192"):
            ctx.map_search(np.zeros((1, 8193), np.int64), np.arange(1, 8194, dtype=np.int32)[None, :], 1.0, 0.5)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_hclust_cut_polished(kind):
    c = R.case("n65")
    rng = np.random.default_rng(1)
    truth = c["init"][1]
    samples = np.stack([np.where(rng.random(65) < 0.15, rng.integers(1, 5, 65), truth) for _ in range(12)]).astype(np.int64)
    ctx = make_context(kind, c["D"])
    try:
        ctx.set_params(**c["P"])
        counts = _lib.samples_counts(samples)[0]
        cut, hi = rc.hclustpointestimate(counts, numsamples=12, maxK=8, criterion="posterior", data=ctx, r=1.5, p=0.1)
        pol, pi = rc.hclustpointestimate(counts, numsamples=12, maxK=8, criterion="posterior", data=ctx, r=1.5, p=0.1, polish=True)
        assert "polish" not in hi and np.array_equal(pi["logposterior"], hi["logposterior"])
        top = rc.scorelabellings(ctx, pol, None, 1.5, 0.1)["logposterior"][0]
        assert top >= hi["logposterior"][hi["K"] - 1]
        with pytest.raises(ValueError, match="polish"):
            rc.hclustpointestimate(counts, numsamples=12, maxK=8, polish=True)
    finally:
        ctx.close()
