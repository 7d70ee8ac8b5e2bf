"""rc_map_search_large (csrc/mapsearch_large.inc.hip: k_map_cells, k_map_large) through Context.map_search_large, and searchmap
(-m gpu): the MAP search for n <= 32767.  Wherever rc_map_search accepts the input the two must agree byte for byte, the
blocks_out cells included; above its limit the NumPy restatement (tests/map_search_ref.py) decides, on the context's own
integers, with its decision gaps held above 1e-6 as tests/test_gpu_mapsearch.py holds them."""
import ctypes as C

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import map_search_ref as R
from test_gpu_mapsearch import KINDS, ARG, CAP, make_context, integers, assert_equal_to_reference, mid_chain_context, kernel_values
import score_ref as SR

pytestmark = pytest.mark.gpu

KEYS = ("labels", "slots", "blocks", "loglik", "logprior", "logposterior", "start_logposterior", "sweeps", "moves", "K", "converged", "capped", "best")


def both(ctx, c, **kw):
    """(the large entry's result, rc_map_search's) of a case, the second held equal to the first in every byte"""
    args = (c["init"], c["order"], c["r"], c["p"])
    kw = dict(dict(maxK=c["maxK"], maxsweeps=c["maxsweeps"], want_state=True), **kw)
    large, old = ctx.map_search_large(*args, **kw), ctx.map_search(*args, **kw)
    for k in KEYS:
        assert np.array_equal(large[k], old[k], equal_nan=True), k
    assert large["kernel_ms"] > 0
    return large


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", R.CASES)
def test_reference_cases(name, kind):
    """every fixed input of the reference module, "diag" (a nonzero diagonal of D) among them"""
    c = R.case(name)
    ctx = make_context(kind, c["D"])
    try:
        ctx.set_params(**c["P"])
        assert_equal_to_reference(both(ctx, c), R.run_case(c, *integers(ctx)))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (5, 130, 1025, 1026, 1027, 2049))
def test_row_widths(n, kind):
    """n mod 4 = 1, 2, 1, 2, 3, 1 (every residue of the two-column chunks), 2049 one column past a full pass of 512 chunks of
    four; starts from empty labels, a planted labelling (k_map_cells runs) and singletons — beyond the 1024 slots a noisy
    labelling, which the cap admits — each with and without repulsion, two sweeps."""
    D, truth = R.planted(n, 4, 0.3, 40 + n)
    init, order = R.starts(n, 4, truth, n, ("empty", "planted", "singletons" if n <= 1024 else "noisy"))
    ctx = make_context(kind, D)
    try:
        for rep in (True, False):
            c = dict(init=init, order=order, r=1.5 + 0.25 * np.arange(3), p=np.full(3, 0.1), maxK=0, maxsweeps=2)
            res = both(ctx, c, params=dict(R.P0, repulsion=rep))
            assert res["moves"][0] >= n
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_context_in_mid_chain(kind):
    """pi is not the identity: the result is a fresh context's, and the state, the layout and the counts stay as they were"""
    c = R.case("n130")
    ctx, plain = mid_chain_context(kind, c["D"], c["P"]), make_context(kind, c["D"])
    try:
        snapshot = lambda: (ctx.get_state(), ctx.layout_info(), ctx.cocluster_counts(), ctx.bulk_kernel_name(), ctx.capacity_info(), ctx.loglik())
        before = snapshot()
        res = both(ctx, c)
        after = snapshot()
        assert all(np.array_equal(x, y) for x, y in zip(before[0][:2], after[0][:2])) and before[0][2] == after[0][2]
        assert before[1] == after[1] and np.array_equal(before[2], after[2]) and before[3:] == after[3:]
        plain.set_params(**c["P"])
        fresh = both(plain, c)
        for k in KEYS:
            assert np.array_equal(res[k], fresh[k], equal_nan=True), k
    finally:
        ctx.close(); plain.close()


def above_case(n=8200, K=3, seed=21, wrong=40):
    """(points, start, order): K centres on the unit sphere, noise 0.15, the truth with `wrong` points moved to the next cluster"""
    g = np.random.default_rng(seed)
    cen = g.normal(size=(K, 3))
    cen /= np.linalg.norm(cen, axis=1)[:, None]
    z = g.integers(0, K, n)
    X = cen[z] + 0.15 * g.normal(size=(n, 3))
    start = z.astype(np.int64) + 1
    hit = g.choice(n, wrong, replace=False)
    start[hit] = start[hit] % K + 1
    return X, start, (g.permutation(n) + 1).astype(np.int32)


P_ABOVE = dict(R.P0, repulsion=False, alpha=20.0)


@pytest.mark.parametrize("bits", (64, 32))
def test_above_the_old_limit(bits):
    """n = 8200: rc_map_search refuses, so the reference decides (one sweep; on the host it takes about 10 s)"""
    X, start, order = above_case()
    ctx = rc.Context.from_points(X, storage_bits=bits)
    try:
        ctx.set_params(**P_ABOVE)
        with pytest.raises(rc.RedClustHIPError, match="RC_ERR_CAPACITY"):
            ctx.map_search(start[None, :], order[None, :], 1.5, 0.5, maxsweeps=1)
        res = ctx.map_search_large(start[None, :], order[None, :], 1.5, 0.5, maxsweeps=1, want_state=True)
        ref = R.search(*integers(ctx), start, order, 1.5, 0.5, P_ABOVE, 0, 1)
        assert_equal_to_reference(res, [ref])
        lab, Kf = res["labels"][0], int(res["K"][0])
        sc = ctx.score(lab, want_blocks=True)
        slot_of = np.zeros(Kf + 1, np.int64)
        slot_of[lab] = res["slots"][0]
        VD, VL = kernel_values(res["blocks"][0])
        iu = np.triu_indices(Kf)
        s = slot_of[1:] - 1
        assert [(VD[s[a], s[b]], VL[s[a], s[b]]) for a, b in zip(*iu)] == SR.values(sc["blocks"][0])
        top = rc.scorelabellings(ctx, lab, None, 1.5, 0.5)
        assert (res["loglik"][0], res["logprior"][0], res["logposterior"][0]) == (top["loglik"][0], top["logprior"][0], top["logposterior"][0])
        assert res["logposterior"][0] >= res["start_logposterior"][0] == rc.scorelabellings(ctx, start, None, 1.5, 0.5)["logposterior"][0]
        # searchmap routes to the large entry: the run from init under the order searchmapestimate would draw
        with pytest.raises(rc.RedClustHIPError, match="RC_ERR_CAPACITY"):
            rc.searchmapestimate(ctx, None, None, 1.5, 0.5, init=[start], maxsweeps=1, seed=3)
        _, info = rc.searchmap(ctx, None, None, 1.5, 0.5, init=[start], maxsweeps=1, seed=3)
        o3 = np.random.Generator(np.random.Philox(key=3)).permutation(8200).astype(np.int32) + 1
        own = ctx.map_search_large(start[None, :], o3[None, :], 1.5, 0.5, maxsweeps=1)
        assert np.array_equal(info["labels"][0], own["labels"][0]) and info["logposterior"][0] == own["logposterior"][0]
    finally:
        ctx.close()


def test_searchmap_is_searchmapestimate_up_to_8192():
    D, truth = R.planted(300, 4, 0.3, 9)
    ctx = make_context("derived64", D)
    try:
        ctx.set_params(**R.P0)
        a, ia = rc.searchmap(ctx, [truth, np.ones(300, np.int64)], None, 1.5, 0.1, nruns=2, seed=4)
        b, ib = rc.searchmapestimate(ctx, [truth, np.ones(300, np.int64)], None, 1.5, 0.1, nruns=2, seed=4)
        assert np.array_equal(a, b) and ia.keys() == ib.keys()
        for k in ("labels", "logposterior", "start_logposterior", "sweeps", "moves", "K", "runs", "candidate_logposterior"):
            assert np.array_equal(ia[k], ib[k], equal_nan=True), k
    finally:
        ctx.close()


def test_errors_come_before_any_device_work():
    c = R.case("n65")
    ctx = make_context("derived64", c["D"])
    big = rc.Context.from_points(np.random.default_rng(8).normal(0, 1, (32768, 2)), storage_bits=32)
    try:
        ctx.set_params(**c["P"]); big.set_params(**c["P"])
        L, best = rc.lib(), C.c_int32()

        def raw(h, n, nruns=1, init=0, order=None, r=1.5, maxK=0, maxsweeps=5):
            init = np.full((1, n), init, np.int64) if np.isscalar(init) else init
            order = np.arange(1, n + 1, dtype=np.int32)[None, :] if order is None else order
            r_, p_, labels, runs = np.array([r]), np.array([0.1]), np.zeros((1, n), np.int64), (_lib.RcMapRun * 1)()
            code = L.rc_map_search_large(h, nruns, None if init is None else init.ctypes.data, order.ctypes.data, r_.ctypes.data, p_.ctypes.data,
                                         None, maxK, maxsweeps, labels.ctypes.data, runs, None, None, C.byref(best), None)
            return code, L.rc_last_error(h).decode()
        assert raw(ctx.h, 65)[0] == 0
        twice = np.arange(1, 66, dtype=np.int32)[None, :].copy(); twice[0, 3] = twice[0, 4]
        for kw, code, text in ((dict(h=big.h, n=32768), CAP, "n = 32768 exceeds the 32767"), (dict(maxK=1025), CAP, "the slot cap 1025 (maxK) exceeds 1024"),
                               (dict(nruns=0), ARG, "nruns >= 1"), (dict(maxsweeps=0), ARG, "maxsweeps >= 1"), (dict(init=66), ARG, "label 66 of run 1 outside 0..n"),
                               (dict(order=twice), ARG, "the order of run 1 is not a permutation"), (dict(r=0.0), ARG, "r of run 1 must be positive and finite"),
                               (dict(r=0.0, maxK=1025), ARG, "r of run 1"), (dict(init=np.arange(1, 66)[None, :].copy(), maxK=3), ARG, "starts with 65 clusters")):
            code_, msg = raw(**dict(dict(h=ctx.h, n=65), **kw))
            assert code_ == code and text in msg and msg.startswith("rc_map_search_large:"), (kw, code_, msg)
        assert L.rc_map_search_large(None, 1, None, None, None, None, None, 0, 5, None, None, None, None, None, None) == ARG
    finally:
        ctx.close(); big.close()
