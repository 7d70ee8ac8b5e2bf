"""The hierarchical point estimates on the GPU (csrc/hclust.inc.hip through rc_hclust / rc_hclust_samples / rc_hclust_ctx,
rc_psm_expected_loss and hclust, hclustpointestimate, expectedlosses).  The linkage and the Binder numerators are exact
integer functions of the counts and are held to tests/hclust_ref.py and psm_search_ref.binder_num bit for bit.

Shapes: those of test_gpu_pointsearch.py — the wave (63/64/65) and workgroup (1000/1025 around the 1024 threads) edges, n = 1
and 2 — and three more for the tie rules and the zero-similarity merges: noise 0 (every count is 0 or m), every point planted
alone, and m = 3 with two clusters.  The 128-bit comparison's high word needs m·n⁴/16 > 2^64 (n near 8192 with m >= 65536)
and is out of any test's reach.

VI tolerance.  The returned loss is a plain f64 host sum of at most 1025·2 log terms of magnitude <= log(m·n) ≈ 17 (each
within an ulp or two of NumPy's), divided by n: far below LOSS_TOL = 1e-9, test_gpu_pointsearch.py's derivation unchanged.
MOVE_TOL = 1e-8 is that file's bound on a search step's score."""
import functools

import numpy as np
import pytest

import hclust_ref as H
import psm_search_ref as R
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1, 0.0), (2, 3, 2, 0.0), (63, 7, 3, 0.1), (64, 7, 4, 0.1), (65, 50, 5, 0.2), (257, 20, 16, 0.2),
          (1000, 20, 40, 0.3), (1025, 9, 10, 0.2), (64, 7, 4, 0.0), (65, 5, 65, 0.5), (100, 3, 2, 0.4)]
IDS = [f"n{s[0]}m{s[1]}K{s[2]}" for s in SHAPES]
LINKS = ["average", "complete", "single"]
LOSS_TOL, MOVE_TOL = 1e-9, 1e-8
ARG, STATE, CAP = -1, -5, -6


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(samples, counts) of a shape; computed once and shared (never modified)."""
    n, m, K, noise = shape
    S, C = R.planted_counts(n, m, K, noise, seed=1000 + n + (0 if noise else 7))
    S.setflags(write=False); C.setflags(write=False)
    return S, C


@functools.lru_cache(maxsize=None)
def reference(shape, linkage):
    return H.hclust_ref(problem(shape)[1], shape[1], H.LINKAGES[linkage])


def cut_sizes(shape):
    n, K = shape[0], shape[2]
    return sorted({1, min(2, n), min(3, n), min(K, n), n // 2 + 1, n})


@pytest.mark.parametrize("linkage", LINKS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_linkage_equals_the_reference_bit_for_bit(shape, linkage):
    n, m = shape[0], shape[1]
    _, C = problem(shape)
    ref = reference(shape, linkage)
    got = _lib.hclust(C, m, H.LINKAGES[linkage])
    print(shape, linkage, "kernel_ms", got["kernel_ms"], "first merges", got["merges"][:3])
    for f in ("a", "b", "size", "m_ab", "s_ab"):
        assert np.array_equal(got["merges"][f], ref["merges"][f]), f
    assert np.array_equal(got["binder_num"], ref["binder_num"])
    for k in cut_sizes(shape):
        assert np.array_equal(_lib.hclust_cut(got["merges"], n, k), H.cut(ref["merges"], n, k)), k
    again = _lib.hclust(C, m, H.LINKAGES[linkage])
    assert again["merges"].tobytes() == got["merges"].tobytes() and again["binder_num"].tobytes() == got["binder_num"].tobytes()


def test_the_three_linkages_are_three_different_runs():
    for shape in (SHAPES[4], SHAPES[5]):
        runs = {_lib.hclust(problem(shape)[1], shape[1], l)["merges"].tobytes() for l in (0, 1, 2)}
        assert len(runs) == 3


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[5], SHAPES[9]], ids=[IDS[1], IDS[4], IDS[5], IDS[9]])
def test_samples_form_equals_the_host_counts_form(shape):
    S, C = problem(shape)
    for l in (0, 1, 2):
        a = _lib.hclust(C, shape[1], l, maxcut=min(3, shape[0]))
        b = _lib.hclust(None, None, l, maxcut=min(3, shape[0]), samples=S)
        for k in ("merges", "binder_num", "vilb"):
            assert a[k].tobytes() == b[k].tobytes(), (l, k)
        assert b["counts_ms"] > 0


class _Samples:
    def __init__(self, clusts):
        self.clusts = list(clusts)


def _context_with_samples(n=100, nsamples=5):
    d = rc.generatemixture(n, 4, alpha=10, sigma=0.25, dim=4, seed=5)
    D = d["distancematrix"]
    ctx = rc.Context(D)
    ctx.set_params(**rc.likelihood_hyperparams(D, d["clusts"]))
    ctx.set_state(np.random.default_rng(1).integers(1, 7, n).astype(np.int64))
    recorded = []
    for t in range(nsamples):
        ctx.gibbs_sweep(1.0, 0.5, seed=9, sweep_index=t)
        recorded.append(ctx.record_sample())
    return ctx, recorded


def test_context_form_equals_the_host_form_and_leaves_the_chain_alone():
    n, m = 100, 5
    ctx, recorded = _context_with_samples(n, m)
    twin, _ = _context_with_samples(n, m)
    counts = ctx.cocluster_counts()
    before = ctx.get_state()
    labs = np.stack([R.sortlabels(r) for r in recorded] + [np.ones(n, np.int64)])
    for l in (0, 1, 2):
        a = _lib.hclust(None, m, l, maxcut=13, ctx=ctx)
        b = _lib.hclust(counts, m, l, maxcut=13)
        for k in ("merges", "binder_num", "vilb"):
            assert a[k].tobytes() == b[k].tobytes(), (l, k)
    for loss in (R.BINDER, R.VILB):
        a = _lib.psm_expected_loss(labs, None, m, loss, ctx=ctx)
        b = _lib.psm_expected_loss(labs, counts, m, loss)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    clust, info = rc.hclustpointestimate(loss="VI", numsamples=m, ctx=ctx)
    assert len(clust) == n and info["K"] == int(np.argmin(info["loss"])) + 1
    h = rc.hclust(numsamples=m, ctx=ctx)
    assert sorted(h["order"]) == list(range(n)) and h["Z"].shape == (n - 1, 4)
    l2, n2 = rc.expectedlosses(clust, numsamples=m, loss="binder", ctx=ctx)
    assert n2[0] == R.binder_num(clust, counts, m)
    after = ctx.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert np.array_equal(ctx.cocluster_counts(), counts)
    ctx.gibbs_sweep(1.25, 0.4, seed=9, sweep_index=m)
    twin.gibbs_sweep(1.25, 0.4, seed=9, sweep_index=m)
    assert np.array_equal(ctx.get_state()[0], twin.get_state()[0]) and ctx.loglik() == twin.loglik()
    ctx.close(); twin.close()


def labellings(shape, L):
    """L labellings of a shape: n singletons, one cluster, the planted first sample, then random ones with 1..n labels"""
    n = shape[0]
    S, _ = problem(shape)
    rng = np.random.default_rng(n + L)
    labs = [np.arange(1, n + 1), np.ones(n, np.int64), S[0]]
    while len(labs) < L:
        labs.append(rng.integers(1, rng.integers(1, n + 1) + 1, n))
    return np.stack(labs[:L]).astype(np.int64)


@pytest.mark.parametrize("L", [1, 11])                     # one labelling; more than one LDS group of 8
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_expectedlosses(shape, L):
    n, m = shape[0], shape[1]
    _, C = problem(shape)
    labs = labellings(shape, L)
    bl, bn = rc.expectedlosses(labs, C, m, "binder")
    vl, vn = rc.expectedlosses(labs, C, m, "VI")
    assert bl.shape == bn.shape == vl.shape == (L,) and not vn.any()
    for l in range(L):
        err = abs(vl[l] - rc.expectedloss(labs[l], C, m, "VI"))
        print(shape, l, "K", len(np.unique(labs[l])), "num", bn[l], "VI err", err)
        assert int(bn[l]) == R.binder_num(labs[l], C, m)
        assert bl[l] == rc.expectedloss(labs[l], C, m, "binder")
        assert err <= LOSS_TOL
    again = rc.expectedlosses(labs, C, m, "VI")
    assert again[0].tobytes() == vl.tobytes()
    # labels outside 1..n are compacted like expectedloss's; one labelling may come as a vector
    one = rc.expectedlosses(labs[-1] * 7 + 100, C, m, "binder")
    assert one[1][0] == bn[-1]


@pytest.mark.parametrize("linkage", LINKS)
@pytest.mark.parametrize("loss", ["binder", "VI"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[5], SHAPES[8], SHAPES[10]], ids=[IDS[0], IDS[4], IDS[5], IDS[8], IDS[10]])
def test_hclustpointestimate(shape, loss, linkage):
    n, m, K, noise = shape
    S, C = problem(shape)
    clust, info = rc.hclustpointestimate(C, loss, linkage, numsamples=m)
    maxK = -(-n // 8)
    assert len(info["loss"]) == maxK
    k = info["K"]
    assert k == int(np.argmin(info["loss"])) + 1                                       # np.argmin: the first minimum, the smaller K
    assert np.array_equal(clust, H.cut(reference(shape, linkage)["merges"], n, k))
    if loss == "binder":
        assert int(info["loss_num"][k - 1]) == R.binder_num(clust, C, m) == int(info["binder_num"][n - k])
        assert info["loss"][k - 1] == rc.expectedloss(clust, C, m, "binder")
        for kk in range(1, maxK + 1):
            assert int(info["loss_num"][kk - 1]) == int(reference(shape, linkage)["binder_num"][n - kk])
    else:
        for kk in sorted({1, k, maxK}):
            c = H.cut(reference(shape, linkage)["merges"], n, kk)
            assert abs(info["loss"][kk - 1] - rc.expectedloss(c, C, m, "VI")) <= LOSS_TOL, kk
    # the samples form; an explicit maxK
    c2, i2 = rc.hclustpointestimate(_Samples(S), loss, linkage, maxK=min(3, n))
    assert len(i2["loss"]) == min(3, n) and np.array_equal(i2["loss"], info["loss"][: min(3, n)])
    # a deterministic start for the search, which is never worse than it
    _, si = rc.searchpointestimate(C, loss, numsamples=m, nruns=0, init=[clust])
    print(shape, loss, linkage, "K", k, "loss", info["loss"][k - 1], "after the search", si["loss"][0])
    if loss == "binder":
        assert int(si["loss_num"][0]) <= int(info["loss_num"][k - 1])
    else:
        assert si["loss"][0] <= info["loss"][k - 1] + MOVE_TOL
    if noise == 0.0:                                                                    # the planted partition comes back
        assert np.array_equal(clust, R.sortlabels(S[0]))


def test_hclust_surface():
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    shape = SHAPES[5]
    n, m = shape[0], shape[1]
    S, C = problem(shape)
    for linkage in LINKS:
        h = rc.hclust(C, linkage, numsamples=m)
        ref = reference(shape, linkage)
        assert h["merges"].tobytes() == ref["merges"].tobytes() and np.array_equal(h["binder_num"], ref["binder_num"])
        assert hier.is_valid_linkage(h["Z"]) and np.array_equal(h["order"], hier.leaves_list(h["Z"]))
        assert np.array_equal(h["Z"][:, 2], H.heights(ref["merges"], m, H.LINKAGES[linkage]))
    hs = rc.hclust(_Samples(S), "average")
    assert hs["merges"].tobytes() == reference(shape, "average")["merges"].tobytes()


def test_errors_return_their_codes_and_the_process_goes_on():
    L = _lib.lib()
    n, m = 8, 3
    _, C = R.planted_counts(n, m, 2, 0.2, seed=1)
    merges = np.zeros(n, _lib.HCLUST_MERGE)
    bnum = np.zeros(n, np.int64)
    vilb = np.zeros(n)
    labs = np.ones((2, n), np.int64)
    lo, nu = np.zeros(2), np.zeros(2, np.int64)
    p = lambda x: None if x is None else x.ctypes.data

    def hc(counts=C, m_=m, n_=n, linkage=0, merges_=merges, bnum_=bnum, maxcut=0, vilb_=vilb):
        code = L.rc_hclust(0, p(counts), m_, n_, linkage, p(merges_), p(bnum_), maxcut, p(vilb_), None)
        return code, L.rc_last_error(None).decode()

    def el(counts=C, m_=m, n_=n, loss=0, L_=2, labs_=labs, lo_=lo, nu_=nu):
        code = L.rc_psm_expected_loss(0, p(counts), m_, n_, loss, L_, p(labs_), p(lo_), p(nu_), None)
        return code, L.rc_last_error(None).decode()

    asym = C.copy(); asym[0, 1] += 1
    diag = C.copy(); diag[2, 2] = m - 1
    big = C.copy(); big[0, 1] = big[1, 0] = m + 1
    bad_label = labs.copy(); bad_label[1, 3] = n + 1
    zero_label = labs.copy(); zero_label[0, 0] = 0
    for what, (code, msg) in [("n = 8193", hc(n_=8193)), ("m·n >= 2^31", hc(m_=2 ** 31)), ("n = 8193", el(n_=8193)),
                              ("m·n >= 2^31", el(m_=2 ** 28)), ("too many labellings", el(L_=65537))]:
        assert code == CAP and msg, (what, code, msg)
    cases = [("NULL counts", hc(counts=None)), ("NULL merges", hc(merges_=None)), ("NULL binder_num", hc(bnum_=None)),
             ("m < 1", hc(m_=0)), ("n < 1", hc(n_=0)), ("bad linkage", hc(linkage=3)), ("negative linkage", hc(linkage=-1)),
             ("maxcut > n", hc(maxcut=n + 1)), ("maxcut without vilb", hc(maxcut=2, vilb_=None)),
             ("asymmetric counts", hc(counts=asym)), ("diagonal not m", hc(counts=diag)), ("count above m", hc(counts=big)),
             ("wrong m", hc(m_=m + 1)),
             ("NULL counts", el(counts=None)), ("NULL labels", el(labs_=None)), ("NULL loss_out", el(lo_=None)),
             ("NULL num_out", el(nu_=None)), ("bad loss", el(loss=2)), ("L < 1", el(L_=0)), ("label above n", el(labs_=bad_label)),
             ("label 0", el(labs_=zero_label)), ("asymmetric counts", el(counts=asym)), ("wrong m", el(m_=m + 1))]
    for what, (code, msg) in cases:
        assert code == ARG and msg, (what, code, msg)
    # the context forms: NULL context, nothing recorded yet, the wrong number of samples
    hargs = (m, 0, p(merges), p(bnum), 0, None, None)
    eargs = (m, 0, 2, p(labs), p(lo), p(nu), None)
    assert L.rc_hclust_ctx(None, *hargs) == ARG and L.rc_psm_expected_loss_ctx(None, *eargs) == ARG
    d = rc.generatemixture(n, 2, alpha=10, sigma=0.25, dim=2, seed=1)
    ctx = rc.Context(d["distancematrix"])
    assert L.rc_hclust_ctx(ctx.h, *hargs) == STATE and b"recorded" in L.rc_last_error(ctx.h)
    assert L.rc_psm_expected_loss_ctx(ctx.h, *eargs) == STATE
    ctx.set_params(**rc.likelihood_hyperparams(d["distancematrix"], d["clusts"]))
    ctx.set_state(d["clusts"])
    ctx.record_sample()
    assert L.rc_hclust_ctx(ctx.h, *((2,) + hargs[1:])) == ARG            # one sample recorded, two claimed
    assert L.rc_hclust_ctx(ctx.h, *((1,) + hargs[1:])) == 0
    assert np.array_equal(_lib.hclust_cut(merges[: n - 1], n, len(np.unique(d["clusts"]))), R.sortlabels(d["clusts"]))
    ctx.close()
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.hclust(asym, m, 0)
    with pytest.raises(ValueError):
        rc.hclust(C, "ward", numsamples=m)
    with pytest.raises(ValueError):
        rc.hclustpointestimate(C, "ID", numsamples=m)
    # and valid calls afterwards
    code, msg = hc(maxcut=2)
    ref = H.hclust_ref(C, m, H.AVERAGE)
    assert code == 0 and merges[: n - 1].tobytes() == ref["merges"].tobytes() and np.array_equal(bnum, ref["binder_num"])
    assert abs(vilb[1] - rc.expectedloss(H.cut(ref["merges"], n, 2), C, m, "VI")) <= LOSS_TOL
    code, msg = el()
    assert code == 0 and nu[0] == R.binder_num(labs[0], C, m)
