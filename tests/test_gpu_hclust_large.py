"""The hierarchical point estimates for n <= 32767 (csrc/hclust_large.inc.hip through rc_hclust_large*, rc_hclust_cut_large,
rc_psm_expected_loss_large* and dendrogram, dendrogrampointestimate, expectedlosses).  A run is integer arithmetic on the
counts: wherever rc_hclust runs too, the large kernel is held to tests/hclust_ref.py and to rc_hclust's bytes, on the shapes
of test_gpu_hclust.py — which cross the 32 rows of a second-level block (63/64/65), its tie and zero-similarity shapes
included, and span 33 blocks at n = 1025.  Above 8192 points there is no reference (the restatement is too slow), so one shape,
n = 8195 with m = 5 (0.5 GB of S), is held to what needs none: the Binder curve against the numerators of the independent
expected-loss kernel, the single-linkage heights against SciPy's as a multiset (they do not depend on ties), and the validity
of the merge sequence.  VI tolerance: LOSS_TOL of test_gpu_hclust.py — at n = 8195 the f64 host sum has 8195·2 log terms below
log(m·n) ≈ 11, divided by n, the same bound."""
import functools

import numpy as np
import pytest

import hclust_ref as H
import psm_search_ref as R
import redclust_amd as rc
from redclust_amd import _lib
from test_gpu_hclust import IDS, LINKS, LOSS_TOL, SHAPES, _Samples, cut_sizes, labellings, problem, reference

pytestmark = pytest.mark.gpu

BIG = (8195, 5, 50, 0.2)
ARG, CAP = -1, -6


@functools.lru_cache(maxsize=None)
def big_run(linkage):
    """the large entry's result on BIG's host counts; computed once per linkage and shared (never modified)"""
    return _lib.hclust_large(problem(BIG)[1], BIG[1], H.LINKAGES[linkage])


@pytest.mark.parametrize("linkage", LINKS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_large_linkage_equals_the_reference_and_rc_hclust_bit_for_bit(shape, linkage):
    n, m = shape[0], shape[1]
    _, C = problem(shape)
    ref = reference(shape, linkage)
    got = _lib.hclust_large(C, m, H.LINKAGES[linkage], maxcut=min(3, n))
    old = _lib.hclust(C, m, H.LINKAGES[linkage], maxcut=min(3, n))
    for f in ("a", "b", "size", "m_ab", "s_ab"):
        assert np.array_equal(got["merges"][f], ref["merges"][f]), f
    assert np.array_equal(got["binder_num"], ref["binder_num"])
    for k in cut_sizes(shape):
        assert np.array_equal(_lib.hclust_cut_large(got["merges"], n, k), H.cut(ref["merges"], n, k)), k
    for k in ("merges", "binder_num", "vilb"):
        assert got[k].tobytes() == old[k].tobytes(), k


@pytest.mark.parametrize("linkage", LINKS)
def test_above_8192_the_binder_curve_the_heights_and_the_merge_sequence(linkage):
    n, m, K, _ = BIG
    _, C = problem(BIG)
    got = big_run(linkage)
    ks = [1, 2, 50, 1024, n]
    cuts = np.stack([_lib.hclust_cut_large(got["merges"], n, k) for k in ks])      # (a sequence that is not valid is refused)
    assert [len(np.unique(c)) for c in cuts] == ks
    _, num = rc.expectedlosses(cuts, C, m, "binder")
    print(linkage, "kernel_ms", got["kernel_ms"], "num", num)
    assert [int(x) for x in num] == [int(got["binder_num"][n - k]) for k in ks]
    if linkage == "single":
        hier = pytest.importorskip("scipy.cluster.hierarchy")
        from scipy.spatial.distance import squareform
        D = 1.0 - C.astype(np.float64) / m
        np.fill_diagonal(D, 0.0)
        Zs = hier.linkage(squareform(D, checks=False), "single")
        assert np.array_equal(np.sort(Zs[:, 2]), np.sort(H.heights(got["merges"], m, H.SINGLE)))


@pytest.mark.parametrize("group", [1, 2, None])
@pytest.mark.parametrize("L", [1, 11])
@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[5], SHAPES[7]], ids=[IDS[4], IDS[5], IDS[7]])
def test_large_expected_loss_equals_rc_psm_expected_loss_byte_for_byte(shape, L, group, monkeypatch):
    if group:
        monkeypatch.setenv("RC_ELOSS_GROUP", str(group))
    _, C = problem(shape)
    labs = labellings(shape, L)
    for loss in (R.BINDER, R.VILB):
        a = _lib.psm_expected_loss_large(labs, C, shape[1], loss)
        b = _lib.psm_expected_loss(labs, C, shape[1], loss)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), loss


def test_expected_loss_above_8192_against_numpy():
    n, m = BIG[0], BIG[1]
    S, C = problem(BIG)
    bl, bn = rc.expectedlosses(S[0], C, m, "binder")
    vl, _ = rc.expectedlosses(S[0], C, m, "VI")
    err = abs(vl[0] - rc.expectedloss(S[0], C, m, "VI"))
    print("num", bn[0], "VI err", err)
    assert int(bn[0]) == R.binder_num(S[0], C, m) and bl[0] == rc.expectedloss(S[0], C, m, "binder")
    assert err <= LOSS_TOL


def test_the_new_names_return_the_old_bytes_at_n_100():
    shape = SHAPES[10]
    S, C = problem(shape)
    a, b = rc.dendrogram(C, "complete", numsamples=shape[1]), rc.hclust(C, "complete", numsamples=shape[1])
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("merges", "binder_num", "Z", "order"))
    for loss, kw in (("binder", {}), ("VI", {}), ("VI", dict(exact=True))):
        src = _Samples(S) if kw else C
        (c1, i1), (c2, i2) = (f(src, loss, numsamples=shape[1], **kw) for f in (rc.dendrogrampointestimate, rc.hclustpointestimate))
        assert np.array_equal(c1, c2) and i1["K"] == i2["K"] and np.array_equal(i1["loss"], i2["loss"])
        assert i1["merges"].tobytes() == i2["merges"].tobytes()


def test_above_8192_the_new_names_return_the_large_entries_results_in_every_form():
    n, m = BIG[0], BIG[1]
    S, C = problem(BIG)
    want = big_run("average")
    d = rc.generatemixture(n, 4, alpha=10, sigma=0.25, dim=4, seed=3)
    ctx = rc.Context(d["distancematrix"])
    P = rc.likelihood_hyperparams(d["distancematrix"], d["clusts"])
    ctx.set_params(**P)
    for s in S:
        ctx.set_state(s)
        ctx.record_sample()
    forms = dict(counts=lambda f, *a, **k: f(C, *a, numsamples=m, **k), samples=lambda f, *a, **k: f(_Samples(S), *a, **k),
                 context=lambda f, *a, **k: f(None, *a, numsamples=m, ctx=ctx, **k))
    vilb = _lib.hclust_large(C, m, 0, maxcut=3)["vilb"]
    for name, call in forms.items():
        h = call(rc.dendrogram, "average")
        assert h["merges"].tobytes() == want["merges"].tobytes() and np.array_equal(h["binder_num"], want["binder_num"]), name
        clust, info = call(rc.dendrogrampointestimate, "VI", maxK=3)
        assert np.array_equal(info["loss"], vilb) and np.array_equal(clust, _lib.hclust_cut_large(want["merges"], n, info["K"])), name
    ctx.close()
    with pytest.raises(ValueError, match="8192"):
        rc.dendrogrampointestimate(C, numsamples=m, criterion="posterior", data=d["distancematrix"], r=1.0, p=0.5, params=P, polish=True)


def test_the_large_entries_refuse_beyond_their_capacity_before_any_device_work():
    L = _lib.lib()
    buf, out = np.zeros(64, np.int64), np.zeros(64)
    p = lambda x: x.ctypes.data
    for n, m in ((32768, 3), (8, 2 ** 28)):                             # n above 32767; m·n = 2^31
        calls = [lambda: L.rc_hclust_large(0, p(buf), m, n, 0, p(buf), p(buf), 0, None, None),
                 lambda: L.rc_hclust_large_samples(0, p(buf), m, n, 0, p(buf), p(buf), 0, None, None, None),
                 lambda: L.rc_psm_expected_loss_large(0, p(buf), m, n, 0, 1, p(buf), p(out), p(buf), None)]
        for call in calls:
            assert call() == CAP and "32767" in L.rc_last_error(None).decode(), (n, m)
    assert L.rc_hclust_cut_large(p(buf), 32768, 1, p(buf)) == ARG and "32767" in L.rc_last_error(None).decode()
