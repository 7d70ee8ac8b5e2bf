"""A nonzero diagonal of D through the CPU references (-m "not gpu").

The reference keeps D's diagonal as given: types.jl:155 zeroes only logD's.  loglik adds it (matsum(D, clust_k, clust_k)/2 of
mcmc.jl:32 includes D[i,i]); the Gibbs sweep never sees it, because the swept point is taken out of its cluster before its row
is summed.  This file pins both statements on the three restatements the GPU tests are held against (tests/test_gpu_diagonal.py):
the NumPy transcription, the literal oracle and the fixed-point ("stable") oracle, on paper dataset 2 (golden case d2_random)
with three diagonals — positive, mixed sign, and larger than every off-diagonal entry.
"""
import numpy as np
import pytest

import np_transcription as T
import oracle_lib as O
from helpers import cluster_terms_positive, golden_case, load_golden, rp_schedule, with_diagonal

NSWEEPS = 4


@pytest.mark.parametrize("kind", ["positive", "mixed", "large"])
def test_sweep_ignores_the_diagonal_and_loglik_sees_it(kind):
    g, d = load_golden()
    D0, P, init, seed = golden_case(g, d, "d2_random")
    n = D0.shape[0]
    assert np.all(np.diag(D0) == 0.0)
    D = with_diagonal(D0, kind)
    off = D0[~np.eye(n, dtype=bool)]
    if kind == "positive":
        assert np.all(np.diag(D) > 0)
    elif kind == "mixed":
        assert np.any(np.diag(D) < 0) and np.any(np.diag(D) > 0)
    else:
        assert np.diag(D).min() > off.max()

    o = O.Oracle(D, P)                                     # literal and stable sweeps: separate label states
    os_ = O.Oracle(D, P)
    oz = O.Oracle(D0, P, eD=os_.eD, eL=os_.eL)             # the zero-diagonal chain of the same quantisation
    assert np.all(np.diag(o.logD) == 0.0) and np.all(np.diag(o.Lq) == 0)           # types.jl:155
    logD = T.make_logD(D)
    assert np.all(np.diag(logD) == 0.0)
    assert np.array_equal(logD, T.make_logD(D0))
    assert np.array_equal(np.diag(os_.Dq), np.rint(np.ldexp(np.diag(D), os_.eD)).astype(np.int64))
    m = ~np.eye(n, dtype=bool)
    assert np.array_equal(os_.Dq[m], oz.Dq[m]) and np.array_equal(os_.Lq, oz.Lq)

    for x in (o, os_, oz):
        x.set_state(init)
    clusts = init.copy()
    sizes, K = T.state_from_labels(clusts)
    for t in range(NSWEEPS):
        r, p = rp_schedule(t)
        K = T.sweep(D, logD, clusts, sizes, P, r, p, seed, t)
        o.sweep_literal(r, p, seed, t)
        os_.sweep_stable(r, p, seed, t)
        oz.sweep_stable(r, p, seed, t)
        assert np.array_equal(clusts, o.clusts) and K == o.K, (kind, t)
        assert np.array_equal(os_.clusts, o.clusts) and os_.K == o.K, (kind, t)
        assert np.array_equal(oz.clusts, o.clusts) and oz.K == o.K, (kind, t)      # the sweep does not see the diagonal
        assert np.array_equal(sizes, o.sizes) and np.array_equal(os_.sizes, o.sizes)
        assert cluster_terms_positive(D, clusts, P["beta"]), (kind, t)
        ll_t = T.loglik(D, logD, clusts, sizes, P)
        ll_l, ll_s, ll_z = o.loglik_literal(), os_.loglik_stable(), oz.loglik_stable()
        assert np.isfinite(ll_t) and np.isfinite(ll_l) and np.isfinite(ll_s)
        assert abs(ll_t - ll_l) <= 1e-7 * max(1.0, abs(ll_l)), (kind, t, ll_t, ll_l)
        assert abs(ll_s - ll_l) <= 1e-7 * max(1.0, abs(ll_l)), (kind, t, ll_s, ll_l)
        assert abs(ll_s - ll_z) > 1e-3 * max(1.0, abs(ll_z)), (kind, t, ll_s, ll_z)  # loglik does see it
    assert len(np.unique(clusts)) > 1


def test_diagonal_moves_loglik_by_the_diagonal_term_only():
    """With one cluster the within-cluster sum is the whole matrix: loglik(D + diag) and loglik(D) differ exactly as
    β + ΣD/2 differs — the transcription's formula with the two sums put in."""
    g, d = load_golden()
    D0, P, init, _ = golden_case(g, d, "d2_random")
    n = D0.shape[0]
    D = with_diagonal(D0, "positive")
    one = np.ones(n, np.int64)
    sizes, _ = T.state_from_labels(one)
    logD = T.make_logD(D)
    a = T.loglik(D, logD, one, sizes, P)
    b = T.loglik(D0, logD, one, sizes, P)
    pairs = n * (n - 1) / 2
    shape = P["alpha"] + P["delta1"] * pairs
    expect = -shape * (np.log(P["beta"] + D.sum() / 2) - np.log(P["beta"] + D0.sum() / 2))
    assert abs(expect) > 1.0
    assert abs((a - b) - expect) <= 1e-12 * max(abs(a), abs(b)), (a - b, expect)   # (a few ulps of the two totals)
    o = O.Oracle(D, P)
    o.set_state(one)
    assert abs(o.loglik_stable() - a) <= 1e-7 * abs(a) and abs(o.loglik_literal() - a) <= 1e-7 * abs(a)
