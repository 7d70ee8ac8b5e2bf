"""CPU checks of the fitprior / k-medoids layer: the NumPy restatement of the device k-medoids (tests/kmedoids_ref.py)
against brute force and against its own sampling law, detectknee (src/prior.jl:340-360), the maximum-likelihood fits,
sample_rp (src/mcmc.jl:592-636), fitprior's argument checks (src/prior.jl:30-56) and the C ABI of the new entry points."""
import os
import re

import numpy as np
import pytest
import scipy.stats as st

import kmedoids_ref as KR
import redclust_amd as rc
from redclust_amd import prior as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_int_matrix(rng, n, hi):
    A = rng.integers(1, hi, size=(n, n)).astype(np.int64)
    D = np.triu(A, 1)
    return D + D.T


@pytest.mark.parametrize("seed", range(6))
def test_medoid_update_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    n, k = int(rng.integers(5, 40)), int(rng.integers(1, 6))
    Dq = random_int_matrix(rng, n, 4 if seed % 2 else 1000)   # small range: many ties
    a = rng.integers(0, k, n)
    a[:k] = np.arange(k)                                      # no empty group
    med = KR.update_medoids(Dq, a, k)
    for g in range(k):
        best = None
        for i in range(n):
            if a[i] != g:
                continue
            c = sum(int(Dq[h, i]) for h in range(n) if a[h] == g)
            if best is None or c < best[0]:                   # strict <: the lowest index keeps a tie
                best = (c, i)
        assert med[g] == best[1]


def test_assignment_ties_go_to_the_first_medoid():
    Dq = np.array([[0, 2, 2], [2, 0, 5], [2, 5, 0]], np.int64)
    a, tc = KR.assign(Dq, [2, 1])
    assert list(a) == [0, 1, 0] and tc == 2                 # point 0 is 2 from both medoids: the first one (point 2) wins


def test_seeding_draws_follow_the_min_costs():
    w = np.array([0, 3, 1, 0, 6, 2], np.int64)
    N = 24000
    cnt = np.bincount([KR.draw(w, KR.u53(s, 6, 1)) for s in range(N)], minlength=len(w))
    prob = w / w.sum()
    assert cnt[0] == 0 and cnt[3] == 0
    assert np.max(np.abs(cnt / N - prob)) < 4 * np.sqrt(0.25 / N)


def test_kmpp_seeds_are_distinct_and_runs_converge():
    rng = np.random.default_rng(3)
    Dq = random_int_matrix(rng, 30, 10 ** 6)
    for k in (1, 2, 7, 30):
        s = KR.kmpp_seeds(Dq, k, 5)
        assert len(set(s)) == k
        r = KR.kmedoids(Dq, 20, k, seed=5)
        assert r["converged"] and sorted(set(r["assignments"])) == list(range(1, k + 1))
        assert np.all(r["assignments"][r["medoids"] - 1] == np.arange(1, k + 1))


def test_detectknee_hand_computed():
    # line through (1, 10) and (5, 2): y = 12 - 2x; distances of the inner points 4, 3, 1.5 (over sqrt 5)
    assert rc.detectknee([1, 2, 3, 4, 5], [10, 4, 3, 2.5, 2]) == (2, 4.0)
    assert rc.detectknee([5, 3, 1, 4, 2], [2, 3, 10, 2.5, 4]) == (2, 4.0)   # sorted by x first
    assert rc.detectknee([1, 2, 3], [3.0, 2.0, 1.0])[0] == 1                # a straight line: all distances 0, the first wins
    assert rc.detectknee([4, 5, 6, 7], [9.0, 1.0, 0.5, 0.0])[0] == 5


def test_beta_and_gamma_mle_against_scipy():
    rng = np.random.default_rng(0)
    x = rng.beta(2.5, 7.0, size=4000)
    u, v = PR._beta_mle(x)
    su, sv, _, _ = st.beta.fit(x, floc=0, fscale=1)
    assert np.allclose([u, v], [su, sv], rtol=1e-4)
    y = rng.gamma(3.0, 0.5, size=4000)
    shape, rate = PR._gamma_mle(y)
    sa, _, sscale = st.gamma.fit(y, floc=0)
    assert np.allclose([shape, rate], [sa, 1 / sscale], rtol=1e-4)


def test_sample_rp_equals_explicit_loop():
    sizes = np.array([5, 0, 12, 3, 0, 1, 9])
    opts = rc.MCMCOptionsList(numiters=300, burnin=50, thin=2)
    got = rc.sample_rp(sizes, opts, verbose=False, seed=21)
    rng = np.random.default_rng(21)
    P = rc.PriorHyperparamsList()
    C = sizes[sizes > 0]
    r, p = rng.gamma(P.eta, P.sigma), rng.beta(P.u, P.v)
    rs, ps = [], []
    for i in range(1, 301):
        r, _ = rc.sample_r(rng, r, p, C, len(C), P.eta, P.sigma, P.proposalsd_r)
        p = rc.sample_p(rng, len(C), int(C.sum()), r, P.u, P.v)
        if i > 50 and (i - 50) % 2 == 0:
            rs.append(r); ps.append(p)
    assert np.array_equal(got["r"], rs) and np.array_equal(got["p"], ps)


def test_fitprior_argument_checks():
    D = np.abs(np.subtract.outer(np.arange(6.0), np.arange(6.0)))
    pts = np.random.default_rng(0).normal(size=(10, 3))
    with pytest.raises(ValueError, match="not square"):
        rc.fitprior(pts, "k-medoids", True, verbose=False)
    with pytest.raises(ValueError, match="k-means"):
        rc.fitprior(D, "k-means", True, verbose=False)
    with pytest.raises(NotImplementedError, match="k-medoids"):
        rc.fitprior(pts, "k-means", verbose=False)
    with pytest.raises(ValueError, match="Algo"):
        rc.fitprior(D, "pam", True, verbose=False)
    with pytest.raises(ValueError, match="Kmin and Kmax"):
        rc.fitprior(D, "k-medoids", True, Kmin=4, Kmax=3, verbose=False)
    with pytest.raises(ValueError, match="Kmin and Kmax"):
        rc.fitprior(D, "k-medoids", True, Kmax=7, verbose=False)
    with pytest.raises(ValueError, match="Kmin and Kmax"):
        rc.fitprior(D, "k-medoids", True, Kmin=0, verbose=False)
    with pytest.raises(ValueError, match="diss = true"):
        rc.fitprior([list(r) for r in pts], "k-medoids", True, verbose=False)


def test_new_prototypes_are_bound():
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    for name, nargs in (("rc_kmedoids", 10), ("rc_kmedoids_scan", 9)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        assert len(args) == nargs and len(rc.SIGNATURES[name][1]) == nargs, name
