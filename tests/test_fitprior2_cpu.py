"""CPU checks of fitprior2 / sampleK / sampledist (prior.py): the weighted likelihood fit against a literal restatement of
src/prior.jl:238-266 (explicit A_k / B_k vectors, Distributions' weighted sufficient statistics and its Newton shape fit),
its fallbacks and zero-weight error, pmf (src/prior.jl:362-367), the vectorised Philox of tests/samplek_ref.py, the
argument checks (which raise before any device is touched), sampledist's moments and the C ABI of the new entry points."""
import os
import re
import warnings

import numpy as np
import pytest
from scipy.special import digamma, polygamma

import np_transcription as T
import samplek_ref as SR
import redclust_amd as rc
from redclust_amd import prior as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gamma_shape_distributions(sx, slogx, tw, tol=1e-16, maxiter=1000):
    """fit_mle(Gamma, ::GammaStats) of Distributions.jl: the shape by its Newton iteration on the weighted statistics."""
    mx, mlogx = sx / tw, slogx / tw
    logmx = np.log(mx)
    a = (logmx - mlogx) / 2
    for _ in range(maxiter):
        ia = 1 / a
        z = ia + (mlogx - logmx + np.log(a) - digamma(a)) / (a * a * (ia - polygamma(1, a)))
        a_new = 1 / z
        if abs(a_new - a) <= tol * a:
            return float(a_new)
        a = a_new
    return float(a)


def literal_fit(D, labellings, Kprior, Kmin, Kmax):
    """src/prior.jl:211-266 as written: A_k / B_k vectors of the upper triangle, weights repeated per entry."""
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    out = []
    for same_side in (True, False):
        vec, wts, sz = [], [], []
        for k in range(Kmin, Kmax + 1):
            lab = labellings[k]
            same = (lab[:, None] == lab[None, :])[iu]
            x = D[iu][same if same_side else ~same]
            vec.append(x); sz.append(len(x)); wts.append(np.full(len(x), Kprior[k - 1]))
        x, w = np.concatenate(vec), np.concatenate(wts)
        if len(x) == 0:
            out += [1.0, 1.0, 1.0]
            continue
        sx = slx = tw = 0.0
        for xi, wi in zip(x, w):   # suffstats(GammaStats, x, w): one pass in order
            sx += wi * xi; slx += wi * np.log(xi); tw += wi
        shape = gamma_shape_distributions(sx, slx, tw)
        out += [shape, float(np.sum(np.array(sz) * Kprior[Kmin - 1:Kmax])) * shape, float(np.sum(x * w))]
    return out


def stats_of(D, labellings, Kmin, Kmax):
    iu = np.triu_indices(D.shape[0], 1)
    st = {f"{a}_{b}": [] for a in ("count", "sum", "sumlog") for b in ("within", "between")}
    for k in range(Kmin, Kmax + 1):
        lab = labellings[k]
        same = (lab[:, None] == lab[None, :])[iu]
        for side, m in (("within", same), ("between", ~same)):
            x = D[iu][m]
            st["count_" + side].append(len(x)); st["sum_" + side].append(x.sum()); st["sumlog_" + side].append(np.log(x).sum())
    return st


def small_case(seed, n=14):
    rng = np.random.default_rng(seed)
    P = rng.normal(size=(n, 2))
    D = np.sqrt(((P[:, None] - P[None]) ** 2).sum(-1))
    labellings = {k: (np.arange(n) % k) + 1 if k > 1 else np.ones(n, np.int64) for k in range(1, n + 1)}
    for k in range(2, n):
        labellings[k] = rng.permutation(labellings[k])
    Kprior = rng.dirichlet(np.ones(n))
    return D, labellings, Kprior


@pytest.mark.parametrize("seed,Kmin,Kmax", [(0, 1, 7), (1, 2, 13), (2, 3, 3), (3, 1, 14)])
def test_fit_weighted_equals_literal_restatement(seed, Kmin, Kmax):
    D, labellings, Kprior = small_case(seed)
    want = literal_fit(D, labellings, Kprior, Kmin, Kmax)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = PR._fit_weighted(stats_of(D, labellings, Kmin, Kmax), Kprior, Kmin, Kmax)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w), (got, want)


def test_fit_weighted_fallbacks_and_zero_weight():
    D, labellings, Kprior = small_case(5)
    n = D.shape[0]
    with pytest.warns(UserWarning, match="single cluster.*repulsion"):
        got = PR._fit_weighted(stats_of(D, labellings, 1, 1), Kprior, 1, 1)
    assert got[3:] == (1.0, 1.0, 1.0) and got[0] != 1.0
    with pytest.warns(UserWarning, match="all singletons.*cohesion"):
        got = PR._fit_weighted(stats_of(D, labellings, n, n), Kprior, n, n)
    assert got[:3] == (1.0, 1.0, 1.0) and got[3] != 1.0
    zero = Kprior.copy()
    zero[2:6] = 0.0
    with pytest.raises(ValueError, match="no weight on Kmin..Kmax = 3..6"):
        PR._fit_weighted(stats_of(D, labellings, 3, 6), zero, 3, 6)


def test_pmf_and_padding():
    X = np.array([3, 5, 3, 4, 3, 5])
    want = [0, 0, 3 / 6, 1 / 6, 2 / 6]                         # zeros for 1..min(X)-1, then counts over min..max
    assert np.array_equal(rc.pmf(X), want)
    assert np.array_equal(rc.pmf(X, 8), want + [0, 0, 0])
    assert np.array_equal(rc.pmf([1, 1, 2]), [2 / 3, 1 / 3])
    with pytest.raises(ValueError):
        rc.pmf([0, 1])


def test_vectorised_philox_equals_transcription():
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, size=(300, 4), dtype=np.uint64)
    for key in ((0, 0), (123456789, 0x534D504B), (2 ** 32 - 1, 2 ** 31 + 7)):
        got = SR.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key)
        for t in range(len(ctr)):
            assert tuple(int(g[t]) for g in got) == T.philox4x32_10(tuple(int(c) for c in ctr[t]), key)
    u = SR.uniforms(2 ** 40 + 5, np.arange(1, 9), 2 ** 33 + 1)
    for K in range(1, 9):
        c = T.philox4x32_10((K, 1, 2, 0), ((2 ** 40 + 5) & 0xFFFFFFFF, ((2 ** 40 + 5) >> 32) ^ 0x534D504B))
        assert u[K - 1] == ((((c[0] << 32) | c[1]) >> 12) + 0.5) * 2.0 ** -52


def test_restated_draw_rules():
    assert SR.draw(1, 2.0, 0.4, 0, 0)[0] == 1
    assert SR.draw(9, 1.5, 1.0, 0, 3) == (1, np.inf)            # p = 1: every lp is -inf -> K = 1
    assert SR.draw(9, 1.5, 0.0, 0, 3)[0] == 9                   # p = 0: only lp[n] = 0 is finite
    lp = SR.logprobs(6, 0.7, 0.3)
    K = np.arange(1, 6)
    from scipy.special import betaln
    assert np.allclose(lp[:-1], 0.7 * K * np.log(0.7) + (6 - K) * np.log(0.3) - np.log(6 - K) - betaln(0.7 * K, 6 - K), rtol=1e-12)


def test_argument_checks_before_the_device():
    D = np.abs(np.subtract.outer(np.arange(6.0), np.arange(6.0)))
    pts = np.random.default_rng(0).normal(size=(10, 3))
    with pytest.raises(NotImplementedError, match="fitprior2.*k-medoids"):
        rc.fitprior2(pts, "k-means", verbose=False)
    with pytest.raises(ValueError, match="k-means"):
        rc.fitprior2(D, "k-means", True, verbose=False)
    with pytest.raises(ValueError, match="Algo"):
        rc.fitprior2(D, "pam", True, verbose=False)
    for bad in (dict(Kmin=4, Kmax=3), dict(Kmax=7), dict(Kmin=0)):
        with pytest.raises(ValueError, match="Kmin and Kmax"):
            rc.fitprior2(D, "k-medoids", True, verbose=False, **bad)
    with pytest.raises(ValueError, match="not square"):
        rc.fitprior2(pts, "k-medoids", True, verbose=False)
    with pytest.raises(ValueError, match="diss = true"):
        rc.fitprior2([list(r) for r in pts], "k-medoids", True, verbose=False)
    P = rc.PriorHyperparamsList()
    with pytest.raises(ValueError, match="n must be a positive integer"):
        rc.sampleK(P, 10, 0)
    with pytest.raises(ValueError, match="numsamples must be a positive integer"):
        rc.sampleK(1.0, 1.0, 1.0, 1.0, 0, 5)
    with pytest.raises(TypeError):
        rc.sampleK(P, 10)
    with pytest.raises(ValueError, match="type must be"):
        rc.sampledist(P, "cluster", 3)
    with pytest.raises(ValueError, match="numsamples must be a positive integer"):
        rc.sampledist(P, "intracluster", 0)


@pytest.mark.parametrize("kind", ["intracluster", "intercluster"])
def test_sampledist_mean(kind):
    P = rc.PriorHyperparamsList(delta1=2.0, alpha=9.0, beta=4.0, delta2=5.0, zeta=12.0, gamma=30.0)
    a, b, d = (P.alpha, P.beta, P.delta1) if kind == "intracluster" else (P.zeta, P.gamma, P.delta2)
    m = 200000
    x = rc.sampledist(P, kind, m, seed=3)
    assert x.shape == (m,) and np.all(x > 0)
    mean = d * b / (a - 1)
    var = d * b * b * (d + a - 1) / ((a - 1) ** 2 * (a - 2))     # E[x²] = δ(δ+1) b² / ((a-1)(a-2))
    assert abs(x.mean() - mean) < 4 * np.sqrt(var / m), (x.mean(), mean)


def test_new_prototypes_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    for name, nargs in (("rc_kmedoids_scan_split", 10), ("rc_sample_k", 8), ("rc_kmedoids_scan", 9)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        assert len(args) == nargs and len(rc.SIGNATURES[name][1]) == nargs, name
