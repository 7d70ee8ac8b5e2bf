"""fitprior (prior.py: batched device k-medoids scan, elbow, notional clustering, device A / B split, host fits) against a
host composition of the same steps, and runsampler's default parameters and starting state (src/mcmc.jl:516-527)."""
import os

import numpy as np
import pytest

import kmedoids_ref as KR
import redclust_amd as rc
from redclust_amd import prior as PR
from redclust_amd.datagen import _gamma_shape_mle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("delta1", "delta2", "alpha", "beta", "zeta", "gamma", "eta", "sigma", "proposalsd_r", "u", "v")


def paper(i):
    d = np.load(os.path.join(HERE, "golden", "paper_datasets.npz"))
    return d[f"D{i}"], d[f"labels{i}"].astype(np.int64)


def host_fitprior(ctx, seed):
    """The restatement's scan, detectknee, a host A / B split over the device's matrix (exact integer sums, as the
    device forms them), the same sample_rp chain and fits."""
    Dq, eD = KR.device_matrix(ctx)
    n = Dq.shape[0]
    L = ctx.get_matrix(1)
    _, _, _, eL = ctx.debug_rowsums(1)
    Lq = np.rint(np.ldexp(L, eL)).astype(np.int64)
    s_scan = PR.kmedoids_stream_seed(seed, PR.KMED_STREAM_SCAN)
    cost = [KR.kmedoids(Dq, eD, k, maxiter=1000, seed=s_scan)["totalcost"] for k in range(1, n // 2 + 1)]
    K = int(rc.detectknee(np.arange(1, n // 2 + 1), cost)[0])
    lab = KR.kmedoids(Dq, eD, K, maxiter=1000, seed=PR.kmedoids_stream_seed(seed, PR.KMED_STREAM_NOTIONAL))["assignments"]
    iu = np.triu_indices(n, 1)
    same = (lab[:, None] == lab[None, :])[iu]
    cA, cB = int(same.sum()), int((~same).sum())
    sA, sB = float(int(Dq[iu][same].sum())) * 2.0 ** -eD, float(int(Dq[iu][~same].sum())) * 2.0 ** -eD
    lA, lB = float(int(Lq[iu][same].sum())) * 2.0 ** -eL, float(int(Lq[iu][~same].sum())) * 2.0 ** -eL
    temp = rc.sample_rp(np.bincount(lab)[1:], verbose=False, seed=seed)
    eta, sigma = PR._gamma_mle(temp["r"])
    u, v = PR._beta_mle(temp["p"])
    d1 = _gamma_shape_mle(sA / cA, lA / cA)
    d2 = _gamma_shape_mle(sB / cB, lB / cB)
    return K, lab, dict(delta1=d1, delta2=d2, alpha=cA * d1, beta=sA, zeta=cB * d2, gamma=sB, eta=eta, sigma=sigma,
                        proposalsd_r=float(np.std(temp["r"], ddof=1)), u=u, v=v)


@pytest.mark.parametrize("ds", [1, 2, 3])
def test_fitprior_equals_host_composition(ds):
    D, _ = paper(ds)
    P = rc.fitprior(D, "k-medoids", True, verbose=False, seed=4)
    ctx = rc.Context(D)
    K, _, ref = host_fitprior(ctx, 4)
    ctx.close()
    assert P.K_initial == K
    for f in FIELDS:
        assert abs(getattr(P, f) - ref[f]) <= 1e-12 * abs(ref[f]), (f, getattr(P, f), ref[f])


@pytest.mark.parametrize("ds", [1, 2, 3])
def test_notional_K_near_the_true_cluster_count(ds):
    """Sanity bound, not parity: the elbow of the k-medoids cost curve lands within a factor of two of the number of
    clusters the paper's datasets were generated with."""
    D, truth = paper(ds)
    P = rc.fitprior(D, "k-medoids", True, verbose=False)
    Ktrue = len(np.unique(truth))
    assert Ktrue / 2 <= P.K_initial <= 2 * Ktrue, (P.K_initial, Ktrue)


def test_fitprior_points_and_ctx_reuse():
    data = rc.generatemixture(300, 5, seed=8, points_only=True)
    P1 = rc.fitprior(data["points"], "k-medoids", verbose=False, seed=1)
    ctx = rc.Context.from_points(data["points"])
    P2 = rc.fitprior(rc.MCMCData(data["points"]), "k-medoids", verbose=False, seed=1, ctx=ctx)
    ctx.close()
    assert vars(P1) == vars(P2)


def _explicit_composition(data, options, seed):
    ctx = (rc.Context.from_points(data.points) if data.points is not None else rc.Context(data.D))
    params = rc.fitprior(data, "k-medoids", True, verbose=False, seed=seed, ctx=ctx)
    k0 = min(params.maxK, params.K_initial) if params.maxK > 0 else params.K_initial
    clusts = ctx.kmedoids(k0, maxiter=1000, seed=PR.kmedoids_stream_seed(seed, PR.KMED_STREAM_INIT)).assignments
    ctx.close()
    rng = np.random.default_rng(seed)
    init = rc.MCMCState(clusts, rng.gamma(params.eta, 1.0 / params.sigma), rng.beta(params.u, params.v))
    return rc.runsampler(data, options, params, init, verbose=False, seed=seed)


@pytest.mark.parametrize("kind", ["D", "points"])
def test_runsampler_defaults_equal_explicit_composition(kind):
    if kind == "D":
        data = rc.MCMCData(paper(1)[0])
    else:
        data = rc.MCMCData(rc.generatemixture(200, 4, seed=2, points_only=True)["points"])
    opts = rc.MCMCOptionsList(numiters=60, burnin=10)
    a = rc.runsampler(data, opts, verbose=False, seed=3)
    b = rc.runsampler(data, opts, verbose=False, seed=3)
    c = _explicit_composition(data, opts, 3)
    for x in (b, c):
        assert vars(x.params) == vars(a.params)
        assert np.array_equal(np.stack(x.clusts), np.stack(a.clusts))
        assert np.array_equal(x.r, a.r) and np.array_equal(x.p, a.p) and np.array_equal(x.loglik, a.loglik)
        assert np.array_equal(x.posterior_coclustering, a.posterior_coclustering)
    d = rc.runsampler(data, opts, verbose=False, seed=4)
    assert not (np.array_equal(d.r, a.r) and vars(d.params) == vars(a.params))
