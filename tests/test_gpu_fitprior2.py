"""fitprior2 on the device: the k-medoids scan's per-k split (rc_kmedoids_scan_split) against rc_within_between of the
same labelling, bit for bit, on every kind of context; fitprior2 against fitprior (Kmin = 1: the same elbow and partition
prior) and against the explicit composition scan -> sampleK -> pmf -> _fit_weighted; the reference's edge cases and inputs."""
import os

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import prior as PR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WB = ("count_within", "count_between", "sum_within", "sumlog_within", "sum_between", "sumlog_between")


def check_split(ctx, kmin, kmax, ks, seed, maxiter=1000):
    scan = ctx.kmedoids_scan(kmin, kmax, maxiter=maxiter, seed=seed, split=True)
    plain = ctx.kmedoids_scan(kmin, kmax, maxiter=maxiter, seed=seed)
    for f in ("totalcost", "iterations", "converged"):
        assert np.array_equal(scan[f], plain[f]), f
    for k in ks:
        ctx.set_state(ctx.kmedoids(k, maxiter=maxiter, seed=seed).assignments)
        wb = ctx.within_between()
        for f in WB:
            assert scan[f][k - kmin] == wb[f], (k, f, scan[f][k - kmin], wb[f])
    return scan


def elbow(scan, kmin, kmax):
    return int(rc.detectknee(np.arange(kmin, kmax + 1), scan["totalcost"])[0])


def test_split_mixture_500():
    D = rc.generatemixture(500, 12, seed=1)["distancematrix"]
    ctx = rc.Context(D)
    scan = check_split(ctx, 1, 500, [500, 1, 2, 3, 40, 250, 499], seed=11)
    check_split(ctx, 1, 250, [elbow(scan, 1, 250)], seed=11)
    ctx.close()


def test_split_32bit_storage():
    D = rc.generatemixture(400, 8, seed=2)["distancematrix"]
    ctx = rc.Context(D, storage_bits=32)
    scan = check_split(ctx, 1, 200, [200, 1, 2, 7, 150], seed=5)
    check_split(ctx, 1, 200, [elbow(scan, 1, 200)], seed=5)
    ctx.close()


def test_split_from_points():
    pts = rc.generatemixture(300, 6, dim=6, seed=3)["points"]
    ctx = rc.Context.from_points(pts)
    check_split(ctx, 2, 300, [300, 2, 3, 6, 77], seed=2 ** 40 + 3)
    ctx.close()


def test_split_stored_logd():
    # a pair of (nearly) coincident points: too few quanta to derive logD from Dq, so the context stores it
    D = rc.generatemixture(300, 10, seed=4)["distancematrix"]
    D[0, 1] = D[1, 0] = D.max() * 1e-13
    ctx = rc.Context(D)
    check_split(ctx, 1, 150, [150, 1, 2, 10, 90], seed=8)
    ctx.close()
    ctx = rc.Context(D, logD=rc.MCMCData(D).logD)                # the caller's logD: stored as well
    check_split(ctx, 1, 150, [1, 2, 33], seed=8)
    ctx.close()


def test_split_8192_spans_chunks():
    D = rc.generatemixture(8192, 20, seed=0)["distancematrix"]
    ctx = rc.Context(D)
    scan = check_split(ctx, 1, 4096, [4096, 1, 2, 20, 1000, 1913, 1914, 3500], seed=6)
    K = elbow(scan, 1, 4096)
    ctx.set_state(ctx.kmedoids(K, maxiter=1000, seed=6).assignments)
    wb = ctx.within_between()
    assert all(scan[f][K - 1] == wb[f] for f in WB)
    ctx.close()


def test_fitprior2_partition_prior_equals_fitprior():
    D = rc.generatemixture(300, 10, seed=7)["distancematrix"]
    P1 = rc.fitprior(D, "k-medoids", True, verbose=False, seed=3)
    P2 = rc.fitprior2(D, "k-medoids", True, verbose=False, seed=3)
    for f in ("K_initial", "eta", "sigma", "u", "v", "proposalsd_r"):
        assert getattr(P1, f) == getattr(P2, f), f


@pytest.mark.parametrize("Kmin,Kmax", [(1, None), (3, 40)])
def test_fitprior2_equals_explicit_composition(Kmin, Kmax):
    D = rc.generatemixture(240, 8, seed=9)["distancematrix"]
    seed, N = 12, 240
    Kmax_ = N // 2 if Kmax is None else Kmax
    P = rc.fitprior2(D, "k-medoids", True, Kmin=Kmin, Kmax=Kmax_, verbose=False, seed=seed)
    ctx = rc.Context(D)
    scan = ctx.kmedoids_scan(Kmin, Kmax_, maxiter=1000, seed=PR.kmedoids_stream_seed(seed, PR.KMED_STREAM_SCAN), split=True)
    K = elbow(scan, Kmin, Kmax_)
    notional = ctx.kmedoids(K, maxiter=1000, seed=PR.kmedoids_stream_seed(seed, PR.KMED_STREAM_NOTIONAL)).assignments
    ctx.close()
    sd, eta, sigma, u, v = PR._partition_prior(notional, False, seed)
    Ks = rc.sampleK(eta, sigma, u, v, max(10000, 100 * N), N, seed=PR.kmedoids_stream_seed(seed, PR.SAMPLEK_STREAM))
    got = (P.delta1, P.alpha, P.beta, P.delta2, P.zeta, P.gamma)
    assert got == PR._fit_weighted(scan, rc.pmf(Ks, N), Kmin, Kmax_)
    assert P.K_initial == K and (P.eta, P.sigma, P.u, P.v, P.proposalsd_r) == (eta, sigma, u, v, sd)


def test_fitprior2_edge_cases_warn_and_fall_back():
    pts = rc.generatemixture(20, 3, dim=3, seed=5)["points"]
    with pytest.warns(UserWarning, match="Falling back to defaults for repulsion"):
        P = rc.fitprior2(pts, "k-medoids", Kmin=1, Kmax=1, verbose=False)
    assert P.K_initial == 1 and (P.delta2, P.zeta, P.gamma) == (1.0, 1.0, 1.0)
    with pytest.warns(UserWarning, match="Falling back to defaults for cohesion"):
        P = rc.fitprior2(pts, "k-medoids", Kmin=20, Kmax=20, verbose=False)
    assert P.K_initial == 20 and (P.delta1, P.alpha, P.beta) == (1.0, 1.0, 1.0)


def test_fitprior2_inputs():
    g = rc.generatemixture(150, 5, dim=5, seed=8)
    pts, D = g["points"], g["distancematrix"]
    Pp = rc.fitprior2(pts, "k-medoids", verbose=False, seed=1)
    Pl = rc.fitprior2([list(x) for x in pts], "k-medoids", verbose=False, seed=1)
    Pd = rc.fitprior2(D, "k-medoids", True, verbose=False, seed=1)
    Pm = rc.fitprior2(rc.MCMCData(D), "k-medoids", verbose=False, seed=1)
    assert Pp == Pl and Pd == Pm
    for P in (Pp, Pd):
        assert 1 <= P.K_initial <= 75 and all(np.isfinite([P.delta1, P.alpha, P.beta, P.delta2, P.zeta, P.gamma]))
    ctx = rc.Context(D)
    ctx.set_state(np.ones(150, np.int64))
    assert rc.fitprior2(D, "k-medoids", True, verbose=False, seed=1, ctx=ctx) == Pd
    assert ctx.get_state()[2] == 1                              # the context's state is left as it was
    ctx.close()
