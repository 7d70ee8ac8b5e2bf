"""The k-means prior fits on the device: the scan's per-k split (rc_kmeans_scan_split) against rc_within_between of the same
labelling, bit for bit; fitprior_kmeans against the composition of the public pieces it is made of; fitprior2_kmeans
against fitprior_kmeans (Kmin = 1: the same elbow and partition prior) and against its own composition; the inputs the
reference refuses and the unchanged refusal of the string "k-means"."""
import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import prior as PR
from redclust_amd.datagen import _gamma_shape_mle

pytestmark = pytest.mark.gpu
WB = ("count_within", "count_between", "sum_within", "sumlog_within", "sum_between", "sumlog_between")
FIELDS = ("delta1", "delta2", "alpha", "beta", "zeta", "gamma", "eta", "sigma", "proposalsd_r", "u", "v", "K_initial")


@pytest.fixture(scope="module")
def pts():
    p = rc.generatemixture(200, 4, dim=4, seed=9, sigma=0.2, points_only=True)["points"]
    p.setflags(write=False)
    return p


def test_scan_split_equals_within_between(pts):
    n = len(pts)
    ctx = rc.Context.from_points(pts)
    scan = ctx.kmeans_scan(1, n, maxiter=1000, seed=21, split=True)
    plain = ctx.kmeans_scan(1, n, maxiter=1000, seed=21)
    chunked = ctx.kmeans_scan(1, n, maxiter=1000, seed=21, split=True, slots_per_chunk=33)
    for f in ("totalcost", "iterations", "converged"):
        assert np.array_equal(scan[f], plain[f]), f
    for f in scan:
        assert np.array_equal(scan[f], chunked[f]), f
    for k in (1, 2, 3, 4, 17, n // 2, n - 1, n):
        ctx.set_state(ctx.kmeans(k, maxiter=1000, seed=21).assignments)
        wb = ctx.within_between()
        for f in WB:
            assert scan[f][k - 1] == wb[f], (k, f, scan[f][k - 1], wb[f])
    assert scan["count_within"][0] == n * (n - 1) // 2 and scan["count_within"][n - 1] == 0
    sub = ctx.kmeans_scan(3, 40, maxiter=1000, seed=21, split=True)   # kmin > 1
    for f in scan:
        assert np.array_equal(sub[f], scan[f][2:40]), f
    ctx.close()


def test_scan_split_on_32_bit_storage():
    """The split of rc_kmeans_scan_split on a context that stores D in 32 bits.  n = 130: two full waves plus two lanes, a
    partial 256-thread tile, and at k = 1 a group that takes both the "> 64 members" and the "> n/16" branches.  (dim = 3: the
    smallest generatemixture accepts for three components.)"""
    p = rc.generatemixture(130, 3, dim=3, seed=4, points_only=True)["points"]
    ctx = rc.Context.from_points(p, storage_bits=32)
    scan = ctx.kmeans_scan(1, 130, maxiter=1000, seed=3, split=True)
    chunked = ctx.kmeans_scan(1, 130, maxiter=1000, seed=3, split=True, slots_per_chunk=7)
    assert set(scan) == set(chunked) and set(WB) <= set(scan)
    for f in scan:
        assert np.array_equal(scan[f], chunked[f]), f
    for k in (1, 2, 3, 17, 129, 130):
        ctx.set_state(ctx.kmeans(k, maxiter=1000, seed=3).assignments)
        wb = ctx.within_between()
        for f in WB:
            assert scan[f][k - 1] == wb[f], (k, f, scan[f][k - 1], wb[f])
    ctx.close()


def compose_fitprior(ctx, n, seed, Kmin=1, Kmax=None):
    """fitprior_kmeans from the public pieces: scan -> elbow -> notional run -> set_state / within_between -> host fits."""
    Kmax = n // 2 if Kmax is None else Kmax
    scan = ctx.kmeans_scan(1, Kmax - Kmin + 1, maxiter=1000, seed=PR.kmedoids_stream_seed(seed, PR.KMED_STREAM_SCAN))
    K = int(rc.detectknee(np.arange(Kmin, Kmax + 1), scan["totalcost"])[0])
    lab = ctx.kmeans(K, maxiter=1000, seed=PR.kmedoids_stream_seed(seed, 1)).assignments
    ctx.set_state(lab)
    wb = ctx.within_between()
    proposalsd_r, eta, sigma, u, v = PR._partition_prior(lab, False, seed)
    cA, cB = wb["count_within"], wb["count_between"]
    d1 = _gamma_shape_mle(wb["sum_within"] / cA, wb["sumlog_within"] / cA)
    d2 = _gamma_shape_mle(wb["sum_between"] / cB, wb["sumlog_between"] / cB)
    return dict(delta1=d1, delta2=d2, alpha=cA * d1, beta=wb["sum_within"], zeta=cB * d2, gamma=wb["sum_between"], eta=eta,
                sigma=sigma, proposalsd_r=proposalsd_r, u=u, v=v, K_initial=K)


@pytest.mark.parametrize("Kmin,Kmax", [(1, None), (2, 60)])
def test_fitprior_kmeans_equals_composition(pts, Kmin, Kmax):
    P = rc.fitprior_kmeans(pts, Kmin=Kmin, Kmax=Kmax, verbose=False, seed=4)
    ctx = rc.Context.from_points(pts)
    ref = compose_fitprior(ctx, len(pts), 4, Kmin, Kmax)
    assert 1 < ref["K_initial"] < len(pts)
    for f in FIELDS:
        assert getattr(P, f) == ref[f], (f, getattr(P, f), ref[f])
    # the same through an MCMCData built from the points and a caller's context
    P2 = rc.fitprior_kmeans(rc.MCMCData(pts), Kmin=Kmin, Kmax=Kmax, verbose=False, seed=4, ctx=ctx)
    ctx.close()
    assert vars(P2) == vars(P)
    assert vars(rc.fitprior_kmeans(pts, Kmin=Kmin, Kmax=Kmax, verbose=False, seed=5)) != vars(P)


def test_fitprior2_kmeans_shares_the_partition_prior_and_equals_its_composition(pts):
    n, seed = len(pts), 4
    P1 = rc.fitprior_kmeans(pts, verbose=False, seed=seed)
    P2 = rc.fitprior2_kmeans(pts, verbose=False, seed=seed)
    for f in ("K_initial", "eta", "sigma", "u", "v", "proposalsd_r"):
        assert getattr(P2, f) == getattr(P1, f), f
    ctx = rc.Context.from_points(pts)
    scan = ctx.kmeans_scan(1, n // 2, maxiter=1000, seed=PR.kmedoids_stream_seed(seed, PR.KMED_STREAM_SCAN), split=True)
    ctx.close()
    Ks = rc.sampleK(P1.eta, P1.sigma, P1.u, P1.v, max(10000, 100 * n), n, seed=PR.kmedoids_stream_seed(seed, PR.SAMPLEK_STREAM))
    d1, al, be, d2, ze, ga = PR._fit_weighted(scan, rc.pmf(Ks, n), 1, n // 2)
    assert (P2.delta1, P2.alpha, P2.beta, P2.delta2, P2.zeta, P2.gamma) == (d1, al, be, d2, ze, ga)


def test_refused_inputs(pts):
    D = rc.MCMCData(pts).D
    for fn in (rc.fitprior_kmeans, rc.fitprior2_kmeans):
        with pytest.raises(ValueError, match="Cannot use algorithm `k-means` with a dissimilarity matrix"):
            fn(rc.MCMCData(D), verbose=False)
        ctx = rc.Context(D)   # a context that holds no observations
        with pytest.raises(ValueError, match="Cannot use algorithm `k-means` with a dissimilarity matrix"):
            fn(pts, verbose=False, ctx=ctx)
        ctx.close()
        with pytest.raises(ValueError, match="Kmin and Kmax"):
            fn(pts, Kmin=0, verbose=False)
        with pytest.raises(ValueError, match="Kmin and Kmax"):
            fn(pts, Kmax=len(pts) + 1, verbose=False)
    for fn in (rc.fitprior, rc.fitprior2):   # the string still reaches no k-means
        with pytest.raises(NotImplementedError, match="k-medoids"):
            fn(pts, "k-means", verbose=False)
        with pytest.raises(ValueError, match="Cannot use algorithm `k-means` with a dissimilarity matrix"):
            fn(D, "k-means", True, verbose=False)
