"""GPU k-medoids (csrc/kmedoids.inc.hip through rc_kmedoids / rc_kmedoids_scan) against the NumPy restatement
(tests/kmedoids_ref.py): exact medoids, assignments, iteration counts and convergence flags, total cost to its double
rounding — single runs, the batched scan, 32-bit storage, distances computed from points — and the context's chain
state left untouched."""
import os

import numpy as np
import pytest

import kmedoids_ref as KR
import redclust_amd as rc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def paper(i):
    d = np.load(os.path.join(HERE, "golden", "paper_datasets.npz"))
    return d[f"D{i}"], d[f"labels{i}"].astype(np.int64)


def assert_same(res, ref):
    assert np.array_equal(res.medoids, ref["medoids"])
    assert np.array_equal(res.assignments, ref["assignments"])
    assert res.iterations == ref["iterations"] and res.converged == ref["converged"]
    assert res.totalcost == ref["totalcost"]


@pytest.mark.parametrize("ds", [1, 2, 3])
@pytest.mark.parametrize("seed", [0, 12345678901])
def test_paper_datasets_every_k_equals_restatement(ds, seed):
    D, _ = paper(ds)
    ctx = rc.Context(D)
    Dq, eD = KR.device_matrix(ctx)
    scan = ctx.kmedoids_scan(1, 50, maxiter=1000, seed=seed)
    for k in range(1, 51):
        ref = KR.kmedoids(Dq, eD, k, maxiter=1000, seed=seed)
        assert_same(ctx.kmedoids(k, maxiter=1000, seed=seed), ref)
        assert scan["totalcost"][k - 1] == ref["totalcost"] and scan["iterations"][k - 1] == ref["iterations"]
        assert bool(scan["converged"][k - 1]) == ref["converged"]
    ctx.close()


def test_mixture_2000_sampled_k():
    data = rc.generatemixture(2000, 20, seed=3)
    ctx = rc.Context(data["distancematrix"])
    Dq, eD = KR.device_matrix(ctx)
    for k in (1, 2, 3, 17, 250, 999, 1000):
        ref = KR.kmedoids(Dq, eD, k, seed=7)
        assert_same(ctx.kmedoids(k, seed=7), ref)
    ctx.close()


def test_scan_entries_equal_single_runs():
    """Every entry of a batched scan (one job, largest k first, converged runs dropping out) equals the single run."""
    data = rc.generatemixture(600, 8, seed=4, sigma=0.3)
    ctx = rc.Context(data["distancematrix"])
    scan = ctx.kmedoids_scan(5, 300, seed=11)
    for k in range(5, 301):
        r = ctx.kmedoids(k, seed=11)
        assert scan["totalcost"][k - 5] == r.totalcost and scan["iterations"][k - 5] == r.iterations, k
        assert bool(scan["converged"][k - 5]) == r.converged, k
    assert np.any(scan["iterations"] != scan["iterations"][0])   # runs of different lengths were batched together
    ctx.close()


def test_32bit_storage_context():
    data = rc.generatemixture(800, 10, seed=5)
    ctx = rc.Context(data["distancematrix"], storage_bits=32)
    Dq, eD = KR.device_matrix(ctx)
    scan = ctx.kmedoids_scan(1, 60, seed=2)
    for k in (1, 2, 10, 33, 60):
        ref = KR.kmedoids(Dq, eD, k, seed=2)
        assert_same(ctx.kmedoids(k, seed=2), ref)
        assert scan["totalcost"][k - 1] == ref["totalcost"]
    ctx.close()


def test_from_points_context():
    data = rc.generatemixture(900, 12, seed=6, points_only=True)
    ctx = rc.Context.from_points(data["points"])
    Dq, eD = KR.device_matrix(ctx)
    for k in (1, 4, 12, 100):
        assert_same(ctx.kmedoids(k, seed=9), KR.kmedoids(Dq, eD, k, seed=9))
    ctx.close()


def test_result_does_not_depend_on_a_state():
    D, truth = paper(2)
    a = rc.Context(D)
    r0 = [a.kmedoids(k, seed=5) for k in (1, 3, 7)]
    s0 = a.kmedoids_scan(1, 20, seed=5)
    b = rc.Context(D)
    b.set_params(**rc.likelihood_hyperparams(D, truth))
    b.set_state(truth)
    b.gibbs_sweep(1.0, 0.5, 3, 0)
    for k, r in zip((1, 3, 7), r0):
        assert_same(b.kmedoids(k, seed=5), dict(medoids=r.medoids, assignments=r.assignments, iterations=r.iterations,
                                                 converged=r.converged, totalcost=r.totalcost))
    s1 = b.kmedoids_scan(1, 20, seed=5)
    for key in s0:
        assert np.array_equal(s0[key], s1[key])
    a.close(); b.close()


def test_module_function_on_a_matrix():
    D, _ = paper(1)
    ctx = rc.Context(D)
    assert_same(rc.kmedoids(D, 4, seed=3), dict(vars(ctx.kmedoids(4, seed=3))))
    ctx.close()


def test_chain_unchanged_by_a_kmedoids_call():
    """Sweeps, a kmedoids call in the middle, more sweeps: labels, loglik and co-clustering counts equal a chain without it."""
    D, truth = paper(3)
    P = rc.likelihood_hyperparams(D, truth)
    init = np.random.default_rng(1).integers(1, 9, 100).astype(np.int64)
    out = []
    for call in (False, True):
        ctx = rc.Context(D)
        ctx.set_params(**P)
        ctx.set_state(init)
        ctx.cocluster_reset()
        for t in range(6):
            if call and t == 3:
                ctx.kmedoids(10, seed=1)
                ctx.kmedoids_scan(1, 30, seed=2)
            ctx.gibbs_sweep(1.2, 0.4, 77, t)
            ctx.record_sample(False)
        out.append((ctx.get_state()[0], ctx.loglik(), ctx.cocluster_counts(), ctx.layout_info()))
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and out[0][3] == out[1][3]


def test_nonzero_diagonal_empty_group_is_a_domain_error():
    """A point farther from itself than from another medoid leaves its group empty: RC_ERR_DOMAIN, not undefined behaviour."""
    x = np.array([0.0, 1.0, 3.0, 10.0])   # nearest other point: 0->1, 1->0, 2->1, 3->2; nobody picks point 3
    D = np.abs(x[:, None] - x[None, :])
    np.fill_diagonal(D, 100.0)
    ctx = rc.Context(D)
    with pytest.raises(rc.RedClustDomainError):
        ctx.kmedoids(4, seed=0)
    ctx.close()


def test_argument_errors():
    D, _ = paper(1)
    ctx = rc.Context(D)
    for k in (0, 101):
        with pytest.raises(rc.RedClustHIPError):
            ctx.kmedoids(k)
    with pytest.raises(rc.RedClustHIPError):
        ctx.kmedoids_scan(5, 4)
    ctx.close()


def test_chunked_scan_equals_single_runs_at_n8192():
    """At n = 8192 the scan over k = 1..4096 does not fit one workspace chunk (512 MiB: 2184 k values, 4096..1913, then
    1912..1): the entries on both sides of the chunk boundary, and at the ends, equal the single runs."""
    data = rc.generatemixture(8192, 20, seed=0)
    ctx = rc.Context(data["distancematrix"])
    scan = ctx.kmedoids_scan(1, 4096, maxiter=1000, seed=3)
    for k in (1, 2, 1912, 1913, 1914, 4096):
        r = ctx.kmedoids(k, maxiter=1000, seed=3)
        assert scan["totalcost"][k - 1] == r.totalcost and scan["iterations"][k - 1] == r.iterations, k
        assert bool(scan["converged"][k - 1]) == r.converged, k
    ctx.close()
