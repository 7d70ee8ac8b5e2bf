"""GPU k-means (csrc/kmeans.inc.hip through rc_kmeans / rc_kmeans_scan) against the NumPy restatement
(tests/kmeans_ref.py): every field bit for bit — centres, assignments, costs, counts, total cost, iteration count and
convergence flag — for single runs over a sampled cross product of shapes, an init-given run, the repicking of an empty
group, the batched scan with and without forced chunk boundaries, and the context's chain state left untouched."""
import os

import numpy as np
import pytest

import kmeans_ref as KM
import redclust_amd as rc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (7, (1 << 32) + 12345678901)

HAND = np.array([[2, 8], [1, 2], [1, 8], [6, 6], [3, 8], [1, 4], [2, 4], [3, 9], [5, 0]], dtype=np.float64)
HAND_INIT = [1, 3, 4, 5]

# (n, dim, k): n in {1, 2, 63, 64, 65, 257, 1000}, dim in {1, 2, 3, 17, 50}, k in {1, 2, 3, n // 2, n}, sampled; and dim = 70,
# beyond the 64 coordinates the assignment kernel keeps in registers (its other path)
SHAPES = [(1, 1, 1), (1, 3, 1), (2, 2, 1), (2, 2, 2), (2, 50, 2),
          (63, 17, 1), (63, 17, 3), (63, 1, 31), (63, 17, 63),
          (64, 1, 2), (64, 3, 32), (64, 2, 64),
          (65, 50, 2), (65, 50, 3), (65, 3, 32), (65, 50, 65), (65, 70, 3), (65, 70, 32),
          (257, 3, 1), (257, 2, 2), (257, 17, 3), (257, 3, 128), (257, 50, 257),
          (1000, 50, 3), (1000, 1, 2), (1000, 17, 500), (1000, 50, 500), (1000, 3, 1000)]

_points = {}


def points(n, dim):
    if (n, dim) not in _points:
        pts = rc.generatemixture(n, min(dim, 5, n), dim=dim, seed=n + dim, sigma=0.25, points_only=True)["points"]
        pts.setflags(write=False)
        _points[(n, dim)] = pts
    return _points[(n, dim)]


def assert_same(res, ref):
    assert np.array_equal(res.assignments, ref["assignments"])
    assert np.array_equal(res.counts, ref["counts"])
    assert res.iterations == ref["iterations"] and res.converged == ref["converged"]
    assert np.array_equal(res.centers, ref["centers"])
    assert np.array_equal(res.costs, ref["costs"])
    assert res.totalcost == ref["totalcost"]


@pytest.mark.parametrize("n,dim,k", SHAPES)
def test_single_run_equals_restatement(n, dim, k):
    X = points(n, dim)
    seed = SEEDS[(n + dim + k) % 2]
    ctx = rc.Context.from_points(X)
    try:
        assert_same(ctx.kmeans(k, seed=seed), KM.kmeans(X, k, seed=seed))
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_both_seeds_and_maxiter_rules(seed):
    X = points(257, 17)
    ctx = rc.Context.from_points(X)
    for k, maxiter in ((5, 100), (5, 0), (5, 2), (1, 100), (40, 1000)):
        assert_same(ctx.kmeans(k, maxiter=maxiter, seed=seed), KM.kmeans(X, k, maxiter=maxiter, seed=seed))
    r = ctx.kmeans(1, seed=seed)
    assert r.iterations == 1 and r.converged
    r = ctx.kmeans(5, maxiter=0, seed=seed)
    assert r.iterations == 0 and not r.converged
    ctx.close()


def test_empty_group_is_repicked_on_the_device():
    ref = KM.kmeans(HAND, 4, init=HAND_INIT, seed=3)
    assert ref["repicks"] >= 1
    ctx = rc.Context.from_points(HAND)
    res = ctx.kmeans(4, init=HAND_INIT, seed=3)
    ctx.close()
    assert_same(res, ref)
    assert np.all(res.counts > 0)


def test_init_given_run_equals_restatement():
    X = points(257, 3)
    init = np.random.default_rng(5).permutation(257)[:9] + 1
    ctx = rc.Context.from_points(X)
    assert_same(ctx.kmeans(9, init=init, seed=1), KM.kmeans(X, 9, init=init, seed=1))
    assert_same(rc.kmeans(X, 9, init=init), dict(vars(ctx.kmeans(9, init=init)), repicks=0))   # the module function
    ctx.close()


@pytest.mark.parametrize("slots_per_chunk", [0, 7])
def test_scan_entries_equal_single_runs(slots_per_chunk):
    """Every entry of a batched scan (largest k first, converged runs dropping out, chunk boundaries inside the scan)
    equals the single run."""
    X = rc.generatemixture(300, 5, dim=5, seed=4, sigma=0.3, points_only=True)["points"]
    ctx = rc.Context.from_points(X)
    scan = ctx.kmeans_scan(1, 150, seed=11, slots_per_chunk=slots_per_chunk)
    for k in range(1, 151):
        r = ctx.kmeans(k, seed=11)
        assert scan["totalcost"][k - 1] == r.totalcost and scan["iterations"][k - 1] == r.iterations, k
        assert bool(scan["converged"][k - 1]) == r.converged, k
    assert np.any(scan["iterations"] != scan["iterations"][0])   # runs of different lengths were batched together
    for k in (1, 2, 77, 150):   # and the single runs are the restatement's
        assert scan["totalcost"][k - 1] == KM.kmeans(X, k, seed=11)["totalcost"], k
    ctx.close()


def test_result_does_not_depend_on_a_state():
    data = rc.generatemixture(200, 4, dim=4, seed=2)
    X, truth = data["points"], np.asarray(data["clusts"], dtype=np.int64)
    a = rc.Context.from_points(X)
    r0 = [a.kmeans(k, seed=5) for k in (1, 3, 7)]
    s0 = a.kmeans_scan(1, 20, seed=5)
    b = rc.Context.from_points(X)
    b.set_params(**rc.likelihood_hyperparams(data["distancematrix"], truth))
    b.set_state(truth)
    b.gibbs_sweep(1.0, 0.5, 3, 0)
    for k, r in zip((1, 3, 7), r0):
        assert_same(b.kmeans(k, seed=5), vars(r))
    s1 = b.kmeans_scan(1, 20, seed=5)
    for key in s0:
        assert np.array_equal(s0[key], s1[key])
    a.close(); b.close()


def test_chain_unchanged_by_a_kmeans_call():
    """Sweeps, kmeans calls in the middle, more sweeps: labels, loglik and co-clustering counts equal a chain without them."""
    data = rc.generatemixture(100, 4, dim=4, seed=6)
    X, truth = data["points"], np.asarray(data["clusts"], dtype=np.int64)
    P = rc.likelihood_hyperparams(data["distancematrix"], truth)
    init = np.random.default_rng(1).integers(1, 9, 100).astype(np.int64)
    out = []
    for call in (False, True):
        ctx = rc.Context.from_points(X)
        ctx.set_params(**P)
        ctx.set_state(init)
        ctx.cocluster_reset()
        for t in range(6):
            if call and t == 3:
                ctx.kmeans(10, seed=1)
                ctx.kmeans_scan(1, 30, seed=2)
                ctx.kmeans_scan(1, 30, seed=2, split=True)
            ctx.gibbs_sweep(1.2, 0.4, 77, t)
            ctx.record_sample(False)
        out.append((ctx.get_state()[0], ctx.loglik(), ctx.cocluster_counts(), ctx.layout_info()))
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and out[0][3] == out[1][3]


def test_argument_and_state_errors():
    X = points(63, 17)
    ctx = rc.Context.from_points(X)
    bad_calls = [lambda: ctx.kmeans(0), lambda: ctx.kmeans(64), lambda: ctx.kmeans_scan(5, 4), lambda: ctx.kmeans_scan(0, 4),
                 lambda: ctx.kmeans(3, maxiter=-1), lambda: ctx.kmeans(3, maxiter=(1 << 24) + 1), lambda: ctx.kmeans(3, tol=-1.0),
                 lambda: ctx.kmeans(3, tol=float("nan"))]
    for call in bad_calls:
        with pytest.raises(rc.RedClustHIPError) as e:
            call()
        assert e.value.code == -4   # RC_ERR_DOMAIN
    for bad in ([1, 2, 64], [0, 2, 3], [4, 9, 4]):
        with pytest.raises(rc.RedClustHIPError) as e:
            ctx.kmeans(3, init=bad)
        assert e.value.code == -1   # RC_ERR_ARG
    assert_same(ctx.kmeans(3, seed=1), KM.kmeans(X, 3, seed=1))   # the context is still good
    ctx.close()
    D = np.load(os.path.join(HERE, "golden", "paper_datasets.npz"))["D1"]
    ctx = rc.Context(D)   # from a matrix: no observations to cluster
    for call in (lambda: ctx.kmeans(3), lambda: ctx.kmeans_scan(1, 5), lambda: ctx.kmeans_scan(1, 5, split=True)):
        with pytest.raises(rc.RedClustHIPError) as e:
            call()
        assert e.value.code == -5   # RC_ERR_STATE
    ctx.close()


def test_duplicate_points_are_a_domain_error():
    """Exact duplicates never reach k-means: a context refuses zero distances.  Points that coincide to within 2^-29 of the
    bounding box have squared distances whose integer weights are all zero — the draw Clustering.jl's wsample fails on."""
    with pytest.raises(rc.RedClustDomainError):
        rc.Context.from_points(np.ones((4, 2)))
    with pytest.raises(ValueError):
        KM.kmeans(np.ones((4, 2)), 2)
    Y = np.array([[0.0, 0.0], [1e-10, 0.0], [0.0, 1e-10], [1.0, 0.0]])   # three near-duplicates and one far point
    ctx = rc.Context.from_points(Y)
    for seed in SEEDS:
        with pytest.raises(ValueError):
            KM.kmeans(Y, 3, seed=seed)
        with pytest.raises(rc.RedClustDomainError):
            ctx.kmeans(3, seed=seed)
        with pytest.raises(rc.RedClustDomainError):
            ctx.kmeans_scan(1, 4, seed=seed)
        assert_same(ctx.kmeans(2, seed=seed), KM.kmeans(Y, 2, seed=seed))   # two distinct locations: fine
    ctx.close()
