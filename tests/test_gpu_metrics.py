"""Metrics from coordinates on the GPU (csrc/metric.inc.hip, predictpoints.inc.hip, pairwise.inc.hip): both kernels bit for bit
against the restatement of tests/metric_ref.py and against each other, predict_points in a metric against rc_predict on its own
distances, contexts made from points in a metric against contexts made from rc.pairwise's matrix, a chain end to end, the
errors (found through the flag word or the host checks, never by a fault) and the chunking."""
import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import metric_ref as M
import predict_points_ref as R

pytestmark = pytest.mark.gpu

CASES = [(metric, shape) for metric in M.METRICS for shape in M.shapes(metric)]
IDS = [f"{metric}-{'x'.join(map(str, shape))}" for metric, shape in CASES]


def _differing(a, b):
    return np.flatnonzero(np.ascontiguousarray(a).view(np.uint64).ravel() != np.ascontiguousarray(b).view(np.uint64).ravel())


# ---------------------------------------------------------------------------------------------------------------
# the two kernels, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,shape", CASES, ids=IDS)
def test_new_against_training_points_equals_the_restatement(metric, shape):
    X, Y, ref = M.case(metric, *shape)
    assert ref.min() > 0                                            # the value test stays inside the domain
    D = rc.pairwise(X, Y, metric=metric)
    assert D.shape == ref.shape and D.dtype == np.float64
    bad = _differing(D, ref)
    print("distances that differ:", len(bad), "of", ref.size, "smallest reference distance:", ref.min())
    assert len(bad) == 0, (bad[:5], D.ravel()[bad[:5]], ref.ravel()[bad[:5]])


@pytest.mark.parametrize("metric,shape", CASES, ids=IDS)
def test_the_symmetric_matrix_equals_the_restatement_and_the_other_kernel(metric, shape):
    X, ref = M.self_case(metric, *shape)
    n = len(X)
    off = ~np.eye(n, dtype=bool)
    D = rc.pairwise(X, metric=metric)
    assert D.shape == (n, n)
    assert np.array_equal(D.view(np.uint64), D.T.copy().view(np.uint64)) and not D.diagonal().any()
    bad = _differing(D[off], ref[off])
    print("entries that differ from the restatement:", len(bad), "of", int(off.sum()))
    assert len(bad) == 0, (bad[:5], D[off][bad[:5]], ref[off][bad[:5]])
    other = _differing(D[off], rc.pairwise(X, X, metric=metric)[off])
    print("entries that differ between the two kernels:", len(other))
    assert len(other) == 0


# ---------------------------------------------------------------------------------------------------------------
# predict_points in a metric
# ---------------------------------------------------------------------------------------------------------------
ONE = dict(r=np.array([1.0]), p=np.array([0.5]), params=R.PR.PARAMS)


@pytest.mark.parametrize("metric", M.METRICS)
def test_predict_points_returns_the_distances_of_pairwise(metric):
    X, Y, ref = M.case(metric, 65, 17, 65)
    out = _lib.predict_points(X, Y, np.ones((1, 65), np.int64), ONE["r"], ONE["p"], ONE["params"], want_dist=True, metric=metric)
    assert len(_differing(out["dist"], rc.pairwise(X, Y, metric=metric))) == 0
    assert len(_differing(out["dist"], ref)) == 0


def _points(c, **kw):
    args = dict(seed=c["seed"], sample_offset=c["sample_offset"], point_offset=c["point_offset"], Kmax=c["Kmax"], want_scores=True,
                want_sums=True, want_dist=True, want_log=True)
    args.update(kw)
    return _lib.predict_points(c["X"], c["Y"], c["samples"], c["r"], c["p"], c["P"], **args)


KEYS = ("labels", "map", "sums", "eD", "eL", "dist", "log")


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["scores"].view(np.uint64), b["scores"].view(np.uint64))


def test_the_euclidean_name_is_the_call_without_a_metric():
    c = R.predict_case()
    _same(_points(c), _points(c, metric="euclidean"))


@pytest.mark.parametrize("metric", ["cityblock", "cosine"])
def test_equals_rc_predict_on_its_distances_and_logs(metric):
    c = R.predict_case()
    out = _points(c, metric=metric)
    assert out["kernel_ms"] > 0
    assert len(_differing(out["dist"][:3], M.distances(metric, c["Y"][:3], c["X"]))) == 0
    ref = _lib.predict(out["dist"], c["samples"], c["r"], c["p"], c["P"], seed=c["seed"], sample_offset=c["sample_offset"],
                       point_offset=c["point_offset"], logDnew=out["log"], Kmax=c["Kmax"], want_scores=True, want_sums=True)
    for k in ("labels", "map", "sums", "eD", "eL"):
        assert np.array_equal(out[k], ref[k]), k
    assert np.array_equal(out["scores"].view(np.uint64), ref["scores"].view(np.uint64))
    assert (out["labels"] > 0).any()


def test_the_public_predict_points_takes_the_metric():
    c = R.predict_case()
    kw = dict(r=c["r"], p=c["p"], params=c["P"], seed=c["seed"])
    plain = _points(c, metric="chebyshev", sample_offset=0, point_offset=0)
    pred = rc.predict_points(c["samples"], c["X"], c["Y"], metric="chebyshev", **kw)
    assert np.array_equal(pred.labels, plain["labels"]) and np.array_equal(pred.map_labels, plain["map"])
    assert not np.array_equal(pred.labels, rc.predict_points(c["samples"], c["X"], c["Y"], **kw).labels)     # the metric matters


def test_chunks_of_samples_and_points_give_the_same_bits(monkeypatch):
    """RC_PREDICT_WORKSPACE_KIB is read per call, so it is set here as tests/test_gpu_predict_points.py sets it (64 KiB: one
    sample and about eight new points per launch); rc_pairwise's rows go through the same cap"""
    c = R.predict_case()
    whole = _points(c, metric="chebyshev")
    D = rc.pairwise(c["X"], c["Y"], metric="chebyshev")
    monkeypatch.setenv("RC_PREDICT_WORKSPACE_KIB", "64")
    _same(whole, _points(c, metric="chebyshev"))
    assert len(_differing(D, rc.pairwise(c["X"], c["Y"], metric="chebyshev"))) == 0
    assert len(_differing(D, whole["dist"])) == 0


# ---------------------------------------------------------------------------------------------------------------
# contexts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("shape", [(65, 17, 65), (129, 33, 3)], ids=["65x17", "129x33"])
@pytest.mark.parametrize("metric", M.METRICS)
def test_a_context_from_points_holds_the_matrix_of_pairwise(metric, shape, bits):
    X, _ = M.self_case(metric, *shape)
    a = rc.Context.from_points(X, metric=metric, storage_bits=bits)
    b = rc.Context(rc.pairwise(X, metric=metric), storage_bits=bits)
    try:
        assert a.metric == metric and a.dim == shape[1]
        for which in (0, 1):
            assert len(_differing(a.get_matrix(which), b.get_matrix(which))) == 0, which
    finally:
        a.close(); b.close()


def test_a_context_from_points_without_a_metric_is_what_it_was():
    """the tolerance of tests/test_gpu_parity.py::test_device_pairwise_distances — 1e-12 of the largest distance — which holds
    the device's matrix and MCMCData(points).D to the same oracle there"""
    X, _ = M.self_case("euclidean", 65, 17, 65)
    a = rc.Context.from_points(X)
    b = rc.Context(rc.MCMCData(X).D)
    try:
        assert a.metric is None
        Da, Db = a.get_matrix(0), b.get_matrix(0)
    finally:
        a.close(); b.close()
    print("largest difference / largest distance:", float(np.max(np.abs(Da - Db)) / Db.max()))
    assert np.array_equal(Da, Da.T) and not Da.diagonal().any()
    assert np.max(np.abs(Da - Db)) <= 1e-12 * Db.max()


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
def test_a_chain_from_points_in_a_metric_is_the_chain_on_its_matrix():
    rng = np.random.default_rng(64)
    X = np.concatenate([rng.standard_normal((32, 5)), 20.0 + rng.standard_normal((32, 5))])
    D = rc.pairwise(X, metric="cityblock")
    truth = np.repeat([1, 2], 32)
    P = rc.likelihood_hyperparams(D, truth)
    params = rc.PriorHyperparamsList(**{k: P[k] for k in ("delta1", "delta2", "alpha", "beta", "zeta", "gamma")})
    options = rc.MCMCOptionsList(numiters=50)
    init = rc.MCMCState(np.arange(64) % 4 + 1, 1.0, 0.5)
    a = rc.runsampler(rc.MCMCData(X, metric="cityblock"), options, params, init, verbose=False, seed=5, engine="native")
    b = rc.runsampler(rc.MCMCData(D), options, params, init, verbose=False, seed=5, engine="native")
    assert len(a.clusts) == len(b.clusts) == options.numsamples > 0
    for s, (u, v) in enumerate(zip(a.clusts, b.clusts)):
        assert np.array_equal(u, v), s
    assert np.array_equal(a.r, b.r) and np.array_equal(a.K, b.K)


# ---------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", M.METRICS)
def test_a_new_point_on_a_training_point_is_named_with_the_metric(metric):
    c = R.predict_case()
    Y = c["Y"].copy()
    Y[41], Y[60] = c["X"][150], c["X"][3]                           # the first in row-major order is (42, 151)
    with pytest.raises(rc.RedClustDomainError, match=r"new point 42 coincides with training point 151 \(metric " + metric + r"\)"):
        _lib.predict_points(c["X"], Y, c["samples"], c["r"], c["p"], c["P"], metric=metric)
    D = rc.pairwise(c["X"], Y, metric=metric)                       # the raw distances are handed out without complaint
    assert D.shape == (c["q"], c["n"]) and np.all(D[[41, 60], [150, 3]] <= (2.0 ** -51 if metric in M.ANGULAR else 0.0))
    assert np.all(np.delete(D.ravel(), [41 * c["n"] + 150, 60 * c["n"] + 3]) > 2.0 ** -51)


def test_parallel_points_are_a_domain_error_under_cosine():
    c = R.predict_case()
    Y = c["Y"].copy()
    Y[7] = 4.0 * c["X"][20]                                         # a power of two: the same chain, scaled exactly
    with pytest.raises(rc.RedClustDomainError, match=r"new point 8 is parallel to training point 21: their cosine distance"):
        _lib.predict_points(c["X"], Y, c["samples"], c["r"], c["p"], c["P"], metric="cosine")
    _lib.predict_points(c["X"], Y, c["samples"], c["r"], c["p"], c["P"], metric="cityblock")     # distinct points otherwise


def test_a_zero_or_constant_vector_is_a_domain_error_that_says_so():
    c = R.predict_case()
    Y = c["Y"].copy()
    Y[5] = 0.0
    with pytest.raises(rc.RedClustDomainError, match=r"new point 6 is the zero vector: its cosine distance is undefined"):
        _lib.predict_points(c["X"], Y, c["samples"], c["r"], c["p"], c["P"], metric="cosine")
    Y[5] = 2.0                                                      # 5·2 / 5 = 2 exactly: the centred vector is zero
    with pytest.raises(rc.RedClustDomainError, match=r"new point 6 has constant coordinates: its correlation distance is undefined"):
        _lib.predict_points(c["X"], Y, c["samples"], c["r"], c["p"], c["P"], metric="correlation")
    X = c["X"].copy()
    X[9] = 0.0
    with pytest.raises(rc.RedClustDomainError, match=r"training point 10 is the zero vector"):
        _lib.predict_points(X, c["Y"], c["samples"], c["r"], c["p"], c["P"], metric="cosine")
    D = rc.pairwise(X, c["Y"], metric="cosine")                     # rc_pairwise hands out what the arithmetic gives
    assert D.shape == (c["q"], c["n"]) and np.all(np.delete(D, 9, axis=1) > 0)


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cityblock", "chebyshev", "cosine"])
def test_identical_training_points_are_refused_by_the_context_and_not_by_pairwise(metric):
    """under cosine the arithmetic gives an exact 0 for a point against itself only when norm·norm rounds back to the squared
    norm (include/redclust_hip.h); (3, 4, 0, 0, 0) has norm 5 exactly"""
    X = np.array(R.predict_case()["X"][:40])
    X[11] = X[30] = [3.0, 4.0, 0.0, 0.0, 0.0]
    with pytest.raises(rc.RedClustDomainError, match="off-diagonal entries of D must be positive"):
        rc.Context.from_points(X, metric=metric)
    D = rc.pairwise(X, metric=metric)
    assert D[11, 30] == 0.0 and D[30, 11] == 0.0 and np.count_nonzero(D == 0.0) == 40 + 2


def test_argument_errors_of_the_library():
    L = rc.lib()
    X = np.ascontiguousarray(R.predict_case()["X"][:8])
    out = np.zeros((8, 8))
    h = _lib.C.c_void_p()
    for metric, dim in ((6, 5), (-1, 5), (5, 1)):
        code = L.rc_pairwise(0, metric, 8, dim, X.ctypes.data, 0, None, out.ctypes.data, None)
        assert _lib.ERRORS.get(code, code) == "RC_ERR_ARG" and L.rc_last_error(None).decode().startswith("rc_pairwise"), (metric, dim)
        code = L.rc_create_from_points_metric(8, dim, X.ctypes.data, metric, 64, 0, 0, _lib.C.byref(h))
        assert _lib.ERRORS.get(code, code) == "RC_ERR_ARG" and L.rc_last_error(None).decode().startswith("rc_create_from_points_metric")
    for args in ((0, 0, 0, 5, X.ctypes.data, 0, None, out.ctypes.data, None), (0, 0, 8, 0, X.ctypes.data, 0, None, out.ctypes.data, None),
                 (0, 0, 8, 5, None, 0, None, out.ctypes.data, None), (0, 0, 8, 5, X.ctypes.data, 0, None, None, None),
                 (0, 0, 8, 5, X.ctypes.data, 0, X.ctypes.data, out.ctypes.data, None), (99, 0, 8, 5, X.ctypes.data, 0, None, out.ctypes.data, None)):
        code = L.rc_pairwise(*args)
        assert _lib.ERRORS.get(code, code) == "RC_ERR_ARG", args
    assert rc.pairwise(X, metric="correlation").shape == (8, 8)     # the device is as it was
