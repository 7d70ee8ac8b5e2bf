"""Metrics from coordinates without a device: the restatement of tests/metric_ref.py against exact rational arithmetic, its
exact symmetry and its behaviour under powers of two, the public surface (exports, keyword-only `metric`, header / SIGNATURES
/ Julia agreement) and the argument errors that come before the library is touched."""
import ctypes as C
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import metric_ref as M
import predict_points_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(7, 1, 3), (9, 5, 4), (5, 33, 3), (3, 200, 2)]          # the shapes of the Euclidean restatement's own test


# ---------------------------------------------------------------------------------------------------------------
# the restatement against exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cityblock", "chebyshev"])
def test_restated_distance_is_close_to_the_exact_one(metric, shape):
    """b = (dim + 4)·2^-53, the bound of tests/test_predict_points_cpu.py.  euclidean: as there, sq·(1 − b)² <= d² <= sq·(1 + b)².
    sqeuclidean: d is that chain before the root, so the same inequality holds for d in place of d².  cityblock: a
    subtraction's rounding enters its term once and each of the dim additions rounds a partial sum of non-negative terms once:
    (dim + 1)·2^-53 of the sum to first order — the bound already grows with dim and covers it.  chebyshev: rounding is
    monotone, so the largest rounded |t| is the rounded largest |t|: d equals the correctly rounded exact value."""
    n, dim, q = shape
    X, Y = PR.coordinates(n, dim, q)
    b = Fraction(dim + 4, 2 ** 53)
    worst = 0.0
    for y in Y:
        for x in X:
            d = Fraction(M.distance(metric, y, x))
            diffs = [abs(Fraction(float(a)) - Fraction(float(c))) for a, c in zip(y, x)]
            if metric == "euclidean":
                sq = sum(t * t for t in diffs)
                assert sq * (1 - b) ** 2 <= d * d <= sq * (1 + b) ** 2
                worst = max(worst, abs(float(d * d / sq) - 1.0) / 2)
            elif metric == "sqeuclidean":
                sq = sum(t * t for t in diffs)
                assert sq * (1 - b) ** 2 <= d <= sq * (1 + b) ** 2
                worst = max(worst, abs(float(d / sq) - 1.0))
            elif metric == "cityblock":
                exact = sum(diffs)
                assert exact * (1 - b) <= d <= exact * (1 + b)
                worst = max(worst, abs(float(d / exact) - 1.0))
            else:
                assert d == Fraction(float(max(diffs)))
    print(metric, "largest relative error / 2^-53 ~", worst * 2.0 ** 53, "bound:", dim + 4)


@pytest.mark.parametrize("metric", M.METRICS)
def test_every_metric_is_symmetric_bit_for_bit(metric):
    X, Y = PR.coordinates(9, 5, 4)
    assert np.array_equal(M.distances(metric, Y, X).view(np.uint64), M.distances(metric, X, Y).T.copy().view(np.uint64))
    X, Y = PR.coordinates(5, 33, 3)
    assert np.array_equal(M.distances(metric, Y, X).view(np.uint64), M.distances(metric, X, Y).T.copy().view(np.uint64))


@pytest.mark.parametrize("e", [100, -100])
@pytest.mark.parametrize("metric", M.METRICS)
def test_scaling_both_point_sets_by_a_power_of_two(metric, e):
    """euclidean, cityblock and chebyshev scale exactly; sqeuclidean by the square (2^±50 there); cosine and correlation do
    not change a bit"""
    X, Y = PR.coordinates(6, 5, 4)
    D = M.distances(metric, Y, X)
    if metric == "sqeuclidean":
        s = math.ldexp(1.0, e // 2)
        assert np.array_equal(M.distances(metric, Y * s, X * s), D * (s * s))
    elif metric in M.ANGULAR:
        s = math.ldexp(1.0, e)
        assert np.array_equal(M.distances(metric, Y * s, X * s).view(np.uint64), D.view(np.uint64))
    else:
        s = math.ldexp(1.0, e)
        assert np.array_equal(M.distances(metric, Y * s, X * s), D * s)


def test_the_value_tests_stay_inside_the_domain():
    """every reference distance of the GPU tests' shapes is positive: one metric of each family at the shape the smallest
    values come from; all of them are checked where they are used (tests/test_gpu_metrics.py)"""
    for metric in ("cityblock", "chebyshev", "cosine"):
        _, _, D = M.case(metric, 257, 3, 9)
        print(metric, "smallest reference distance at (257, 3, 9):", D.min())
        assert D.min() > 0


# ---------------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------------
def test_the_new_names_are_exported():
    assert callable(rc.pairwise) and callable(_lib.pairwise)
    assert list(rc.METRICS) == list(M.METRICS) and list(rc.METRICS.values()) == list(range(6))
    sig = inspect.signature(rc.pairwise)
    assert list(sig.parameters)[:2] == ["points", "new_points"]
    assert sig.parameters["metric"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["metric"].default == "euclidean"
    assert sig.parameters["device"].kind is inspect.Parameter.KEYWORD_ONLY
    for f in (rc.predict_points, rc.predict, rc.predict_joint, _lib.predict_points):
        assert inspect.signature(f).parameters["metric"].kind is inspect.Parameter.KEYWORD_ONLY, f
    assert inspect.signature(rc.predict_points).parameters["metric"].default == "euclidean"
    assert inspect.signature(_lib.Context.from_points).parameters["metric"].default is None
    assert inspect.signature(rc.MCMCData.__init__).parameters["metric"].default is None


def test_header_signatures_and_julia_agree_on_the_three_entry_points():
    import test_oracle_cpu as T
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    for k, name in enumerate(M.METRICS):
        assert f"#define RC_METRIC_{name.upper()} {k}\n" in hdr
    protos = T._header_prototypes(hdr)
    pp = protos["rc_predict_points"]
    want = {"rc_pairwise": ("int32_t", ["int32_t", "int32_t", "int64_t", "int64_t", "double*", "int64_t", "double*", "double*", "double*"]),
            "rc_create_from_points_metric": ("int32_t", ["int64_t", "int64_t", "double*", "int32_t", "int32_t", "int32_t", "int64_t", "rc_ctx**"]),
            "rc_predict_points_metric": (pp[0], ["int32_t"] + pp[1])}     # the metric, then rc_predict_points' arguments
    assert protos["rc_create_from_points"] == ("int32_t", ["int64_t", "int64_t", "double*", "int32_t", "int32_t", "int64_t", "rc_ctx**"])
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    calls = T._julia_ccalls(jl)
    for name, (ret, args) in want.items():
        assert protos[name] == (ret, args), name
        res, sig = rc.SIGNATURES[name]
        assert res is C.c_int32 and len(sig) == len(args), name
        for k, (ct, py) in enumerate(zip(args, sig)):
            if ct in scalars:
                assert py is scalars[ct], (name, k, ct, py)
            else:
                assert py in (C.c_void_p, C.POINTER(_lib.RcParams), C.POINTER(C.c_double), C.POINTER(C.c_void_p)), (name, k, ct, py)
        mine = [c for c in calls if c[0] == name]
        assert mine, f"{name} is not called from julia/RedClustHIP.jl"
        for _, jret, jargs, npassed in mine:
            assert jret == "Int32" and len(jargs) == npassed == len(args), name
            for jt, ct in zip(jargs, args):
                assert ct in T._JL2C[jt], (name, jt, ct)
    assert rc.SIGNATURES["rc_predict_points_metric"][1][1:] == rc.SIGNATURES["rc_predict_points"][1]
    assert "function pairwise(b::HIPBackend, points::Matrix{Float64}" in jl and "metric = :euclidean" in jl
    T.test_julia_glue_ccalls_match_the_header()


def test_the_sources_are_part_of_the_build():
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    tu = open(os.path.join(csrc, "redclust_hip.hip")).read()
    for name in ("metric.inc.hip", "pairwise.inc.hip"):
        assert f'#include "{name}"' in tu
        assert os.path.join(csrc, name) in _lib._sources()           # build() watches it
    assert tu.index('#include "metric.inc.hip"') < tu.index('#include "predictpoints.inc.hip"') < tu.index('#include "pairwise.inc.hip"')


# ---------------------------------------------------------------------------------------------------------------
# argument errors before the library
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "pairwise", touched)
    monkeypatch.setattr(_lib, "predict_points", touched)


def _inputs():
    S = np.array([[1, 1, 2, 2], [1, 2, 3, 3]], np.int64)
    X = np.arange(8.0).reshape(4, 2) ** 2
    Y = np.array([[0.5, 0.25], [9.0, 1.0], [2.0, 2.5]])
    kw = dict(r=np.array([1.0, 2.0]), p=np.array([0.5, 0.25]), params=PR.PR.PARAMS)
    return S, X, Y, kw


CALLS = {
    "pairwise": lambda S, X, Y, kw, metric: rc.pairwise(X, Y, metric=metric),
    "pairwise_self": lambda S, X, Y, kw, metric: rc.pairwise(X, metric=metric),
    "MCMCData": lambda S, X, Y, kw, metric: rc.MCMCData(X, metric=metric),
    "from_points": lambda S, X, Y, kw, metric: rc.Context.from_points(X, metric=metric),
    "predict_points": lambda S, X, Y, kw, metric: rc.predict_points(S, X, Y, metric=metric, **kw),
    "lib_predict_points": lambda S, X, Y, kw, metric: _lib_predict_points(X, Y, S, kw["r"], kw["p"], kw["params"], metric=metric),
    "predict": lambda S, X, Y, kw, metric: rc.predict(S, new_points=Y, points=X, metric=metric, **kw),
    "predict_joint": lambda S, X, Y, kw, metric: rc.predict_joint(S, new_points=Y, points=X, metric=metric, **kw),
}
_lib_predict_points = _lib.predict_points                             # the binding itself, taken before the fixture replaces the name


@pytest.mark.parametrize("call", list(CALLS))
def test_an_unknown_metric_is_refused_before_the_library(call, no_library):
    S, X, Y, kw = _inputs()
    for bad in ("minkowski", "Euclidean", 2, ""):
        with pytest.raises(ValueError, match="metric"):
            CALLS[call](S, X, Y, kw, bad)


@pytest.mark.parametrize("call", list(CALLS))
def test_correlation_in_one_dimension_is_refused_before_the_library(call, no_library):
    S, X, Y, kw = _inputs()
    with pytest.raises(ValueError, match="correlation"):
        CALLS[call](S, X[:, :1], Y[:, :1], kw, "correlation")


def test_a_metric_with_a_square_matrix_is_refused(no_library):
    D = np.array([[0.0, 1.0], [1.0, 0.0]])
    with pytest.raises(ValueError, match="metric"):
        rc.MCMCData(D, metric="cityblock")
    assert rc.MCMCData(D).metric is None


# ---------------------------------------------------------------------------------------------------------------
# defaults
# ---------------------------------------------------------------------------------------------------------------
def test_mcmcdata_keeps_its_metric_and_evaluates_it_on_the_host(no_library):
    _, X, _, _ = _inputs()
    assert rc.MCMCData(X).metric is None
    X, _, _ = M.case("cityblock", 65, 17, 65)
    data = rc.MCMCData(X, metric="cityblock")
    assert data.metric == "cityblock" and data.n == 65
    ref = M.distances("cityblock", X, X)
    D = data.D
    assert D.shape == (65, 65) and np.array_equal(D, D.T) and not D.diagonal().any()
    off = ~np.eye(65, dtype=bool)
    # both sum 17 rounded terms; either is within (dim + 1)·2^-53 of the exact sum (above), so within (dim + 4)·2^-52 of the other
    assert np.all(np.abs(D[off] - ref[off]) <= (17 + 4) * 2.0 ** -52 * ref[off])
    assert np.array_equal(data.logD[off], np.log(D[off]))
    for metric in M.METRICS:                                        # every name evaluates, to the restatement within rounding
        H = rc.MCMCData(X[:9], metric=metric).D
        R = M.distances(metric, X[:9], X[:9])
        o = ~np.eye(9, dtype=bool)
        assert np.allclose(H[o], R[o], rtol=1e-9, atol=0), metric
