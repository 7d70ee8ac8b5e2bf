"""The restatement of rc_predict_points' distance (tests/predict_points_ref.py) against exact rational arithmetic, and the
argument checks of rc.predict_points that need no device."""
import math
from fractions import Fraction

import numpy as np
import pytest

import redclust_amd as rc
import predict_points_ref as R


@pytest.mark.parametrize("shape", [(7, 1, 3), (9, 5, 4), (5, 33, 3), (3, 200, 2)])
def test_restated_distance_is_close_to_the_exact_one(shape):
    """Relative error <= b = (dim + 4)·2^-53.  Each fma rounds a partial sum of non-negative terms once (dim roundings, each at
    most 2^-53 of the final sum); a subtraction's rounding enters its square twice (2·2^-53 of that term, so of the sum at
    most); the root halves the sum of these and adds one rounding: (dim + 4)·2^-54 to first order, doubled in the bound.
    Checked in rationals without a root: sq·(1 − b)² <= d² <= sq·(1 + b)²."""
    n, dim, q = shape
    X, Y = R.coordinates(n, dim, q)
    b = Fraction(dim + 4, 2 ** 53)
    worst = 0.0
    for y in Y:
        for x in X:
            d = Fraction(R.distance(y, x))
            sq = R.exact_distance_sq(y, x)
            worst = max(worst, abs(float(d * d / sq) - 1.0) / 2)    # the figure, to first order; the assertion is exact
            assert sq * (1 - b) ** 2 <= d * d <= sq * (1 + b) ** 2
    print("largest relative error / 2^-53 ~", worst * 2.0 ** 53, "bound:", dim + 4)


def test_fma_restatement_rounds_once():
    a = 1.0 + 2.0 ** -30
    assert R.fma(a, a, -1.0) == 2.0 ** -29 + 2.0 ** -60             # a·a − 1 exactly; a*a alone rounds the 2^-60 away
    assert a * a - 1.0 == 2.0 ** -29
    assert R.fma(3.0, 3.0, 0.0) == 9.0 and R.fma(0.0, 0.0, 0.0) == 0.0
    assert R.fma(2.0 ** 52 + 1, 2.0, 1.0) == 2.0 ** 53 + 4.0        # 2^53 + 3 is a tie between 2^53 + 2 and 2^53 + 4: to even


@pytest.mark.parametrize("e", [100, -100])
def test_scaling_by_a_power_of_two_scales_every_distance_exactly(e):
    X, Y = R.coordinates(6, 5, 4)
    D = R.distances(Y, X)
    s = math.ldexp(1.0, e)
    assert np.array_equal(R.distances(Y * s, X * s), D * s)


def test_the_restatement_sees_a_close_pair_that_the_expanded_form_loses():
    x = np.array([1e8, 1e8, 1e8])
    y = x + np.array([1e-3, 0.0, 0.0])
    d = R.distance(y, x)
    assert abs(d - (y[0] - x[0])) <= 2 * math.ulp(d) and d > 0
    e = y @ y + x @ x - 2 * (y @ x)                                 # |a|² + |b|² − 2a·b: cancels at 1e16
    assert not (0.5 * d * d <= e <= 2 * d * d)


# ---------------------------------------------------------------------------------------------------------------
# the public surface: exported, and its argument errors come before the library is touched
# ---------------------------------------------------------------------------------------------------------------
def _inputs():
    S = np.array([[1, 1, 2, 2], [1, 2, 3, 3]], np.int64)
    X = np.arange(8.0).reshape(4, 2)
    Y = np.array([[0.5, 0.25], [9.0, 1.0], [2.0, 2.5]])
    kw = dict(r=np.array([1.0, 2.0]), p=np.array([0.5, 0.25]), params=R.PR.PARAMS)
    return S, X, Y, kw


def test_predict_points_is_exported():
    assert callable(rc.predict_points)
    import inspect
    sig = inspect.signature(rc.predict_points)
    assert list(sig.parameters)[:3] == ["result_or_samples", "points", "new_points"]
    for name in ("relabelling", "keep_labels", "r", "p", "params", "seed", "scores", "device"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert "rc_predict_points" in rc.SIGNATURES
    P = rc.Prediction(np.zeros((1, 1), np.int64), np.zeros((1, 1), np.int64))
    assert P.counts is None and P.map_counts is None and P.pivot_labels is None and P.scores is None and P.kernel_ms == 0.0


@pytest.fixture
def no_library(monkeypatch):
    from redclust_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "predict_points", touched)


@pytest.mark.parametrize("case", ["points_rows", "points_1d", "new_dim", "new_1d", "new_empty", "dim0", "nan_new", "inf_points",
                                  "keep_false_alone", "scores_without_labels", "r_shape", "no_params"])
def test_argument_errors_come_before_the_library(case, no_library):
    S, X, Y, kw = _inputs()
    args = dict(kw)
    if case == "points_rows":
        X = X[:3]
    elif case == "points_1d":
        X = X[:, 0]
    elif case == "new_dim":
        Y = np.ones((3, 3))
    elif case == "new_1d":
        Y = Y[0]
    elif case == "new_empty":
        Y = np.zeros((0, 2))
    elif case == "dim0":
        X, Y = np.zeros((4, 0)), np.zeros((3, 0))
    elif case == "nan_new":
        Y = Y.copy(); Y[1, 1] = np.nan
    elif case == "inf_points":
        X = X.copy(); X[0, 0] = np.inf
    elif case == "keep_false_alone":
        args["keep_labels"] = False
    elif case == "scores_without_labels":
        args.update(keep_labels=False, scores=True,
                    relabelling=rc.Relabelling(S, np.array([[1, 2, -1], [1, 2, 0]]), np.zeros(2, np.int64), np.zeros((4, 3), np.uint32), np.array([1, 2])))
    elif case == "r_shape":
        args["r"] = np.array([1.0])
    elif case == "no_params":
        args["params"] = None
    with pytest.raises(ValueError):
        rc.predict_points(S, X, Y, **args)


def test_a_relabelling_of_other_samples_is_refused(no_library):
    S, X, Y, kw = _inputs()
    rel = rc.Relabelling(S[:1], np.array([[1, 2]]), np.zeros(1, np.int64), np.zeros((4, 3), np.uint32), np.array([1, 2]))
    with pytest.raises(ValueError):
        rc.predict_points(S, X, Y, relabelling=rel, **kw)
    bad = rc.Relabelling(S, np.array([[1, 7, -1], [1, 2, 0]]), np.zeros(2, np.int64), np.zeros((4, 3), np.uint32), np.array([1, 2]))
    with pytest.raises(ValueError):
        rc.predict_points(S, X, Y, relabelling=bad, **kw)


def test_counts_methods_of_a_prediction():
    c = np.array([[0, 3, 1], [2, 2, 0], [1, 0, 3]], np.uint32)
    P = rc.Prediction(None, None, counts=c, map_counts=c, pivot_labels=np.array([4, 9]))
    assert P.allocation_counts() is c
    assert np.array_equal(P.probabilities(), c / 4.0)
    assert np.array_equal(P.hard_allocation(), [4, 0, 9])           # row 1 ties: the smaller column
    with pytest.raises(ValueError):
        rc.Prediction(np.zeros((1, 1), np.int64), np.zeros((1, 1), np.int64)).allocation_counts()
