"""The several-partition summary on the GPU (redclust.jl_amd/wasabi.py on rc_partition_distances and rc_vi_search_groups) against
the NumPy restatement tests/wasabi_ref.py handed the library's table: the driver is integer arithmetic between device calls
that are themselves exact, so particles, assignment, trace, objective and the chosen start have to agree bit for bit.  The one
f64 value, `wasserstein`, is W/(2^32·n·m): against f64 arithmetic on the partitions themselves (expectedvi's) it may differ by
the fixed point's 2·2^-32, the bound DESIGN.md §8 states for the exact VI search."""
import functools

import numpy as np
import pytest

import partdist_ref as PD
import wasabi_ref as W
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

FIXED_POINT_TOL = 2 * 2.0 ** -32
KW = dict(nstarts=2, seed=0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    S = W.planted_bimodal()[0] if name == "bimodal" else PD.varied_samples(n=48, m=40, K=4, noise=0.15, seed=7)
    G = _lib.vi_gtable(S.shape[1])
    G.setflags(write=False)
    return S, G


@functools.lru_cache(maxsize=None)
def reference(name, L):
    S, G = inputs(name)
    return W.wasabi_ref(S, L, G, **KW)


@functools.lru_cache(maxsize=None)
def result(name, L):
    return rc.wasabi(inputs(name)[0], L, **KW)


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("name", ["bimodal", "varied"])
def test_wasabi_equals_the_reference_bit_for_bit(name, L):
    got, ref = result(name, L), reference(name, L)
    print(name, L, "W", got.objective_num, "trace", got.trace, "starts", got.starts, "start", got.start, "weights", got.weights.tolist(),
          "iterations", got.iterations, "kernel ms", got.kernel_ms)
    assert np.array_equal(got.particles, ref["particles"]) and np.array_equal(got.assignment, ref["assignment"])
    assert got.trace == ref["trace"] and got.objective_num == ref["objective_num"] and got.start == ref["start"]
    assert got.starts == ref["starts"] and got.group_num == ref["group_num"] and np.array_equal(got.weights, ref["weights"])
    assert (got.iterations, got.converged) == (ref["iterations"], ref["converged"])
    assert got.wasserstein == ref["wasserstein"] and got.kernel_ms > 0


def test_the_planted_modes_come_back():
    S, A, B = W.planted_bimodal()
    got = result("bimodal", 2)
    assert np.array_equal(got.particles, np.stack([A, B])) and np.array_equal(got.weights * 48, [30, 18])


@pytest.mark.parametrize("name,L", [("bimodal", 2), ("varied", 3)])
def test_wasserstein_against_f64_arithmetic(name, L):
    S, _ = inputs(name)
    got = result(name, L)
    m = len(S)
    f64 = sum(rc.expectedvi(got.particles[l], S[got.assignment == l]) * int((got.assignment == l).sum()) for l in range(len(got.particles))) / m
    print(name, L, "wasserstein", got.wasserstein, "f64", f64, "difference", got.wasserstein - f64)
    assert abs(got.wasserstein - f64) <= FIXED_POINT_TOL
    assert sum(got.group_num) == got.objective_num


def test_scan_is_monotone_and_equals_the_reference():
    S, G = inputs("bimodal")
    out, curve = rc.wasabi_scan(S, [3, 1, 2, 4], **KW)
    ref, rcurve = W.scan_ref(S, [1, 2, 3, 4], G, **KW)
    print("curve", curve.tolist())
    assert list(out) == [1, 2, 3, 4] and np.array_equal(curve, rcurve)
    assert all(a >= b for a, b in zip(curve, curve[1:])) and curve[0] - curve[1] > curve[1] - curve[3]
    for L in out:
        assert np.array_equal(out[L].particles, ref[L]["particles"]) and out[L].objective_num == ref[L]["objective_num"], L
        assert out[L].start == ref[L]["start"] and out[L].trace == ref[L]["trace"], L


def test_expectedvi_and_credibleball_are_the_direct_calls():
    S, _ = inputs("varied")
    got = result("varied", 3)
    ev = got.expectedvi()
    direct, num = rc.expecteddistances(got.particles, S, "VI")
    assert np.array_equal(ev, direct)
    dist, info = rc.partitiondistances(got.particles, S, "VI")
    assert np.array_equal(num, info["num"].sum(axis=1))
    # the objective is the distances' minimum over the particles, summed
    assert int(info["num"].min(axis=0).sum()) == got.objective_num
    assert np.array_equal(np.argmin(info["num"], axis=0), got.assignment)
    for l in range(len(got.particles)):
        members = np.flatnonzero(got.assignment == l)
        ball = got.credibleball(l, 0.1)
        want = rc.credibleball(got.particles[l], S[members], "VI", 0.1)
        assert np.array_equal(ball["members"], members)
        for k in ("epsilon_num", "level", "epsilon"):
            assert ball[k] == want[k], (l, k)
        for k in ("ball", "horizontal_index", "upper_index", "lower_index", "distances_num", "horizontal", "upper", "lower"):
            assert np.array_equal(ball[k], want[k]), (l, k)
        assert int(ball["distances_num"].sum()) == got.group_num[l]
