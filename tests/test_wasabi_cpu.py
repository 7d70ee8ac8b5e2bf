"""The several-partition summary without a GPU: the NumPy restatement the device is held to (tests/wasabi_ref.py) against a brute
force over all pairs of partitions, on planted inputs and at its edges; the ABI declarations of rc_vi_search_groups; and the
argument errors of the Python layer that are raised before the library is loaded."""
import os
import re

import numpy as np
import pytest

import psm_search_ref as R
import partdist_ref as PD
import vi_search_ref as V
import wasabi_ref as W
import redclust_amd as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_modes_n6():
    """n = 6, m = 12: seven samples around {123}{456} and five around {12}{34}{56}, one point moved in some of them"""
    A, B = [1, 1, 1, 2, 2, 2], [1, 1, 2, 2, 3, 3]
    rows = [A] * 5 + [[1, 1, 2, 2, 2, 2], [1, 1, 1, 1, 2, 2]] + [B] * 4 + [[1, 1, 2, 2, 3, 1]]
    return np.array(rows, np.int64)


@pytest.fixture(scope="module")
def planted():
    S, A, B = W.planted_bimodal()
    G = V.numpy_G(S.shape[1])
    out, curve = W.scan_ref(S, [1, 2, 3, 4], G, nstarts=2, seed=0)
    return S, A, B, out, curve


def test_brute_force_bounds_the_reference_and_is_met_on_two_planted_modes():
    S = _two_modes_n6()
    G = V.numpy_G(6)
    best2, best1 = W.brute_force_pairs(S, G)
    r2 = W.wasabi_ref(S, 2, G, nstarts=3, seed=0)
    r1 = W.wasabi_ref(S, 1, G, nstarts=2, seed=0)
    print("two modes: optimum", best2, best1, "reference", r2["objective_num"], r1["objective_num"])
    assert r2["objective_num"] == best2 and r1["objective_num"] >= best1
    assert sorted((r2["weights"] * 12).round().astype(int).tolist()) == [5, 7]
    # never below the optimum, whatever the samples
    for seed in range(4):
        X = np.random.default_rng(seed).integers(1, 4, size=(12, 6)).astype(np.int64)
        b2, b1 = W.brute_force_pairs(X, G)
        for s in range(2):
            w2 = W.wasabi_ref(X, 2, G, nstarts=2, seed=s)["objective_num"]
            w1 = W.wasabi_ref(X, 1, G, nstarts=1, seed=s)["objective_num"]
            print("random", seed, s, "optimum", b2, b1, "reference", w2, w1)
            assert w2 >= b2 and w1 >= b1 and w2 <= w1


def test_planted_bimodal_posterior_is_recovered(planted):
    S, A, B, out, curve = planted
    r = out[2]
    print("curve", curve.tolist(), "trace", r["trace"], "weights", r["weights"].tolist())
    assert np.array_equal(r["particles"][0], A) and np.array_equal(r["particles"][1], B)
    assert np.array_equal(r["weights"] * 48, [30, 18])
    assert np.array_equal(r["assignment"], [0] * 30 + [1] * 18)
    assert all(a > b for a, b in zip(r["trace"], r["trace"][1:])) and len(r["trace"]) >= 2
    assert curve[0] - curve[1] > curve[1] - curve[3] > 0
    assert sum(r["group_num"]) == r["objective_num"] == r["trace"][-1]
    # the objective is what the distances say
    G = V.numpy_G(S.shape[1])
    d = np.array(W.vi_distances(r["particles"], S, G), dtype=object)
    assert sum(min(d[0][s], d[1][s]) for s in range(48)) == r["objective_num"]
    assert abs(r["wasserstein"] - r["objective_num"] / (2.0 ** 32 * 40 * 48)) < 1e-15


def test_scan_curve_never_rises(planted):
    _, _, _, out, curve = planted
    nums = [out[L]["objective_num"] for L in (1, 2, 3, 4)]
    assert all(a >= b for a, b in zip(nums, nums[1:])) and all(a >= b for a, b in zip(curve, curve[1:]))
    for L in (1, 2, 3, 4):
        assert all(a >= b for a, b in zip(out[L]["trace"], out[L]["trace"][1:]))     # W never rises within a start


def test_empty_group_is_repaired_by_the_farthest_sample():
    S, A, B = W.planted_bimodal()
    G = V.numpy_G(40)
    # two copies of one particle: the second gets no sample (ties go to the lower index) and is repaired
    init = np.stack([A, A])
    r = W.wasabi_ref(S, 2, G, nstarts=0, init=init)
    d0 = W.vi_distances(A, S, G)[0]
    far = max(range(48), key=lambda s: (d0[s], -s))
    first = sum(d0)
    rep = W.vi_distances(np.stack([A, R.sortlabels(S[far])]), S, G)
    assert r["trace"][0] == first and r["trace"][1] == sum(min(a, b) for a, b in zip(*rep)) < first
    assert len(r["particles"]) == 2 and np.array_equal(r["particles"][0], A) and np.array_equal(r["particles"][1], B)
    assert r["start"] == 0 and r["converged"]


def test_fewer_distinct_samples_than_particles():
    a, b = np.arange(10) % 2 + 1, np.arange(10) // 5 + 1
    S = np.stack([a, b, a, a, b, 3 - a]).astype(np.int64)                # 3 − a is a's partition under other names
    G = V.numpy_G(10)
    r = W.wasabi_ref(S, 4, G, nstarts=2, seed=3)
    assert r["objective_num"] == 0 and r["wasserstein"] == 0.0 and r["converged"]
    assert len(r["particles"]) == 2
    assert np.array_equal(r["particles"][0], R.sortlabels(a)) and np.array_equal(r["particles"][1], R.sortlabels(b))
    assert np.array_equal(r["weights"], [4 / 6, 2 / 6]) and np.array_equal(r["assignment"], [0, 1, 0, 0, 1, 0])
    assert r["group_num"] == [0, 0]


def test_one_particle_is_the_minimum_expected_vi_search():
    S = PD.varied_samples(n=24, m=15, K=3, noise=0.15, seed=5)
    G = V.numpy_G(24)
    r = W.wasabi_ref(S, 1, G, nstarts=2, seed=1)
    d = W.vi_distances(r["particles"][0], S, G)[0]
    assert r["objective_num"] == sum(d) == r["group_num"][0] and np.array_equal(r["assignment"], np.zeros(15))
    assert r["objective_num"] == V.q_direct(r["particles"][0], S, G) + V.constant(S, G)     # rc_vi_search's criterion
    assert np.array_equal(r["weights"], [1.0])
    # no sample is a better single particle than the searched partition
    assert r["objective_num"] <= min(sum(W.vi_distances(s, S, G)[0]) for s in S)


def test_a_run_is_a_function_of_the_seed():
    S = PD.varied_samples(n=24, m=15, K=3, noise=0.15, seed=5)
    G = V.numpy_G(24)
    a, b = W.wasabi_ref(S, 3, G, nstarts=2, seed=4), W.wasabi_ref(S.copy(), 3, G, nstarts=2, seed=4)
    for k in ("particles", "assignment", "weights"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("trace", "objective_num", "starts", "start", "iterations", "group_num"):
        assert a[k] == b[k], k
    seeds = {tuple(W.wasabi_ref(S, 3, G, nstarts=1, nruns=0, seed=s)["trace"]) for s in range(6)}
    assert len(seeds) > 1                                                # the seed does enter


def _nargs(proto):
    return len([a for a in proto.split(",") if a.strip()])


def test_header_signatures_and_julia_agree_on_rc_vi_search_groups():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "redclust_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+rc_vi_search_groups\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m
    assert "rc_vi_search_groups" in rc.SIGNATURES and _nargs(m.group(1)) == len(rc.SIGNATURES["rc_vi_search_groups"][1]) == 16
    # rc_vi_search's list with the groups in it: the shared parameters keep their types and order
    args, base = rc.SIGNATURES["rc_vi_search_groups"][1], rc.SIGNATURES["rc_vi_search"][1]
    mine, theirs = args[6:7] + args[8:], base[4:]                        # best (index 7) is an array here, one int there
    assert args[:4] == base[:4] and mine[:7] + mine[8:] == theirs[:7] + theirs[8:]
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    assert "ccall((:rc_vi_search_groups, LIB)" in jl and "function wasabi(" in jl and "function visearchgroups(" in jl
    import test_oracle_cpu
    test_oracle_cpu.test_julia_glue_ccalls_match_the_header()
    for name in ("searchvigroups", "wasabi", "wasabi_scan", "WasabiResult"):
        assert hasattr(rc, name), name
    assert callable(rc._lib.vi_search_groups)


def test_argument_errors_raised_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(rc._lib, "lib", no_library)
    S = np.array(_two_modes_n6())
    with pytest.raises(ValueError, match="L must be at least 1"):
        rc.wasabi(S, 0)
    with pytest.raises(ValueError, match="no start"):
        rc.wasabi(S, 2, nstarts=0)
    with pytest.raises(ValueError, match="maxiter"):
        rc.wasabi(S, 2, maxiter=0)
    with pytest.raises(ValueError, match="maxiter"):
        rc.wasabi(S, 2, maxsweeps=0)
    with pytest.raises(ValueError, match="negative"):
        rc.wasabi(S, 2, nruns=-1)
    with pytest.raises(ValueError, match="negative"):
        rc.wasabi(S, 2, maxK=-1)
    with pytest.raises(ValueError, match="init must hold"):
        rc.wasabi(S, 2, init=np.ones((3, 6), np.int64))
    with pytest.raises(ValueError, match="init must hold"):
        rc.wasabi(S, 2, init=np.ones((2, 5), np.int64))
    with pytest.raises(ValueError, match="no samples"):
        rc.wasabi(np.zeros((0, 6), np.int64), 2)
    with pytest.raises(ValueError, match="sets init itself"):
        rc.wasabi_scan(S, [1, 2], init=S[:1])
    with pytest.raises(ValueError, match="positive integers"):
        rc.wasabi_scan(S, [0, 1])
    ident = np.arange(1, 7, dtype=np.int32)[None, :]
    with pytest.raises(ValueError, match="one group id per sample"):
        rc.searchvigroups(S, np.zeros(5, np.int32), S[:1], ident, [0])
    with pytest.raises(ValueError, match="one group id per run"):
        rc.searchvigroups(S, np.zeros(12, np.int32), S[:1], ident, [0, 0])
    with pytest.raises(ValueError, match="init and order"):
        rc.searchvigroups(S, np.zeros(12, np.int32), S[:2], ident, [0, 0])
