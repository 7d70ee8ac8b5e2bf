"""The PEAR search without a GPU: the criterion's exact integers against mcclust's floating-point definition, the properties
of the NumPy restatement of a run (tests/pear_search_ref.py) that the device is then held to bit for bit, the host
arithmetic of expectedpears / maxpear / expectedari, the argument errors raised before any device work, and the interface
(header, SIGNATURES, Julia).  What needs the device — expectedari and maxpear end to end — is in test_gpu_pearsearch.py."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import np_transcription as T
import pear_search_ref as R
import redclust_amd as rc
from redclust_amd import pointestimate as PE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expectedpear_equals_mcclusts_floating_point_definition():
    for n, m, K, seed in ((2, 3, 2, 0), (7, 5, 3, 1), (40, 20, 4, 2), (65, 50, 5, 3)):
        S, C = R.planted_counts(n, m, K, 0.3, seed)
        rng = np.random.default_rng(seed)
        for c in (S[0], np.ones(n, np.int64), np.arange(1, n + 1), rng.integers(1, 4, n), rng.integers(1, n + 1, n)):
            want = R.pear_float(c, C, m)
            got = rc.expectedpear(c, C, m)
            num, den = rc.pearfraction(c, C, m)
            assert (num, den) == R.pear_num_den(c, C, m) and den > 0 and got == num / den
            if np.isnan(want):                                   # mcclust's 0/0: the convention here is 0
                assert (num, den) == (0, 1)
            else:
                assert abs(got - want) <= 1e-12, (n, got, want)


def test_degenerate_inputs_give_zero_where_den_is_zero():
    # n = 1
    assert rc.pearfraction([1], np.array([[4]], np.uint32), 4) == (0, 1) and rc.expectedpear([1], np.array([[4]], np.uint32), 4) == 0.0
    n, m = 6, 3
    # every sample all singletons: P = 0, and den = 0 for the all-singletons labelling (A = 0)
    C = (m * np.eye(n)).astype(np.uint32)
    assert rc.pearfraction(np.arange(1, n + 1), C, m) == (0, 1)
    assert rc.expectedpear(np.arange(1, n + 1), C, m) == 0.0
    assert rc.expectedpear(np.ones(n, np.int64), C, m) == 0.0          # num = 0 there too, den = T·m·T > 0
    # every sample one cluster: den = 0 for the one-cluster labelling
    C = np.full((n, n), m, np.uint32)
    assert rc.pearfraction(np.ones(n, np.int64), C, m) == (0, 1)
    assert rc.expectedpear(np.ones(n, np.int64), C, m) == 0.0
    assert R.pear_num_den(np.zeros(n, np.int64), C, m)[1] > 0           # unallocated points are singletons: A = 0, den = T·P


def starts(n, K, seed):
    rng = np.random.default_rng(seed)
    mixed = rng.integers(1, K + 1, n)
    mixed[rng.permutation(n)[: n // 2]] = 0
    inits = [np.zeros(n, np.int64), np.ones(n, np.int64), mixed.astype(np.int64)]
    orders = [rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]
    return inits, orders


@pytest.mark.parametrize("n,m,K,noise", [(1, 3, 1, 0.0), (2, 3, 2, 0.0), (3, 2, 2, 0.3), (33, 7, 3, 0.2), (65, 20, 6, 0.3)])
def test_reference_runs_never_lose_and_never_see_a_negative_den(n, m, K, noise):
    _, C = R.planted_counts(n, m, K, noise, seed=10 + n)
    for init, order in zip(*starts(n, K, n)):
        for maxK, maxsweeps in ((0, 100), (2, 100), (0, 1)):
            init_ = np.where(init > maxK, maxK, init) if maxK else init
            out = R.pear_search_ref(C, m, init_, order, maxK=maxK, maxsweeps=maxsweeps)
            assert out["min_den"] >= 0                                              # 2: den >= 0 on every state scored
            assert out["den"] > 0 and Fraction(out["num"], out["den"]) >= out["start"]   # 5: never below the start
            assert Fraction(out["num"], out["den"]) <= 1
            assert (out["num"], out["den"]) == rc.pearfraction(out["labels"], C, m)
            if maxK:
                assert out["K"] <= maxK
            if maxsweeps == 100:
                assert out["converged"]


def test_identical_samples_are_recovered_with_pear_one():
    n, m = 24, 5
    truth = np.random.default_rng(4).integers(1, 5, n)
    C = (m * (truth[:, None] == truth[None, :])).astype(np.uint32)
    out = R.pear_search_ref(C, m, np.zeros(n, np.int64), np.random.default_rng(5).permutation(n) + 1)
    assert np.array_equal(out["labels"], R.sortlabels(truth)) and out["num"] == out["den"] > 0 and out["converged"]


def test_ari_from_sums_equals_the_transcribed_randindex():
    rng = np.random.default_rng(6)
    assert PE._ari_from_sums([[1]], [1], [1], 1).tolist() == [[0.0]]                 # n = 1: no pairs (randindex divides by 0 there)
    for n in (2, 9, 50):
        S = rng.integers(1, 5, (6, n)).astype(np.int64)
        S[0] = 1                                                                     # one cluster
        S[1] = np.arange(1, n + 1)                                                   # all singletons
        labs = np.stack([S[0], S[1], S[2], rng.integers(1, 3, n)])
        sq = np.array([[(T.contingency(a, b).astype(np.int64) ** 2).sum() for b in S] for a in labs])
        marg = lambda X: np.array([(np.bincount(x).astype(np.int64) ** 2).sum() for x in X])
        got = PE._ari_from_sums(sq, marg(labs), marg(S), n).mean(axis=1)
        want = [np.mean([T.randindex(a, b)[0] for b in S]) for a in labs]
        assert np.allclose(got, want, rtol=0, atol=1e-12), (n, got, want)


def test_pears_from_binder_numerators_and_the_exact_choice():
    n, m = 40, 20
    S, C = R.planted_counts(n, m, 4, 0.3, seed=8)
    labs = np.stack([S[0], S[1], np.ones(n, np.int64), np.arange(1, n + 1), S[0]])
    P = R.pear_parts(labs[0], C)[2]
    binder = [P + m * R.pear_parts(c, C)[1] - 2 * R.pear_parts(c, C)[0] for c in labs]      # P + m·A − 2·X
    pear, num, den = PE._pears_from_binder(binder, [PE._within_pairs(c) for c in labs], P, m, n)
    for k, c in enumerate(labs):
        assert (int(num[k]), int(den[k])) == rc.pearfraction(c, C, m) and pear[k] == rc.expectedpear(c, C, m)
    fr = [Fraction(int(a), int(b)) for a, b in zip(num, den)]
    assert PE._first_max_fraction(num, den) == fr.index(max(fr))                    # the first of the two equal maxima, if any
    assert PE._first_max_fraction([1, 2, 2, 4], [2, 4, 3, 6]) == 2                  # 1/2 = 2/4 < 2/3 = 4/6


def test_argument_errors_are_value_errors():
    n, m = 6, 3
    S, C = R.planted_counts(n, m, 2, 0.2, seed=9)
    with pytest.raises(ValueError):
        rc.expectedpear(np.ones(n + 1, np.int64), C, m)
    with pytest.raises(ValueError):
        rc.expectedpears(np.ones((2, n + 1), np.int64), C, m)
    with pytest.raises(ValueError):
        rc.expectedpears(np.ones((2, n), np.int64), C)                              # a count matrix needs numsamples
    with pytest.raises(ValueError):
        rc.searchmaxpear()
    with pytest.raises(ValueError):
        rc.searchmaxpear(C)
    with pytest.raises(ValueError):
        rc.searchmaxpear(C[:, :3], numsamples=m)
    with pytest.raises(ValueError, match="Invalid method"):
        rc.maxpear(C, "median", numsamples=m)
    with pytest.raises(ValueError, match="draws"):
        rc.maxpear(C, "draws", numsamples=m)
    with pytest.raises(ValueError, match="search keywords"):
        rc.maxpear(C, "avg", numsamples=m, nruns=2)
    with pytest.raises(ValueError):
        rc.expectedari(np.ones((1, n + 1), np.int64), S)
    # the existing entry points do not learn the new criterion
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.searchpointestimate(C, "omARI", numsamples=m)
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.expectedloss(S[0], C, m, "omARI")


def _nargs(arglist):
    return len([a for a in re.sub(r"/\*.*?\*/", "", arglist, flags=re.S).split(",") if a.strip()])


def test_header_signatures_and_julia_agree_on_the_pear_entries():
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    for name, nargs in (("rc_pear_search", 13), ("rc_pear_search_ctx", 11), ("rc_pear_search_samples", 14)):
        m = re.search(r"int32_t " + name + r"\((.*?)\);", hdr, flags=re.S)
        assert m and _nargs(m.group(1)) == len(rc.SIGNATURES[name][1]) == nargs, name
    # the three mirror rc_psm_search* without the loss argument
    for a, b in (("rc_pear_search", "rc_psm_search"), ("rc_pear_search_ctx", "rc_psm_search_ctx"), ("rc_pear_search_samples", "rc_psm_search_samples")):
        assert len(rc.SIGNATURES[a][1]) == len(rc.SIGNATURES[b][1]) - 1
    import test_oracle_cpu
    fields = dict(test_oracle_cpu._header_structs(hdr))["rc_pear_run_t"]
    assert fields == [("pear", "double"), ("num", "int64_t"), ("den", "int64_t"), ("sweeps", "int32_t"), ("converged", "int32_t"),
                      ("moves", "int64_t"), ("K", "int32_t")]
    assert [f[0] for f in rc._lib.RcPearRun._fields_] == [f[0] for f in fields]
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    assert "ccall((:rc_pear_search_samples, LIB)" in jl and "ccall((:rc_pear_search, LIB)" in jl
    assert "function searchmaxpear(" in jl and "function expectedpear(" in jl
    test_oracle_cpu.test_julia_glue_ccalls_match_the_header()


def test_kernel_resources():
    """The PEAR instances spill nothing, and their argmax partials are static LDS of their own: the Binder and VI instances of
    the same template keep the static LDS they had (576 and 512 bytes) and stay without scratch."""
    import isa
    res = isa.resources(r"psm8k_searchILi")
    assert len(res) == 12, sorted(res)
    for name, r in res.items():
        loss = int(name.split("k_searchILi")[1][0])
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == {0: 576, 1: 512, 2: 896}[loss], (name, r)
