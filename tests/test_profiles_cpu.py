"""Cluster profiles, the parts that need no GPU: the reference (tests/profiles_ref.py) against the definition, the host-only
silhouette arithmetic against exact rationals, the conventions, the argument errors the wrappers raise before any library
call, and the declarations of the interface (translation unit, build list, header, SIGNATURES, Julia)."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import profiles_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def int_matrix(n, seed, diagonal=True):
    """a symmetric integer matrix of positive entries below 2^40 with, if asked, a nonzero diagonal of both signs"""
    rng = np.random.default_rng(seed)
    Q = rng.integers(1, 1 << 40, (n, n))
    Q = np.maximum(Q, Q.T)
    np.fill_diagonal(Q, rng.integers(-(1 << 41), 1 << 41, n) if diagonal else 0)
    if diagonal and n > 1:
        Q[0, 0], Q[1, 1] = -(1 << 41), 1 << 41                   # both signs for certain, larger than any entry
    return Q


def labellings(n, seed):
    rng = np.random.default_rng(seed)
    K = max(1, int(round(np.sqrt(n))))
    out = [np.ones(n, np.int64), rng.permutation(n).astype(np.int64) + 1, np.where(np.arange(n) < max(n // 2, 1), min(2, n), 1),
           rng.permutation(n)[rng.integers(0, K, n)].astype(np.int64) + 1,
           np.array(sorted({min(3, n), min(7, n), n}), np.int64)[rng.integers(0, len({min(3, n), min(7, n), n}), n)]]
    return [np.asarray(z, np.int64) for z in out]


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_reference_matches_the_definition(n):
    Q = int_matrix(n, seed=n)
    for z in labellings(n, seed=10 + n):
        assert R.profile(Q, z) == R.profile_bruteforce(Q, z), z
    if n > 1:                                                   # the diagonal is in neither: another one changes nothing
        z = labellings(n, seed=3)[3]
        assert Q.diagonal().min() < 0 < Q.diagonal().max()
        assert R.profile(Q, z) == R.profile(int_matrix(n, seed=n, diagonal=False), z)


def test_reference_tie_rules_on_a_constant_matrix():
    n = 9
    Q = np.full((n, n), 5, np.int64)
    z = np.array([4, 4, 9, 9, 9, 2, 2, 2, 2])
    p = R.profile(Q, z)
    assert p == R.profile_bruteforce(Q, z)
    assert p["labels"] == [2, 4, 9] and p["medoids"] == [6, 1, 3]          # every member ties: the smallest index
    assert p["neighbour"] == [2, 2, 2, 2, 2, 4, 4, 4, 4]                    # every other cluster ties in mean: the smallest label
    assert p["nearest"] == [20, 20, 20, 20, 20, 10, 10, 10, 10]


def raw_of(Q, batch):
    """the reference's profiles of a batch in the shape Context.profiles returns them (eD = 0)"""
    ps = [R.profile(Q, z) for z in batch]
    return ps, dict(within=np.array([p["within"] for p in ps], np.int64), nearest=np.array([p["nearest"] for p in ps], np.int64),
                    neighbour=np.array([p["neighbour"] for p in ps], np.int64))


@pytest.mark.parametrize("n", [2, 7, 40])
def test_silhouettes_from_sums_against_exact_rationals(n):
    """each of the three float operations — the two means and the quotient — carries 2^-53 relative error and the difference is
    taken relative to max(ā, b̄) <= 1 in magnitude, so a few units of 2^-53 bound the absolute error: 1e-12 leaves three orders"""
    Q = int_matrix(n, seed=20 + n)
    batch = labellings(n, seed=30 + n)
    ps, raw = raw_of(Q, batch)
    s = rc.silhouettes_from_sums(raw["within"], raw["nearest"], raw["neighbour"], np.stack(batch))
    assert s.shape == (len(batch), n) and s.dtype == np.float64
    for l, z in enumerate(batch):
        exact = R.silhouette_exact(ps[l], z)
        assert all(-1 <= x <= 1 for x in exact)
        err = max(abs(Fraction(float(s[l, i])) - exact[i]) for i in range(n))
        print(n, l, float(err))
        assert err <= Fraction(1, 10 ** 12), (l, float(err))
    one = rc.silhouettes_from_sums(raw["within"][3], raw["nearest"][3], raw["neighbour"][3], batch[3])
    assert one.shape == (n,) and np.array_equal(one, s[3])


def test_conventions_give_zero():
    n = 12
    Q = int_matrix(n, seed=4)
    z_one, z_single = np.ones(n, np.int64), np.arange(1, n + 1)
    z_mixed = np.array([1] * 5 + [2] * 6 + [7])                            # point 12 is a singleton beside two clusters
    ps, raw = raw_of(Q, [z_one, z_single, z_mixed])
    s = rc.silhouettes_from_sums(raw["within"], raw["nearest"], raw["neighbour"], np.stack([z_one, z_single, z_mixed]))
    assert not s[0].any() and not s[1].any()                               # K = 1; all singletons
    assert s[2, 11] == 0.0 and s[2, :11].all()
    assert ps[0]["neighbour"] == [0] * n and ps[0]["nearest"] == [0] * n
    assert ps[1]["within"] == [0] * n and ps[1]["medoids"] == list(range(1, n + 1))
    # max(ā, b̄) = 0: all distances zero
    zero = rc.silhouettes_from_sums(np.zeros(4, np.int64), np.zeros(4, np.int64), np.array([2, 2, 1, 1]), np.array([1, 1, 2, 2]))
    assert not zero.any()
    with pytest.raises(ValueError, match="one shape"):
        rc.silhouettes_from_sums(np.zeros(4, np.int64), np.zeros(3, np.int64), np.zeros(4, np.int64), np.ones(4, np.int64))


def test_the_source_is_part_of_the_build():
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    tu = open(os.path.join(csrc, "redclust_hip.hip")).read()
    assert '#include "profile.inc.hip"' in tu
    assert tu.index('#include "profile.inc.hip"') > tu.index('#include "score.inc.hip"')
    assert os.path.join(csrc, "profile.inc.hip") in _lib._sources()        # build() watches it
    src = re.sub(r"//.*", "", open(os.path.join(csrc, "profile.inc.hip")).read())
    assert "asm" not in src                                                # plain C++ and vector memory operations only
    assert "slab::run_rows" in src and "k_predict_sums" not in src         # phase 1 is shared, not copied or instantiated anew:
    slab = re.sub(r"//.*", "", open(os.path.join(csrc, "slab.inc.hip")).read())
    assert "asm" not in slab and "launch_sums" in slab.split("run_rows(", 1)[1]   # the slab driver launches it
    assert "rc_load_L" not in src and "rc_qlog" not in src                 # no logarithm is involved


def test_header_signatures_and_julia_agree():
    import test_oracle_cpu as T
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    protos = T._header_prototypes(hdr)
    want = ["rc_ctx*", "int64_t", "int64_t*", "int64_t*", "int64_t*", "int64_t*", "int64_t", "int64_t*", "int64_t*", "int64_t*",
            "int32_t*", "double*"]
    assert re.fullmatch(r"rc_[a-z_]+", "rc_cluster_profiles")
    assert protos["rc_cluster_profiles"] == ("int32_t", want), protos["rc_cluster_profiles"]
    res, sig = rc.SIGNATURES["rc_cluster_profiles"]
    assert res is C.c_int32 and len(sig) == len(want)
    for k, (ct, py) in enumerate(zip(want, sig)):
        if ct == "int64_t":
            assert py is C.c_int64, (k, py)
        else:
            assert py in (C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)), (k, ct, py)
    assert hasattr(rc.lib(), "rc_cluster_profiles")
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    assert "ccall((:rc_cluster_profiles, LIB)" in jl
    calls = [c for c in T._julia_ccalls(jl) if c[0] == "rc_cluster_profiles"]
    assert len(calls) == 1
    _, jret, jargs, npassed = calls[0]
    assert jret == "Int32" and len(jargs) == npassed == len(want)
    for jt, ct in zip(jargs, want):
        assert ct in T._JL2C[jt], (jt, ct)
    assert "function clusterprofiles(b::HIPBackend" in jl and "export clusterprofiles" in jl
    T.test_julia_glue_ccalls_match_the_header()


def test_argument_errors_that_need_no_device():
    L = rc.lib()
    lab = np.ones((1, 3), np.int64)
    assert L.rc_cluster_profiles(None, 1, lab.ctypes.data, None, None, None, 0, None, None, None, None, None) == -1
    assert "NULL ctx" in L.rc_last_error(None).decode()
    ctx = rc.Context.__new__(rc.Context)                        # the wrapper's own checks need no library call either
    ctx.n, ctx.h, ctx.L = 3, None, L
    with pytest.raises(ValueError, match="n columns"):
        ctx.profiles(np.ones((2, 4), np.int64))
    with pytest.raises(ValueError, match="n columns"):
        ctx.profiles(np.ones((2, 2, 3), np.int64))
    with pytest.raises(ValueError, match="integer labels"):
        rc.clusterprofiles(ctx, np.ones((2, 3)))
    with pytest.raises(ValueError, match="no labellings"):
        rc.clusterprofiles(ctx, [])


def test_hclustpointestimate_checks_the_silhouette_criterion_first():
    counts = np.zeros((2, 2), np.uint32)
    with pytest.raises(ValueError, match="exact=True"):
        rc.hclustpointestimate(counts, numsamples=1, criterion="silhouette", exact=True, data=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="needs data"):
        rc.hclustpointestimate(counts, numsamples=1, criterion="silhouette")
    with pytest.raises(ValueError, match="linkage"):
        rc.hclustpointestimate(counts, numsamples=1, criterion="silhouette", linkage="ward", data=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="criterion"):                     # unknown strings keep raising
        rc.hclustpointestimate(counts, numsamples=1, criterion="silhouettes")
