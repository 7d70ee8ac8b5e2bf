"""rc_partition_distances on the device against the NumPy restatement (partdist_ref.py), bit for bit: the reference is handed
the library's own table (rc_vi_gtable), and every output is an integer.  Then the Python layer built on it:
partitiondistances, expecteddistances, credibleball and hclustpointestimate(exact=True).  LOSS_TOL is test_gpu_visearch's
(the table's rounding, at most 2·2^-32 per VI); Binder losses are ratios of small integers, compared within 1e-12."""
import ctypes as C_
import functools
import types

import numpy as np
import pytest

import partdist_ref as PD
import psm_search_ref as R
import vi_search_ref as V
import redclust_amd as rc
from redclust_amd import _lib
from test_gpu_visearch import LOSS_TOL, SHAPES, library_table

pytestmark = pytest.mark.gpu

IDS = [f"n{s[0]}" for s in SHAPES]
WPB = 8                                     # labellings per workgroup (csrc/partdist.inc.hip)
VARIED = [(65, 50, 5, 0.2), (257, 17, 16, 0.2)]
LOSSES = ("binder", "VI", "ID")
# environment of a call: the default, the global histograms, a workspace of 1 KiB (a chunk holds a few samples and labellings at
# the most, one of each beyond n = 256), both, and Gq read from global memory instead of its copy in LDS with either histogram
MODES = {"default": {}, "global": {"RC_PARTDIST_HIST_GLOBAL": "1"}, "chunked": {"RC_PARTDIST_WORKSPACE_KIB": "1"},
         "global-chunked": {"RC_PARTDIST_HIST_GLOBAL": "1", "RC_PARTDIST_WORKSPACE_KIB": "1"},
         "gq-global": {"RC_PARTDIST_GQ_GLOBAL": "1"}, "global-gq-global": {"RC_PARTDIST_HIST_GLOBAL": "1", "RC_PARTDIST_GQ_GLOBAL": "1"}}


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(samples, labellings, reference outputs) of a shape; computed once and shared (never modified).  Labellings: all-one,
    all singletons (K = n: beyond 1024 clusters the global histograms on its own), labels under non-compact names up to n, the
    dendrogram's cuts K = 1..min(n, 16), and every sample itself."""
    n, m, K, noise = shape
    S = R.planted_counts(n, m, K, noise, seed=1000 + n)[0]
    merges = _lib.hclust(None, m, 0, samples=S)["merges"]
    rng = np.random.default_rng(n)
    odd = (n + 1 - rng.integers(1, max(n // 3, 1) + 1, n)).astype(np.int64)      # names in n − n/3 + 1 .. n, not all used
    cuts = [_lib.hclust_cut(merges, n, k) for k in range(1, min(n, 16) + 1)]
    labs = np.stack([np.ones(n, np.int64), np.arange(1, n + 1), odd] + cuts + list(S))
    ref = PD.distances_ref(labs, S, library_table(n))
    for a in (S, labs) + ref:
        a.setflags(write=False)
    return S, labs, ref


def assert_equals_reference(got, ref, rows=slice(None)):
    P, T, A, B = ref
    assert np.array_equal(got["sq"], P[rows]), "P"
    assert np.array_equal(got["phi"], T[rows]), "T"
    assert np.array_equal(got["lab_marg"], A[rows]), "labelling marginals"
    assert np.array_equal(got["smp_marg"], B), "sample marginals"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_output_equals_the_reference_bit_for_bit(shape, mode, monkeypatch):
    S, labs, ref = problem(shape)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    got = _lib.partition_distances(labs, S)
    print(shape, mode, "L", len(labs), "kernel_ms", got["kernel_ms"])
    assert_equals_reference(got, ref)
    # every sample against itself: distance 0, that is P and T equal to its own marginals
    own = np.arange(len(labs) - len(S), len(labs)), np.arange(len(S))
    assert np.array_equal(got["sq"][own], got["smp_marg"][:, 0]) and np.array_equal(got["phi"][own], got["smp_marg"][:, 1])


@pytest.mark.parametrize("mode", ["default", "global"])
@pytest.mark.parametrize("L", [1, WPB - 1, WPB, WPB + 1])
def test_labellings_around_one_workgroup_and_rows_on_their_own(L, mode, monkeypatch):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    for shape in (SHAPES[4], SHAPES[7]):                               # n = 65; n = 1025, whose row 1 (singletons) is always global
        S, labs, ref = problem(shape)
        got = _lib.partition_distances(labs[:L], S)
        assert_equals_reference(got, ref, slice(0, L))
        # a row does not depend on its neighbours: alone it gives the same integers
        for l in sorted({0, L // 2, L - 1}):
            one = _lib.partition_distances(labs[l:l + 1], S)
            assert np.array_equal(one["sq"][0], got["sq"][l]) and np.array_equal(one["phi"][0], got["phi"][l])
            assert np.array_equal(one["lab_marg"][0], got["lab_marg"][l])


def raw_call(S, labs, m=None, n=None, L=None, device=0, sq=True, phi=True, lm=True, sm=True, samples_null=False, labels_null=False):
    """rc_partition_distances through ctypes with any argument overridden; returns (rc, outputs or None per pointer)"""
    lib = _lib.lib()
    S, labs = np.ascontiguousarray(S, np.int64), np.ascontiguousarray(labs, np.int64)
    m = S.shape[0] if m is None else m
    n = S.shape[1] if n is None else n
    L = labs.shape[0] if L is None else L
    outs = [np.full((labs.shape[0], S.shape[0]), -1, np.int64) if sq else None, np.full((labs.shape[0], S.shape[0]), -1, np.int64) if phi else None,
            np.full((labs.shape[0], 3), -1, np.int64) if lm else None, np.full((S.shape[0], 3), -1, np.int64) if sm else None]
    ms = C_.c_double(-1.0)
    code = lib.rc_partition_distances(device, None if samples_null else S.ctypes.data, m, n, L, None if labels_null else labs.ctypes.data,
                                      *[None if o is None else o.ctypes.data for o in outs], C_.byref(ms))
    return code, outs


def test_any_output_may_be_null():
    S, labs, ref = problem(SHAPES[4])
    P, T, A, B = ref
    for keep in range(4):
        flags = [k == keep for k in range(4)]
        code, outs = raw_call(S, labs, sq=flags[0], phi=flags[1], lm=flags[2], sm=flags[3])
        assert code == 0
        assert np.array_equal(outs[keep], (P, T, A, B)[keep]), keep


def test_capacity_edge_n_32767():
    n = 32767
    rng = np.random.default_rng(n)
    S = np.stack([np.ones(n, np.int64), rng.integers(1, 3, n), rng.integers(1, 101, n)])
    labs = np.stack([np.ones(n, np.int64), np.arange(1, n + 1)])
    ref = PD.distances_ref(labs, S, library_table(n))
    got = _lib.partition_distances(labs, S)
    assert_equals_reference(got, ref)
    assert got["sq"][0, 0] == n * n and got["phi"][0, 0] == sum(int(g) for g in library_table(n))   # one cell of 32767: the largest count
    assert got["sq"][1, 0] == n and got["phi"][1, 0] == 0


def last_error():
    return _lib.lib().rc_last_error(None).decode()


def test_capacity_errors_come_before_anything_is_read():
    one = np.ones((1, 1), np.int64)
    big = np.ones((1, 32768), np.int64)
    code, _ = raw_call(big, big)
    assert code == -6 and "32768" in last_error()
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_CAPACITY"):
        _lib.partition_distances(big, big)
    code, _ = raw_call(one, one, m=1 << 31)                            # m·n = 2^31 with n = 1: the arrays are never touched
    assert code == -6 and "2^31" in last_error()
    code, _ = raw_call(np.ones((1, 4), np.int64), np.ones((1, 4), np.int64), m=1 << 29)
    assert code == -6 and "2^31" in last_error()
    code, _ = raw_call(one, one, L=65537)
    assert code == -6 and "65537" in last_error()


def test_argument_errors_leave_their_message():
    S, labs, _ = problem(SHAPES[3])
    n = S.shape[1]
    code, _ = raw_call(S, labs, samples_null=True)
    assert code == -1 and "NULL" in last_error()
    code, _ = raw_call(S, labs, labels_null=True)
    assert code == -1 and "NULL" in last_error()
    for kw in (dict(m=0), dict(n=0), dict(L=0), dict(m=-1)):
        code, _ = raw_call(S, labs, **kw)
        assert code == -1 and "m >= 1, n >= 1 and L >= 1" in last_error(), kw
    for bad in (0, n + 1, -3):
        X = S.copy(); X[2, 5] = bad
        code, _ = raw_call(X, labs)
        assert code == -1 and f"label {bad} of sample 3 at position 6" in last_error()
        Y = labs.copy(); Y[4, 0] = bad
        code, _ = raw_call(S, Y)
        assert code == -1 and f"label {bad} of labelling 5 at position 1" in last_error()
    code, _ = raw_call(S, labs, device=99)
    assert code == -1 and "device 99" in last_error()
    code, _ = raw_call(S, labs, device=-1)
    assert code == -1 and "device -1" in last_error()
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        X = S.copy(); X[0, 0] = 0
        _lib.partition_distances(labs, X)


# ---------------------------------------------------------------------------------------------------------------- Python layer

def test_partitiondistances_against_the_pair_measures():
    S, labs, _ = problem(SHAPES[4])
    n = S.shape[1]
    rows = [0, 1, 2, 10, len(labs) - 1]
    for loss, pair, tol in (("binder", lambda a, b: rc.binderloss(a, b, normalised=True), 1e-12), ("VI", rc.varinfo, LOSS_TOL),
                            ("ID", lambda a, b: rc.infodist(a, b, normalised=False), LOSS_TOL)):
        dist, info = rc.partitiondistances(labs[rows], S, loss)
        assert dist.shape == (len(rows), len(S)) and info["num"].dtype == np.int64
        assert np.array_equal(info["K_samples"], [len(np.unique(s)) for s in S])
        assert np.array_equal(info["K_labellings"], [len(np.unique(labs[l])) for l in rows])
        for a, l in enumerate(rows):
            for s in (0, 7, len(S) - 1):
                ref = pair(labs[l], S[s])
                print(loss, l, s, dist[a, s], ref)
                assert abs(dist[a, s] - ref) <= tol, (loss, l, s)
    unnorm, info = rc.partitiondistances(labs[2], types.SimpleNamespace(clusts=list(S)), "binder")     # one labelling, `.clusts`
    assert unnorm.shape == (1, len(S))
    assert info["num"][0, 3] == round(rc.binderloss(labs[2], S[3], normalised=False))
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.partitiondistances(labs[0], S, "omARI")


def test_expecteddistances_against_the_host_loops_and_the_search_criterion():
    shape = SHAPES[4]
    n, m = shape[0], shape[1]
    S, labs, _ = problem(shape)
    C = R.planted_counts(*shape, seed=1000 + n)[1]
    G = library_table(n)
    rows = [0, 1, 2, 5, len(labs) - 1]
    for loss, host in (("VI", lambda c: rc.expectedvi(c, S)), ("ID", lambda c: rc.expectedid(c, S)),
                       ("binder", lambda c: rc.expectedloss(c, C, m, "binder"))):
        losses, num = rc.expecteddistances(labs[rows], S, loss)
        assert num.dtype == np.int64
        for a, l in enumerate(rows):
            print(loss, l, losses[a], host(labs[l]))
            assert abs(losses[a] - host(labs[l])) <= LOSS_TOL, (loss, l)
            if loss == "VI":                                           # rc_vi_search's loss_num plus its constant
                assert int(num[a]) == V.q_direct(labs[l], S, G) + V.constant(S, G)
            if loss == "binder":
                assert int(num[a]) == R.binder_num(labs[l], C, m)
    # the search's own numbers: a converged run's loss_num is Q of its labelling
    run = _lib.vi_search(S, np.zeros((1, n), np.int64), np.arange(1, n + 1, dtype=np.int32)[None, :])
    _, num = rc.expecteddistances(run["labels"][0], S, "VI")
    assert int(num[0]) == int(run["loss_num"][0]) + V.constant(S, G)


@pytest.mark.parametrize("shape", VARIED, ids=[f"n{s[0]}" for s in VARIED])
def test_credibleball_equals_the_restated_definition(shape):
    n = shape[0]
    S = PD.varied_samples(*shape, seed=1000 + n)
    P, T, A, B = PD.distances_ref(S[:1], S, library_table(n))
    for loss in LOSSES:
        num = PD.numerators(P, T, A, B, loss)[0]
        for alpha in (0.05, 0.25):
            ref = PD.credibleball_ref(num, B[:, 2], alpha)
            got = rc.credibleball(S[0], S, loss, alpha)
            assert got["epsilon_num"] == ref["epsilon_num"] and got["level"] == ref["level"], (loss, alpha)
            assert got["epsilon"] == ref["epsilon_num"] / PD.denominator(loss, n)
            assert np.array_equal(got["ball"], ref["ball"]) and np.array_equal(got["distances_num"], num)
            assert np.array_equal(got["distances"], num / PD.denominator(loss, n)) and np.array_equal(got["K"], B[:, 2])
            for name in ("horizontal", "upper", "lower"):
                assert list(got[name + "_index"]) == ref[name + "_index"], (loss, alpha, name)
                assert np.array_equal(got[name], PD.distinct_partitions(S, ref[name + "_index"])), (loss, alpha, name)
            assert list(got["upper_index"]) != list(got["lower_index"])


def test_credibleball_keeps_the_ties_at_the_radius():
    S = R.planted_counts(64, 7, 4, 0.1, seed=1064)[0]
    got = rc.credibleball(S[0], S, "binder", 0.25)
    assert int(got["ball"].sum()) == 7 and got["level"] == 1.0 and len(got["horizontal_index"]) == 2


@pytest.mark.parametrize("loss", LOSSES)
def test_hclustpointestimate_exact_chooses_the_argmin_of_the_exact_curve(loss):
    shape = SHAPES[5]
    n, m = shape[0], shape[1]
    S, _, _ = problem(shape)
    samples = types.SimpleNamespace(clusts=list(S))
    clust, info = rc.hclustpointestimate(samples, loss, "average", maxK=16, exact=True)
    cuts = np.stack([_lib.hclust_cut(info["merges"], n, k) for k in range(1, 17)])
    P, T, A, B = PD.distances_ref(cuts, S, library_table(n))
    curve = [sum(int(x) for x in row) for row in PD.numerators(P, T, A, B, loss)]
    K = min(range(16), key=lambda k: (curve[k], k)) + 1
    print(loss, "K", info["K"], "curve", curve)
    assert info["K"] == K and np.array_equal(clust, cuts[K - 1])
    assert [int(x) for x in info["loss_num"]] == curve
    assert np.allclose(info["loss"], np.array(curve) / (PD.denominator(loss, n) * m), rtol=1e-15, atol=0)
    host = {"VI": lambda c: rc.expectedvi(c, S), "ID": lambda c: rc.expectedid(c, S),
            "binder": lambda c: rc.expectedloss(c, R.planted_counts(*shape, seed=1000 + n)[1], m, "binder")}[loss]
    assert abs(info["loss"][K - 1] - host(clust)) <= LOSS_TOL


def test_hclustpointestimate_without_exact_is_what_it_was():
    shape = SHAPES[5]
    n, m = shape[0], shape[1]
    S, _, _ = problem(shape)
    samples = types.SimpleNamespace(clusts=list(S))
    for loss in ("VI", "binder"):
        # the existing path, spelled out: the linkage with the bound's curve, the first minimum, the library's cut
        res = _lib.hclust(None, m, 0, maxcut=16 if loss == "VI" else 0, samples=S)
        curve = res["vilb"] if loss == "VI" else res["binder_num"][::-1][:16]
        want = _lib.hclust_cut(res["merges"], n, int(np.argmin(curve)) + 1)
        for kw in ({}, {"exact": False}):
            clust, info = rc.hclustpointestimate(samples, loss, "average", maxK=16, **kw)
            assert np.array_equal(clust, want) and info["K"] == int(np.argmin(curve)) + 1
            assert np.array_equal(info["loss"], curve if loss == "VI" else np.array([int(x) / (m * (n * (n - 1) // 2)) for x in curve]))
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.hclustpointestimate(samples, "ID", "average", maxK=16)
