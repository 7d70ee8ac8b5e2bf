"""The exact expected-VI search on the GPU (csrc/visearch.inc.hip through rc_vi_gtable / rc_vi_search and
searchpointestimate(exact=True)).  A run is integer arithmetic on the table Gq, so the device is held to
tests/vi_search_ref.py bit for bit, the reference being handed the library's own table; the table itself is checked against
NumPy's separately (libm and NumPy may round an entry differently: Gq·2^-32 <= 4.3·10^10, where an ulp is 7.6·10^-6, so the
two differ by at most 1).

Shapes: the wave (63/64/65) and workgroup (1000/1025 around the 1024 threads) edges of n, n = 1 and 2; m is never a multiple
of the 16 waves.  Runs per shape: a random order from empty labels, the identity order from one cluster, the reverse order
from labels of which half are unallocated.  The returned loss is (Q + constant)/(2^32·n·m): the table's rounding contributes
at most 2·2^-32 ≈ 4.7e-10, the f64 sums of expectedvi far less: LOSS_TOL = 1e-9."""
import ctypes as C_
import functools

import numpy as np
import pytest

import psm_search_ref as R
import vi_search_ref as V
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1, 0.0), (2, 3, 2, 0.0), (63, 7, 3, 0.1), (64, 7, 4, 0.1), (65, 50, 5, 0.2), (257, 17, 16, 0.2),
          (1000, 20, 40, 0.3), (1025, 9, 10, 0.2)]
IDS = [f"n{s[0]}" for s in SHAPES]
LOSS_TOL = 1e-9
KEYS = ("loss_num", "sweeps", "moves", "converged", "K")


@functools.lru_cache(maxsize=None)
def library_table(n):
    G = _lib.vi_gtable(n)
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(samples, init 3×n, order 3×n) of a shape; computed once and shared (never modified)."""
    n, m, K, noise = shape
    S, _ = R.planted_counts(n, m, K, noise, seed=1000 + n)
    rng = np.random.default_rng(n)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]).astype(np.int32)
    mixed = rng.integers(1, min(K, n) + 1, n)
    mixed[rng.permutation(n)[: n // 2]] = 0
    init = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), mixed.astype(np.int64)])
    for a in (S, init, order):
        a.setflags(write=False)
    return S, init, order


def run_inits(shape, maxK):
    """the three starts, clipped to the slot cap (maxK, or the samples' largest cluster count)"""
    S, init, _ = problem(shape)
    cap = maxK if maxK else V.relabel(S)[1]
    return np.where(init > cap, cap, init)


@functools.lru_cache(maxsize=None)
def reference(shape, maxK, maxsweeps):
    S, _, order = problem(shape)
    init = run_inits(shape, maxK)
    return [V.vi_search_ref(S, library_table(shape[0]), init[r], order[r], maxK=maxK, maxsweeps=maxsweeps) for r in range(3)]


def assert_equals_reference(got, refs, what):
    for r, ref in enumerate(refs):
        print(what, r, "sweeps", got["sweeps"][r], "moves", got["moves"][r], "K", got["K"][r], "Q", got["loss_num"][r])
        assert np.array_equal(got["labels"][r], ref["labels"]), (what, r)
        for k in KEYS:
            assert got[k][r] == ref[k], (what, r, k, got[k][r], ref[k])
    assert got["best"] == int(np.argmin([ref["loss_num"] for ref in refs]))


def test_table_against_numpy():
    G = library_table(8192)
    ref = V.numpy_G(8192)
    diff = np.abs(G - ref)
    print("entries that differ from NumPy's:", int((diff != 0).sum()), "largest difference", int(diff.max()))
    assert G[0] == 0 and len(G) == 8192
    assert diff.max() <= 1
    assert np.array_equal(library_table(5), G[:5])


@pytest.mark.parametrize("maxK,maxsweeps", [(0, 100), (2, 100), (0, 1), (2, 1)], ids=["free", "maxK2", "onesweep", "maxK2-onesweep"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_search_equals_the_reference_bit_for_bit(shape, maxK, maxsweeps):
    n = shape[0]
    S, _, order = problem(shape)
    init = run_inits(shape, maxK)
    got = _lib.vi_search(S, init, order, maxK=maxK, maxsweeps=maxsweeps)
    assert_equals_reference(got, reference(shape, maxK, maxsweeps), shape)
    for r in range(3):
        if maxK:
            assert got["K"][r] <= maxK
        if maxsweeps == 1 and n > 1:
            assert got["sweeps"][r] == 1
    if maxsweeps == 1 and n > 2:
        assert not got["converged"][0]              # a run from empty labels moves every point in its first sweep


@functools.lru_cache(maxsize=None)
def cap_problem():
    """n = 300; one sample has 70 clusters, so a sample's label crosses a wave's width as well"""
    n, m = 300, 7
    S, _ = R.planted_counts(n, m, 5, 0.2, seed=42)
    S = S.copy()
    S[3] = np.random.default_rng(1).permutation(np.arange(n) % 70) + 1
    rng = np.random.default_rng(2)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]).astype(np.int32)
    S.setflags(write=False); order.setflags(write=False)
    return S, order


@pytest.mark.parametrize("maxK", [63, 64, 65, 130])
def test_slot_cap_at_the_lane_edges(maxK):
    n = 300
    S, order = cap_problem()
    start = np.arange(n) % min(130, maxK) + 1                     # 130 round-robin clusters, clipped to the cap
    init = np.stack([start, start, start])
    got = _lib.vi_search(S, init, order, maxK=maxK)
    refs = [V.vi_search_ref(S, library_table(n), init[r], order[r], maxK=maxK) for r in range(3)]
    assert_equals_reference(got, refs, ("cap", maxK))
    assert (got["K"] <= maxK).all()


# (n, m, K, maxK): the paths the kernel takes besides those of SHAPES.  The next point's labels are staged in LDS through one
# register (m <= 1024), four (m <= 4096) or read in place (beyond); a table row is covered by Kcap4/4 threads, which leaves
# R = 1024 // (Kcap4/4) rows per pass, and a thread's samples r, r + R, ... go four at a time while m > 3R, then singly.
PATHS = {"m1500-four-registers": (9, 1500, 3, 0), "m3500-four-registers-unrolled": (9, 3500, 3, 0),
         "m4100-in-place-unrolled": (9, 4100, 3, 0), "m60-K300-unrolled-singletons": (300, 60, 5, 300),
         "K1024-four-rows-per-pass": (1100, 5, 4, 1024)}


@pytest.mark.parametrize("case", list(PATHS))
def test_every_path_equals_the_reference(case):
    n, m, K, maxK = PATHS[case]
    S, _ = R.planted_counts(n, m, K, 0.25, seed=7 + n + m)
    rng = np.random.default_rng(n + m)
    order = np.stack([rng.permutation(n) + 1, rng.permutation(n) + 1]).astype(np.int32)
    cap = maxK if maxK else V.relabel(S)[1]
    init = np.stack([np.zeros(n, np.int64), np.arange(n) % min(cap, n) + 1])       # empty; round-robin over every slot
    got = _lib.vi_search(S, init, order, maxK=maxK)
    refs = [V.vi_search_ref(S, library_table(n), init[r], order[r], maxK=maxK) for r in range(2)]
    assert_equals_reference(got, refs, case)
    assert abs(got["loss"][0] - rc.expectedvi(got["labels"][0], S)) <= LOSS_TOL


def test_returned_loss_is_the_expected_vi():
    for shape in (SHAPES[4], SHAPES[5]):
        S, init, order = problem(shape)
        got = _lib.vi_search(S, run_inits(shape, 0), order)
        for r in range(3):
            err = abs(got["loss"][r] - rc.expectedvi(got["labels"][r], S))
            print(shape, r, "loss", got["loss"][r], "err", err)
            assert err <= LOSS_TOL
        G = library_table(shape[0])
        assert got["loss"][0] == (int(got["loss_num"][0]) + V.constant(V.relabel(S)[0], G)) / (2.0 ** 32 * shape[0] * shape[1])


def test_two_identical_calls_return_identical_bytes():
    shape = SHAPES[5]
    S, _, order = problem(shape)
    init = run_inits(shape, 0)
    a = _lib.vi_search(S, init, order)
    b = _lib.vi_search(S, init, order)
    for k in ("labels", "loss", "loss_num", "sweeps", "converged", "moves", "K"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best"] == b["best"]


class _Samples:
    def __init__(self, clusts):
        self.clusts = list(clusts)


def test_searchpointestimate_exact_is_never_worse_than_its_starts():
    n, m, nruns = 257, 50, 4
    S, _ = R.planted_counts(n, m, 16, 0.2, seed=11)
    samples = _Samples(S)
    extra = np.random.default_rng(3).integers(1, 4, n)
    clust, info = rc.searchpointestimate(samples, "VI", nruns=nruns, seed=3, exact=True, init=[extra])
    mpel = rc.getpointestimate(samples, "MPEL", "VI")[0]
    lower, _ = rc.searchpointestimate(samples, "VI", nruns=nruns, seed=3, init=[extra])
    best = info["loss"][info["best"]]
    print("exact search", best, "MPEL sample", rc.expectedvi(mpel, S), "lower-bound result", rc.expectedvi(lower, S))
    assert len(info["loss"]) == len(info["labels"]) == nruns + 2 + 1
    assert info["best"] == int(np.argmin(info["loss_num"])) and np.array_equal(clust, info["labels"][info["best"]])
    # info["loss"] is the library's fixed-point value, within 2·2^-32 of expectedvi's f64 sum (LOSS_TOL, module docstring):
    # the f64 comparisons carry that slack; the exact statement is the one in the integer criterion below
    assert best <= rc.expectedvi(mpel, S) + LOSS_TOL
    assert best <= rc.expectedvi(lower, S) + LOSS_TOL
    assert abs(best - rc.expectedvi(clust, S)) <= LOSS_TOL
    G = library_table(n)
    qbest = int(info["loss_num"][info["best"]])
    assert qbest == V.q_direct(clust, S, G) and qbest <= V.q_direct(mpel, S, G) and qbest <= V.q_direct(lower, S, G)
    # the default orders are the documented Philox permutations: the same runs through the low-level entry
    rng = np.random.Generator(np.random.Philox(key=3))
    order = np.stack([rng.permutation(n).astype(np.int32) + 1 for _ in range(nruns)])
    low = _lib.vi_search(S, np.zeros((nruns, n), np.int64), order)
    assert np.array_equal(low["labels"], info["labels"][:nruns])
    assert np.array_equal(low["loss_num"], info["loss_num"][:nruns])


def test_errors_return_their_codes_and_the_process_goes_on():
    L = _lib.lib()
    n, m = 8, 3
    S, _ = R.planted_counts(n, m, 2, 0.2, seed=1)
    init = np.zeros((1, n), np.int64)
    order = np.arange(1, n + 1, dtype=np.int32)[None, :].copy()
    labels = np.zeros((1, n), np.int64)
    runs = (_lib.RcPsmRun * 1)()
    best = C_.c_int32()

    def call(samples=S, m_=m, n_=n, nruns=1, init_=init, order_=order, maxK=0, maxsweeps=5, labels_=labels, runs_=runs, best_=best):
        p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x)
        rc_ = L.rc_vi_search(0, p(samples), m_, n_, nruns, p(init_), p(order_), maxK, maxsweeps, p(labels_), runs_,
                             None if best_ is None else C_.byref(best_), None)
        return rc_, L.rc_last_error(None).decode()

    ARG, CAP = -1, -6
    zero_sample = S.copy(); zero_sample[1, 2] = 0
    big_sample = S.copy(); big_sample[2, 0] = n + 1
    bad_label = init.copy(); bad_label[0, 3] = n + 1
    neg_label = init.copy(); neg_label[0, 3] = -1
    not_perm = order.copy(); not_perm[0, 0] = 2
    zero_order = order.copy(); zero_order[0, 0] = 0
    three = np.array([[5, 2, 7, 0, 0, 0, 0, 0]], np.int64)
    lmax = V.relabel(S)[1]
    assert lmax == 2
    cases = [("NULL samples", dict(samples=None)), ("NULL init", dict(init_=None)), ("NULL order", dict(order_=None)),
             ("NULL labels", dict(labels_=None)), ("NULL runs", dict(runs_=None)), ("NULL best", dict(best_=None)),
             ("m < 1", dict(m_=0)), ("n < 1", dict(n_=0)), ("nruns < 1", dict(nruns=0)), ("maxsweeps < 1", dict(maxsweeps=0)),
             ("maxK < 0", dict(maxK=-1)), ("sample label 0", dict(samples=zero_sample)), ("sample label above n", dict(samples=big_sample)),
             ("label above n", dict(init_=bad_label)), ("negative label", dict(init_=neg_label)),
             ("repeated order entry", dict(order_=not_perm)), ("order entry 0", dict(order_=zero_order)),
             ("init beyond maxK", dict(init_=three, maxK=2)), ("init beyond the samples' cluster count", dict(init_=three))]
    for what, kw in cases:
        code, msg = call(**kw)
        assert code == ARG and msg, (what, code, msg)
    # capacity: checked before the samples are read, so the small buffers do
    code, msg = call(n_=8193)
    assert code == CAP and "8192" in msg
    code, msg = call(n_=n, m_=2 ** 26 // n + 1)                       # m·n = 2^26 + n
    assert code == CAP and "2^26" in msg
    assert L.rc_vi_gtable(0, labels.ctypes.data) == ARG and L.rc_vi_gtable(4, None) == ARG
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.vi_search(zero_sample, init, order)
    # rc_psm_search still knows two losses only
    counts = rc.cocluster_counts(list(S))
    assert L.rc_psm_search(0, counts.ctypes.data, m, n, 2, 1, init.ctypes.data, order.ctypes.data, 0, 5, labels.ctypes.data, runs,
                           C_.byref(best), None) == ARG
    # and a valid call afterwards
    code, msg = call()
    ref = V.vi_search_ref(S, library_table(n), init[0], order[0], maxsweeps=5)
    assert code == 0 and np.array_equal(labels[0], ref["labels"]) and runs[0].loss_num == ref["loss_num"] and best.value == 0
    assert (runs[0].sweeps, runs[0].moves, runs[0].K, bool(runs[0].converged)) == (ref["sweeps"], ref["moves"], ref["K"], ref["converged"])
