"""The exact expected-ID search on the GPU (k_visearch<PQ, LOSS_ID> of csrc/visearch.inc.hip through rc_id_search and
searchpointestimate(loss="ID")).  A run is integer arithmetic on the table Gq, so the device is held to tests/id_search_ref.py
bit for bit, the reference being handed the library's own table (test_gpu_visearch.py checks that table against NumPy's).

Shapes, starts and orders are test_gpu_visearch.py's (imported, so they are the same arrays).  The returned loss is
Q_ID/(2^32·n·m): the table's rounding contributes at most 2^-32 ≈ 2.3e-10 (Φq(x) is within x/2 units, the three sums of n
points each within n/2, max is 1-Lipschitz: m·n units in all), the f64 sums of expectedid far less — LOSS_TOL = 1e-9, as
there."""
import ctypes as C_
import functools
import os

import numpy as np
import pytest

import psm_search_ref as R
import vi_search_ref as V
import id_search_ref as I
import test_gpu_visearch as TV
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES, IDS, LOSS_TOL, KEYS = TV.SHAPES, TV.IDS, TV.LOSS_TOL, TV.KEYS
library_table = TV.library_table


@functools.lru_cache(maxsize=None)
def reference(shape, maxK, maxsweeps):
    S, _, order = TV.problem(shape)
    init = TV.run_inits(shape, maxK)
    return [I.id_search_ref(S, library_table(shape[0]), init[r], order[r], maxK=maxK, maxsweeps=maxsweeps) for r in range(3)]


def assert_equals_reference(got, refs, what):
    for r, ref in enumerate(refs):
        print(what, r, "sweeps", got["sweeps"][r], "moves", got["moves"][r], "K", got["K"][r], "Q", got["loss_num"][r],
              "ref: below", ref["below"], "above", ref["above"], "equal", ref["equal"])
        assert np.array_equal(got["labels"][r], ref["labels"]), (what, r)
        for k in KEYS:
            assert got[k][r] == ref[k], (what, r, k, got[k][r], ref[k])
    assert got["best"] == int(np.argmin([ref["loss_num"] for ref in refs]))


@pytest.mark.parametrize("maxK,maxsweeps", [(0, 100), (2, 100), (0, 1), (2, 1)], ids=["free", "maxK2", "onesweep", "maxK2-onesweep"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_search_equals_the_reference_bit_for_bit(shape, maxK, maxsweeps):
    n = shape[0]
    S, _, order = TV.problem(shape)
    init = TV.run_inits(shape, maxK)
    refs = reference(shape, maxK, maxsweeps)
    if n >= 63 and maxK == 0 and maxsweeps == 100:
        # the input condition: candidates on both sides of the max, or one branch of F would go untested
        assert sum(r["below"] for r in refs) > 0 and sum(r["above"] for r in refs) > 0, [(r["below"], r["above"]) for r in refs]
    got = _lib.id_search(S, init, order, maxK=maxK, maxsweeps=maxsweeps)
    assert_equals_reference(got, refs, shape)
    for r in range(3):
        if maxK:
            assert got["K"][r] <= maxK
        if maxsweeps == 1 and n > 1:
            assert got["sweeps"][r] == 1
    if maxsweeps == 1 and n > 2:
        assert not got["converged"][0]              # a run from empty labels moves every point in its first sweep


def test_the_id_search_is_not_the_vi_search():
    """input condition (references only): at some shape the ID run ends in other labels than the VI run from the same start,
    so a kernel that minimised the expected VI instead would fail the test above"""
    differ = []
    for shape in (SHAPES[5], SHAPES[6]):
        vi = TV.reference(shape, 0, 100)
        differ += [not np.array_equal(a["labels"], b["labels"]) for a, b in zip(reference(shape, 0, 100), vi)]
    assert any(differ), differ


@functools.lru_cache(maxsize=None)
def edge_problem(m):
    """n = 65 with m samples around the powers of two the search for p(x) steps through; m = 8: eight copies of ONE sample,
    so Bs is all ties and, once the run has found that sample, Aq meets every Bq_s exactly"""
    n = 65
    S, _ = R.planted_counts(n, max(m, 2), 5, 0.2, seed=300 + m)
    S = S[:m].copy()
    if m == 8:
        S[:] = S[0]
    rng = np.random.default_rng(m)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]).astype(np.int32)
    init = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), np.arange(n) % 3 + 1])
    for a in (S, init, order):
        a.setflags(write=False)
    return S, init, order


@pytest.mark.parametrize("m", [1, 2, 8, 63, 64, 65])
def test_sample_counts_at_the_edges_of_the_table_search(m):
    n = 65
    S, init, order = edge_problem(m)
    refs = [I.id_search_ref(S, library_table(n), init[r], order[r]) for r in range(3)]
    if m == 8:
        assert sum(r["equal"] for r in refs) > 0                                   # Aq meets Bq_s exactly
        assert any(np.array_equal(r["labels"], R.sortlabels(S[0])) and r["loss_num"] == 0 for r in refs)
    got = _lib.id_search(S, init, order)
    assert_equals_reference(got, refs, ("edge", m))


@pytest.mark.parametrize("maxK", [63, 64, 65, 130])
def test_slot_cap_at_the_lane_edges(maxK):
    """test_gpu_visearch.py's cap problem: n = 300, one sample of 70 clusters beside samples of 5 — widely spread Bq_s"""
    n = 300
    S, order = TV.cap_problem()
    start = np.arange(n) % min(130, maxK) + 1                     # 130 round-robin clusters, clipped to the cap
    init = np.stack([start, start, start])
    got = _lib.id_search(S, init, order, maxK=maxK)
    refs = [I.id_search_ref(S, library_table(n), init[r], order[r], maxK=maxK) for r in range(3)]
    assert_equals_reference(got, refs, ("cap", maxK))
    assert (got["K"] <= maxK).all()


def paths_problem(case):
    n, m, K, maxK = TV.PATHS[case]
    S, _ = R.planted_counts(n, m, K, 0.25, seed=7 + n + m)
    rng = np.random.default_rng(n + m)
    order = np.stack([rng.permutation(n) + 1, rng.permutation(n) + 1]).astype(np.int32)
    cap = maxK if maxK else V.relabel(S)[1]
    init = np.stack([np.zeros(n, np.int64), np.arange(n) % min(cap, n) + 1])       # empty; round-robin over every slot
    return S, init, order, maxK


@pytest.mark.parametrize("case", list(TV.PATHS))
def test_every_path_equals_the_reference(case):
    """test_gpu_visearch.py's PATHS — PQ = 4 (m = 1500, 3500), PQ = 0 (m = 4100), PQ = 1 with 300 and 1024 slots — each with
    F's table in LDS (n is small enough in all of them)"""
    n = TV.PATHS[case][0]
    S, init, order, maxK = paths_problem(case)
    got = _lib.id_search(S, init, order, maxK=maxK)
    refs = [I.id_search_ref(S, library_table(n), init[r], order[r], maxK=maxK) for r in range(2)]
    assert_equals_reference(got, refs, case)
    assert abs(got["loss"][0] - rc.expectedid(got["labels"][0], S)) <= LOSS_TOL


def _many_samples(n, m, seed):
    rng = np.random.default_rng(seed)
    truth = rng.integers(1, 4, n)
    S = np.tile(truth, (m, 1)).astype(np.int64)
    flip = rng.random((m, n)) < 0.25
    S[flip] = rng.integers(1, 4, int(flip.sum()))
    return S


@pytest.mark.parametrize("m,where", [(10100, "LDS"), (10200, "global")])
def test_table_at_the_lds_limit_and_beyond(m, where):
    """n = 100 with three slots: the VI state takes 1 520 B of LDS (816 Gq + 32 acc + 448 partials + 16 sz + 208 lab, no label
    staging at PQ = 0), so 16·(m + 1) more fit the 163 840 B up to m = 10 144: m = 10 100 launches with 163 136 B of LDS,
    m = 10 200 reads the table from global memory without being told to"""
    n = 100
    S = _many_samples(n, m, seed=m)
    assert V.relabel(S)[1] == 3
    assert (1520 + 16 * (m + 1) <= 160 * 1024) == (where == "LDS")
    rng = np.random.default_rng(m)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1)]).astype(np.int32)
    init = np.stack([np.zeros(n, np.int64), np.arange(n) % 3 + 1])
    got = _lib.id_search(S, init, order, maxsweeps=2)
    refs = [I.id_search_ref(S, library_table(n), init[r], order[r], maxsweeps=2) for r in range(2)]
    assert refs[0]["below"] > 0 and refs[0]["above"] > 0
    assert_equals_reference(got, refs, (m, where))


def test_table_forced_into_global_memory_returns_the_same_bytes():
    def run(which):
        if which < 2:
            shape = SHAPES[4 + which]                                              # n = 65, m = 50 and n = 257, m = 17
            S, _, order = TV.problem(shape)
            return _lib.id_search(S, TV.run_inits(shape, 0), order), reference(shape, 0, 100)
        S, init, order, maxK = paths_problem("m4100-in-place-unrolled")
        return _lib.id_search(S, init, order, maxK=maxK), None

    old = os.environ.get("RC_ID_TABLE_GLOBAL")
    os.environ.pop("RC_ID_TABLE_GLOBAL", None)
    try:
        plain = [run(w) for w in range(3)]
        os.environ["RC_ID_TABLE_GLOBAL"] = "1"                                     # read by the library at every call
        forced = [run(w) for w in range(3)]
    finally:
        if old is None:
            os.environ.pop("RC_ID_TABLE_GLOBAL", None)
        else:
            os.environ["RC_ID_TABLE_GLOBAL"] = old
    for (a, refs), (b, _) in zip(plain, forced):
        for k in ("labels", "loss", "loss_num", "sweeps", "converged", "moves", "K"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["best"] == b["best"]
        if refs is not None:
            assert_equals_reference(b, refs, "forced global")


def test_returned_loss_is_the_expected_id():
    for shape in (SHAPES[4], SHAPES[5]):
        n, m = shape[0], shape[1]
        S, init, order = TV.problem(shape)
        got = _lib.id_search(S, TV.run_inits(shape, 0), order)
        for r in range(3):
            err = abs(got["loss"][r] - rc.expectedid(got["labels"][r], S))
            print(shape, r, "loss", got["loss"][r], "err", err)
            assert err <= LOSS_TOL
            assert got["loss"][r] == int(got["loss_num"][r]) / (2.0 ** 32 * n * m)


def test_two_identical_calls_return_identical_bytes():
    shape = SHAPES[5]
    S, _, order = TV.problem(shape)
    init = TV.run_inits(shape, 0)
    a = _lib.id_search(S, init, order)
    b = _lib.id_search(S, init, order)
    for k in ("labels", "loss", "loss_num", "sweeps", "converged", "moves", "K"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best"] == b["best"]


class _Samples:
    def __init__(self, clusts):
        self.clusts = list(clusts)


def test_searchpointestimate_id_is_never_worse_than_its_starts():
    n, m, nruns = 257, 50, 4
    S, _ = R.planted_counts(n, m, 16, 0.2, seed=11)
    samples = _Samples(S)
    extra = np.random.default_rng(3).integers(1, 4, n)
    clust, info = rc.searchpointestimate(samples, "ID", nruns=nruns, seed=3, init=[extra])
    mpel = rc.getpointestimate(samples, "MPEL", "ID")[0]
    vi = info["vi"]["labels"][info["vi"]["best"]]
    best = info["loss"][info["best"]]
    print("ID search", best, "MPEL sample", rc.expectedid(mpel, S), "exact-VI result", rc.expectedid(vi, S))
    assert len(info["loss"]) == len(info["labels"]) == nruns + 1 + 2
    assert info["best"] == int(np.argmin(info["loss_num"])) and np.array_equal(clust, info["labels"][info["best"]])
    assert abs(best - rc.expectedid(clust, S)) <= LOSS_TOL
    G = library_table(n)
    qbest = int(info["loss_num"][info["best"]])
    assert qbest == I.q_direct(clust, S, G) and qbest <= I.q_direct(mpel, S, G) and qbest <= I.q_direct(vi, S, G)
    # info["vi"] is the exact-VI call with the same arguments
    again, _ = rc.searchpointestimate(samples, "VI", nruns=nruns, seed=3, exact=True, init=[extra])
    assert np.array_equal(again, vi)
    # exact may be either value, and the default orders are the documented Philox permutations
    clust2, info2 = rc.searchpointestimate(samples, "ID", nruns=nruns, seed=3, init=[extra], exact=True)
    assert np.array_equal(clust2, clust) and np.array_equal(info2["loss_num"], info["loss_num"])
    rng = np.random.Generator(np.random.Philox(key=3))
    order = np.stack([rng.permutation(n).astype(np.int32) + 1 for _ in range(nruns)])
    low = _lib.id_search(S, np.zeros((nruns, n), np.int64), order)
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
        rc_ = L.rc_id_search(0, p(samples), m_, n_, nruns, p(init_), p(order_), maxK, maxsweeps, p(labels_), runs_,
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
    assert V.relabel(S)[1] == 2
    cases = [("NULL samples", dict(samples=None)), ("NULL init", dict(init_=None)), ("NULL order", dict(order_=None)),
             ("NULL labels", dict(labels_=None)), ("NULL runs", dict(runs_=None)), ("NULL best", dict(best_=None)),
             ("m < 1", dict(m_=0)), ("n < 1", dict(n_=0)), ("nruns < 1", dict(nruns=0)), ("maxsweeps < 1", dict(maxsweeps=0)),
             ("maxK < 0", dict(maxK=-1)), ("sample label 0", dict(samples=zero_sample)), ("sample label above n", dict(samples=big_sample)),
             ("label above n", dict(init_=bad_label)), ("negative label", dict(init_=neg_label)),
             ("repeated order entry", dict(order_=not_perm)), ("order entry 0", dict(order_=zero_order)),
             ("init beyond maxK", dict(init_=three, maxK=2)), ("init beyond the samples' cluster count", dict(init_=three))]
    for what, kw in cases:
        code, msg = call(**kw)
        assert code == ARG and msg.startswith("rc_id_search"), (what, code, msg)
    # capacity: checked before the samples are read, so the small buffers do
    code, msg = call(n_=8193)
    assert code == CAP and "8192" in msg
    code, msg = call(n_=n, m_=2 ** 26 // n + 1)                       # m·n = 2^26 + n
    assert code == CAP and "2^26" in msg
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.id_search(zero_sample, init, order)
    # and a valid call afterwards
    code, msg = call()
    ref = I.id_search_ref(S, library_table(n), init[0], order[0], maxsweeps=5)
    assert code == 0 and np.array_equal(labels[0], ref["labels"]) and runs[0].loss_num == ref["loss_num"] and best.value == 0
    assert (runs[0].sweeps, runs[0].moves, runs[0].K, bool(runs[0].converged)) == (ref["sweeps"], ref["moves"], ref["K"], ref["converged"])
