"""The PEAR search on the GPU (csrc/pointsearch.inc.hip through rc_pear_search, _ctx, _samples and searchmaxpear / maxpear).
A run is an exact integer function of its inputs, so every run is held to tests/pear_search_ref.py bit for bit: labels,
sweeps, moves, converged, K, num, den, and the choice of best.

Shapes: n = 1, 2, 3; the wave edge 64 / 65; 257; and 1025, 2049, 4097 — one past the 1, 2 and 4 row registers per thread,
so the three wider template instances of the kernel run.  Planted K <= 8, m <= 20.  Runs per shape: a random order from empty
labels, the identity order from one cluster, the reverse order from labels of which half are unallocated."""
import ctypes as C_
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

import np_transcription as T
import pear_search_ref as R
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1, 0.0), (2, 3, 2, 0.0), (3, 4, 2, 0.3), (64, 7, 4, 0.1), (65, 20, 5, 0.2), (257, 20, 8, 0.2),
          (1025, 9, 8, 0.2), (2049, 12, 6, 0.15), (4097, 10, 5, 0.1)]
IDS = [f"n{s[0]}" for s in SHAPES]
FIELDS = ("sweeps", "moves", "converged", "K", "num", "den")


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(samples, counts, init 3×n, order 3×n) of a shape; computed once and shared (never modified)."""
    n, m, K, noise = shape
    S, C = R.planted_counts(n, m, K, noise, seed=2000 + n)
    rng = np.random.default_rng(n)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]).astype(np.int32)
    mixed = rng.integers(1, min(K, n) + 1, n)
    mixed[rng.permutation(n)[: n // 2]] = 0
    init = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), mixed.astype(np.int64)])
    for a in (S, C, init, order):
        a.setflags(write=False)
    return S, C, init, order


@functools.lru_cache(maxsize=None)
def reference(shape):
    _, C, init, order = problem(shape)
    return [R.pear_search_ref(C, shape[1], init[r], order[r]) for r in range(3)]


def assert_equal_runs(got, refs, what=""):
    for r, ref in enumerate(refs):
        print(what, r, {k: int(got[k][r]) for k in FIELDS}, "pear", got["pear"][r])
        assert np.array_equal(got["labels"][r], ref["labels"]), (what, r)
        for k in FIELDS:
            assert got[k][r] == ref[k], (what, r, k, got[k][r], ref[k])
        assert got["pear"][r] == float(ref["num"]) / float(ref["den"])             # the library divides the two as doubles
    assert got["best"] == R.best_run(refs), what


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_runs_equal_the_reference_bit_for_bit(shape):
    _, C, init, order = problem(shape)
    got = _lib.pear_search(C, shape[1], init, order)
    assert_equal_runs(got, reference(shape), shape)
    assert got["converged"].all()


@pytest.mark.parametrize("maxK,maxsweeps", [(2, 100), (0, 1)], ids=["maxK2", "onesweep"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4], SHAPES[5], SHAPES[6]], ids=["n3", "n65", "n257", "n1025"])
def test_maxk_and_maxsweeps(shape, maxK, maxsweeps):
    n, m = shape[0], shape[1]
    _, C, init, order = problem(shape)
    if maxK:
        init = np.where(init > maxK, maxK, init)
    got = _lib.pear_search(C, m, init, order, maxK=maxK, maxsweeps=maxsweeps)
    refs = [R.pear_search_ref(C, m, init[r], order[r], maxK=maxK, maxsweeps=maxsweeps) for r in range(3)]
    assert_equal_runs(got, refs, (shape, maxK, maxsweeps))
    if maxK:
        assert (got["K"] <= maxK).all() and (n < 65 or (got["K"] == maxK).all())   # planted K >= 5: the cap is reached
    else:
        assert (got["sweeps"] == 1).all() and not got["converged"][0]             # a run from empty labels moves every point


def tie_cases():
    n = 65
    out = {}
    for m in (2, 3):
        out[f"m{m}"] = (R.planted_counts(n, m, 4, 0.3, seed=50 + m)[1], m)
    flat = np.full((33, 33), 2, np.uint32)
    np.fill_diagonal(flat, 4)
    out["equal_offdiagonal"] = (flat, 4)
    truth = np.random.default_rng(7).integers(1, 6, n)
    out["identical_samples"] = ((6 * (truth[:, None] == truth[None, :])).astype(np.uint32), 6)
    return out


@pytest.mark.parametrize("case", ["m2", "m3", "equal_offdiagonal", "identical_samples"])
def test_tie_heavy_inputs(case):
    C, m = tie_cases()[case]
    n = len(C)
    rng = np.random.default_rng(n + m)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1), rng.permutation(n) + 1]).astype(np.int32)
    init = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), np.arange(1, n + 1), rng.integers(0, 4, n)])
    got = _lib.pear_search(C, m, init, order)
    refs = [R.pear_search_ref(C, m, init[r], order[r]) for r in range(4)]
    assert_equal_runs(got, refs, case)
    if case == "identical_samples":
        assert got["num"][0] == got["den"][0] and got["pear"][0] == 1.0


def test_windowed_passes_give_the_same_runs():
    """RC_PSM_WINDOW=5 at n = 65 covers the occupied slots in passes of 5: the runs start with 9 and with 65 occupied slots."""
    n, m = 65, 20
    _, C = R.planted_counts(n, m, 5, 0.2, seed=3)
    init = np.stack([np.arange(n) % 9 + 1, np.arange(1, n + 1), np.zeros(n, np.int64)])
    order = np.stack([np.arange(1, n + 1), np.arange(n, 0, -1), np.random.default_rng(0).permutation(n) + 1]).astype(np.int32)
    old = os.environ.get("RC_PSM_WINDOW")
    try:
        os.environ["RC_PSM_WINDOW"] = "5"                           # read by the library at every call
        got = _lib.pear_search(C, m, init, order)
    finally:
        if old is None:
            os.environ.pop("RC_PSM_WINDOW", None)
        else:
            os.environ["RC_PSM_WINDOW"] = old
    assert_equal_runs(got, [R.pear_search_ref(C, m, init[r], order[r]) for r in range(3)], "window 5")
    plain = _lib.pear_search(C, m, init, order)
    for k in FIELDS + ("labels", "pear"):
        assert plain[k].tobytes() == got[k].tobytes(), k


def test_samples_entry_equals_the_counts_entry():
    shape = SHAPES[5]
    S, C, init, order = problem(shape)
    counts = _lib.samples_counts(S)[0]
    assert np.array_equal(counts, C)
    a = _lib.pear_search_samples(S, init, order)
    b = _lib.pear_search(counts, shape[1], init, order)
    for k in FIELDS + ("labels", "pear"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best"] == b["best"] and a["counts_ms"] >= 0.0
    assert_equal_runs(a, reference(shape), "samples")


def _context_with_samples(n=100, nsamples=5):
    d = rc.generatemixture(n, 4, alpha=10, sigma=0.25, dim=4, seed=5)
    D = d["distancematrix"]
    ctx = rc.Context(D)
    ctx.set_params(**rc.likelihood_hyperparams(D, d["clusts"]))
    ctx.set_state(np.random.default_rng(1).integers(1, 7, n).astype(np.int64))
    recorded = []
    for t in range(nsamples):
        ctx.gibbs_sweep(1.0, 0.5, seed=9, sweep_index=t)
        recorded.append(ctx.record_sample())
    return ctx, recorded


def test_context_form_equals_the_host_form_and_leaves_the_chain_alone():
    n, m = 100, 5
    ctx, recorded = _context_with_samples(n, m)
    twin, _ = _context_with_samples(n, m)
    counts = ctx.cocluster_counts()
    rng = np.random.default_rng(2)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]).astype(np.int32)
    init = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), recorded[0]])
    before, layout = ctx.get_state(), ctx.cocluster_device_buffer()
    a = _lib.pear_search(None, m, init, order, ctx=ctx)
    b = _lib.pear_search(counts, m, init, order)
    for k in FIELDS + ("labels", "pear"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best"] == b["best"]
    assert_equal_runs(a, [R.pear_search_ref(counts, m, init[r], order[r]) for r in range(3)], "ctx")
    clust, info = rc.searchmaxpear(nruns=2, numsamples=m, ctx=ctx)
    assert len(clust) == n and (int(info["num"][info["best"]]), int(info["den"][info["best"]])) == rc.pearfraction(clust, counts, m)
    after = ctx.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert ctx.cocluster_device_buffer() == layout and np.array_equal(ctx.cocluster_counts(), counts)
    ctx.gibbs_sweep(1.25, 0.4, seed=9, sweep_index=m)
    twin.gibbs_sweep(1.25, 0.4, seed=9, sweep_index=m)
    assert np.array_equal(ctx.get_state()[0], twin.get_state()[0]) and ctx.loglik() == twin.loglik()
    ctx.close(); twin.close()


def test_capacity_and_argument_errors_come_before_device_work():
    """All-zero inputs, nothing large allocated: the checks read m, n and the pointers only."""
    L = _lib.lib()
    buf = np.zeros(2 * 8193, np.int64)                                       # init, order, labels: never read
    runs = (_lib.RcPearRun * 2)()
    best = C_.c_int32()

    def call(m, n, nruns=1, maxK=0, maxsweeps=5, counts=buf, best_=best):
        code = L.rc_pear_search(0, counts.ctypes.data if counts is not None else None, m, n, nruns, buf.ctypes.data, buf.ctypes.data, maxK,
                                maxsweeps, buf.ctypes.data, runs, None if best_ is None else C_.byref(best_), None)
        return code, L.rc_last_error(None).decode()

    ARG, CAP = -1, -6
    code, msg = call(3, 8193)
    assert code == CAP and "8192" in msg
    T2 = (8192 * 8191 // 2) ** 2
    assert 4097 * T2 < 2 ** 62 <= 4098 * T2
    code, msg = call(4098, 8192)
    assert code == CAP and "T^2" in msg
    code, msg = call(2 ** 31 // 64, 64)                                       # m·n = 2^31
    assert code == CAP and "31 bits" in msg
    # the argument checks come first, in rc_psm_search's order
    for kw, text in ((dict(counts=None), "NULL argument"), (dict(best_=None), "NULL argument"), (dict(nruns=0), "nruns >= 1"),
                     (dict(maxsweeps=0), "maxsweeps >= 1"), (dict(maxK=-1), "maxK >= 0")):
        code, msg = call(3, 8193, **kw)
        assert code == ARG and text in msg and msg.startswith("rc_pear_search:"), (kw, code, msg)
    s_args = (0, buf.ctypes.data, 4098, 8192, 1, buf.ctypes.data, buf.ctypes.data, 0, 5, buf.ctypes.data, runs, C_.byref(best), None, None)
    assert L.rc_pear_search_samples(*s_args) == CAP and b"rc_pear_search_samples" in L.rc_last_error(None)
    assert L.rc_pear_search_ctx(None, 3, 1, buf.ctypes.data, buf.ctypes.data, 0, 5, buf.ctypes.data, runs, C_.byref(best), None) == ARG
    # the existing entry points keep their loss specifiers
    psm = (_lib.RcPsmRun * 1)()
    small = np.full((2, 2), 3, np.uint32)
    assert L.rc_psm_search(0, small.ctypes.data, 3, 2, 2, 1, buf.ctypes.data, buf.ctypes.data, 0, 5, buf.ctypes.data, psm, C_.byref(best), None) == ARG
    assert "invalid loss specifier 2" in L.rc_last_error(None).decode()
    # and a valid call afterwards
    got = _lib.pear_search(small, 3, np.zeros((1, 2), np.int64), np.array([[1, 2]], np.int32))
    assert got["labels"].tolist() == [[1, 1]] and (got["num"][0], got["den"][0]) == (0, 1)     # every sample one cluster: den = 0


class _Samples:
    def __init__(self, clusts):
        self.clusts = list(clusts)


@functools.lru_cache(maxsize=None)
def searched():
    S, C, _, _ = problem(SHAPES[5])
    return rc.searchmaxpear(_Samples(S), nruns=4, seed=3)


def test_searchmaxpear_is_never_below_its_starts_or_the_mpel_sample():
    n, m = SHAPES[5][0], SHAPES[5][1]
    S, C, _, _ = problem(SHAPES[5])
    samples = _Samples(S)
    clust, info = searched()
    best = Fraction(int(info["num"][info["best"]]), int(info["den"][info["best"]]))
    assert len(info["pear"]) == 6 and np.array_equal(clust, info["labels"][info["best"]])     # 4 orders, the best draw, the best cut
    assert best == Fraction(*rc.pearfraction(clust, C, m)) == max(Fraction(int(a), int(b)) for a, b in zip(info["num"], info["den"]))
    # the starts: the sample of highest PEAR and the average-linkage cut of highest PEAR
    draws = [Fraction(*rc.pearfraction(s, C, m)) for s in S]
    cut, cinfo = rc.maxpear(samples, "avg")
    print("search", float(best), "best draw", float(max(draws)), "best avg cut", cinfo["pear"], "K", info["K"], "sweeps", info["sweeps"])
    assert best >= max(draws) and best >= Fraction(cinfo["num"], cinfo["den"])
    assert Fraction(int(info["num"][4]), int(info["den"][4])) >= max(draws)
    assert Fraction(int(info["num"][5]), int(info["den"][5])) >= Fraction(cinfo["num"], cinfo["den"])
    mpel = rc.getpointestimate(samples, "MPEL", "omARI")[0]
    assert best >= Fraction(*rc.pearfraction(mpel, C, m))
    # the default orders are the documented Philox permutations: the same runs through the low-level entry
    rng = np.random.Generator(np.random.Philox(key=3))
    order = np.stack([rng.permutation(n).astype(np.int32) + 1 for _ in range(4)])
    low = _lib.pear_search(C, m, np.zeros((4, n), np.int64), order)
    assert np.array_equal(low["labels"], info["labels"][:4])
    # counts + numsamples, and an extra start through init=
    c2, i2 = rc.searchmaxpear(C, numsamples=m, nruns=4, seed=3, init=[S[0]])
    assert np.array_equal(i2["labels"][:4], info["labels"][:4]) and len(i2["pear"]) == 6
    assert Fraction(int(i2["num"][4]), int(i2["den"][4])) >= draws[0]


def test_maxpear_all_is_at_least_every_single_method():
    S, C, _, _ = problem(SHAPES[4])
    m = SHAPES[4][1]
    samples = _Samples(S)
    clust, info = rc.maxpear(samples, "all", nruns=2)
    top = Fraction(info["num"], info["den"])
    assert top == Fraction(*rc.pearfraction(clust, C, m)) and info["pear"] == info["num"] / info["den"]
    for method in ("avg", "comp", "draws", "search"):
        kw = dict(nruns=2) if method == "search" else {}
        c1, i1 = rc.maxpear(samples, method, **kw)
        one = Fraction(i1["num"], i1["den"])
        print(method, float(one), "all", float(top), info["method"])
        assert one == Fraction(*rc.pearfraction(c1, C, m)) and top >= one and i1["method"] == method
    # every cut's PEAR equals the host evaluation of the cut
    cuts = np.stack([_lib.hclust_cut(rc.hclust(samples, "average")["merges"], len(C), K) for K in range(1, len(info["avg"]["num"]) + 1)])
    for k, c in enumerate(cuts):
        assert (int(info["avg"]["num"][k]), int(info["avg"]["den"][k])) == rc.pearfraction(c, C, m)
    # the count-matrix form has no draws
    c3, i3 = rc.maxpear(C, "all", numsamples=m, nruns=2)
    assert "draws" not in i3 and Fraction(i3["num"], i3["den"]) == Fraction(*rc.pearfraction(c3, C, m))


def test_expectedpears_and_expectedari():
    S, C, _, _ = problem(SHAPES[4])
    n, m = SHAPES[4][0], SHAPES[4][1]
    labs = np.stack([S[0], S[3], np.ones(n, np.int64), np.arange(1, n + 1)])
    pear, num, den = rc.expectedpears(labs, C, m)
    p2, n2, d2 = rc.expectedpears(labs, _Samples(S))
    for k, c in enumerate(labs):
        assert (int(num[k]), int(den[k])) == (int(n2[k]), int(d2[k])) == rc.pearfraction(c, C, m) and pear[k] == p2[k] == rc.expectedpear(c, C, m)
    ari = rc.expectedari(labs, S)
    want = [np.mean([T.randindex(c, s)[0] for s in S]) for c in labs]
    print("expected ARI", ari, "PEAR", pear)
    assert np.allclose(ari, want, rtol=0, atol=1e-12)
