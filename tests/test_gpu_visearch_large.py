"""rc_vi_search_large / rc_vi_search_groups_large (csrc/visearch_large.inc.hip), n <= 32767: a run is integer arithmetic on the
library's table, so it equals tests/vi_search_ref.py bit for bit, and rc_vi_search's bytes where both kernels run.  Above 8192 one
planted cluster holds ~95 % of the points, so that table cells cross every threshold of the split table (the last at x = 22 026)."""
import ctypes as C_
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import psm_search_ref as R
import vi_search_ref as V
import redclust_amd as rc
from redclust_amd import _lib
from test_gpu_visearch import KEYS, library_table

pytestmark = pytest.mark.gpu
ARRAYS = ("labels", "loss", "best") + KEYS


@functools.lru_cache(maxsize=None)
def problem(n, m=7):
    """(samples, init 3×n, order 3×n): empty labels in a shuffled order, a sample, all points in one slot"""
    S, _ = R.planted_counts(n, m, min(4, n), 0.15, seed=3000 + n)
    init = np.stack([np.zeros(n, np.int64), S[0], np.ones(n, np.int64)])
    order = np.stack([np.random.default_rng(n).permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]).astype(np.int32)
    return S, init, order


@functools.lru_cache(maxsize=None)
def skewed(n, m=3):
    """~95 % of the points in cluster 1, the rest in 2..5; 2 % of the labels redrawn per sample"""
    rng = np.random.default_rng(n)
    base = np.where(rng.random(n) < 0.95, 1, rng.integers(2, 6, n))
    S = np.tile(base, (m, 1)).astype(np.int64)
    for s in range(m):
        at = rng.permutation(n)[: n // 50]
        S[s, at] = rng.integers(1, 6, len(at))
    return S


def assert_runs(got, refs):
    for r, ref in enumerate(refs):
        assert np.array_equal(got["labels"][r], ref["labels"]) and all(got[k][r] == ref[k] for k in KEYS), (r, got, ref)


@pytest.mark.parametrize("n,maxK,maxsweeps", [(1, 0, 100), (2, 0, 100), (5, 0, 100), (63, 0, 100), (257, 0, 100), (1027, 0, 100),
                                              (257, 2, 100), (257, 0, 1)])
def test_equals_the_reference_bit_for_bit(n, maxK, maxsweeps):
    S, init, order = problem(n)
    init = np.where(init > maxK, maxK, init) if maxK else init
    got = _lib.vi_search_large(S, init, order, maxK=maxK, maxsweeps=maxsweeps)
    refs = [V.vi_search_ref(S, library_table(n), init[r], order[r], maxK=maxK, maxsweeps=maxsweeps) for r in range(3)]
    assert_runs(got, refs)
    assert got["best"] == int(np.argmin([ref["loss_num"] for ref in refs]))


@pytest.mark.parametrize("n", [5, 257, 1027, 4099])
def test_equals_the_old_kernel_byte_for_byte(n):
    S, init, order = problem(n)
    new, old = _lib.vi_search_large(S, init, order), _lib.vi_search(S, init, order)
    for k in ARRAYS:
        assert np.array_equal(new[k], old[k]), k


@pytest.mark.parametrize("n,largest", [(8195, 7000), (24001, 22026)])
def test_above_the_old_capacity_with_every_high_word(n, largest):
    S = skewed(n)
    init = np.stack([np.zeros(n, np.int64), S[0]])
    order = np.tile(np.arange(1, n + 1, dtype=np.int32), (2, 1))
    got = _lib.vi_search_large(S, init, order, maxsweeps=1)
    assert np.bincount(got["labels"][0]).max() > largest and np.bincount(got["labels"][1]).max() > largest
    assert_runs(got, [V.vi_search_ref(S, library_table(n), init[r], order[r], maxsweeps=1) for r in range(2)])


@pytest.mark.parametrize("n", [257, 8195])
def test_grouped_runs_equal_the_reference_on_their_groups(n):
    S = np.concatenate([problem(n)[0], problem(n, 5)[0]]) if n < 8192 else np.concatenate([skewed(n, 3), skewed(n, 4)[::-1]])
    m = len(S)
    group = np.repeat(np.arange(3, dtype=np.int32), [m // 6, m // 3, m - m // 6 - m // 3])   # 2, 4, 6 or 1, 2, 4 samples
    run_group = np.array([2, 0, 1, 0], np.int32)
    init = np.stack([np.zeros(n, np.int64), S[0], np.zeros(n, np.int64), np.ones(n, np.int64)])
    order = np.tile(np.arange(1, n + 1, dtype=np.int32), (4, 1))
    sweeps = 100 if n < 8192 else 1
    got = _lib.vi_search_groups_large(S, group, init, order, run_group, maxsweeps=sweeps)
    assert_runs(got, [V.vi_search_ref(S[group == run_group[r]], library_table(n), init[r], order[r], maxsweeps=sweeps) for r in range(4)])
    if n < 8192:
        old = _lib.vi_search_groups(S, group, init, order, run_group, maxsweeps=sweeps)
        for k in ARRAYS:
            assert np.array_equal(got[k], old[k]), k


def test_capacity_is_refused_before_any_device_work():
    L = _lib.lib()
    n = 1030; S = np.arange(1, n + 1, dtype=np.int64)[None, :].copy()
    init, labels, order = np.zeros((1, n), np.int64), np.zeros((1, n), np.int64), np.arange(1, n + 1, dtype=np.int32)[None, :].copy()
    group, run_group, runs, best = np.zeros(2 ** 23 + 1, np.int32), np.zeros(1, np.int32), (_lib.RcPsmRun * 1)(), C_.c_int32()
    p = lambda x: x.ctypes.data

    def call(grouped, m_=1, n_=n, maxK=0):                             # device 99 does not exist: reaching it would be RC_ERR_ARG
        head = (99, p(S), m_, n_) + ((p(group), 1) if grouped else ())
        tail = (1,) + ((p(run_group),) if grouped else ()) + (p(init), p(order), maxK, 5, p(labels), runs, C_.byref(best), None)
        code = (L.rc_vi_search_groups_large if grouped else L.rc_vi_search_large)(*head, *tail)
        return code, L.rc_last_error(None).decode()
    for grouped in (False, True):
        code, msg = call(grouped, n_=32768)                            # before the samples are read, so the small buffers do
        assert code == -6 and "32767" in msg, msg
        code, msg = call(grouped, n_=8, m_=len(group))                 # m·n = 2^26 + 8 (the grouped entry reads the m group ids first)
        assert code == -6 and "2^26" in msg, msg
        code, msg = call(grouped, maxK=1025)
        assert code == -6 and "1024" in msg, msg


def test_searchvi_runs_the_documented_starts():
    n, kw = 8195, dict(nruns=1, seed=3, maxsweeps=2)
    S = skewed(n); mc = SimpleNamespace(clusts=S)
    lower, _ = rc.searchpointestimate(mc, "VI", **kw)
    mpel = np.asarray(rc.getpointestimate(mc, "MPEL", "VI")[0])
    ident = np.arange(1, n + 1, dtype=np.int32)
    order = np.stack([np.random.Generator(np.random.Philox(key=3)).permutation(n).astype(np.int32) + 1, ident, ident])
    need, lmax = max(len(np.unique(mpel)), len(np.unique(lower))), max(len(np.unique(s)) for s in S)
    low = _lib.vi_search_large(S, np.stack([np.zeros(n, np.int64), mpel, lower]), order, maxK=need if need > lmax else 0, maxsweeps=2)
    clust, info = rc.searchvi(S, **kw)
    assert np.array_equal(clust, low["labels"][low["best"]]) and np.array_equal(info["loss_num"], low["loss_num"])
    small = SimpleNamespace(clusts=problem(100)[0])
    a, b = rc.searchvi(small, nruns=2, seed=1), rc.searchpointestimate(small, "VI", exact=True, nruns=2, seed=1)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in ARRAYS)


def test_wasabi_above_the_old_capacity_and_unchanged_below():
    n = 8195
    S = np.concatenate([skewed(n, 4), (skewed(n + 1, 4)[:, :n] + np.arange(n) % 2 * 5)])       # two modes, m = 8
    res = rc.wasabi(S, 2, nstarts=1, maxiter=2, maxsweeps=1, nruns=0)
    num = rc.partitiondistances(res.particles, S, "VI")[1]["num"]
    assert res.objective_num == int(num[res.assignment, np.arange(8)].sum()) and len(res.expectedvi()) == 2
    n = 300                                # one Lloyd step by hand through rc_vi_search_groups, the path of every n <= 8192
    S = np.concatenate([problem(n)[0], problem(n, 6)[0]])
    P0 = np.stack([S[0], S[-1]])
    res = rc.wasabi(S, 2, nstarts=0, init=P0, maxiter=1, nruns=1, seed=5)
    assign = np.argmin(rc.partitiondistances(P0, S, "VI")[1]["num"], axis=0).astype(np.int32)
    ident = np.arange(1, n + 1, dtype=np.int32)
    perm = np.random.Generator(np.random.Philox(key=5)).permutation(n).astype(np.int32) + 1
    cap = max(len(np.unique(r)) for r in S)
    hand = _lib.vi_search_groups(S, assign, np.stack([P0[0], np.zeros(n, np.int64), P0[1], np.zeros(n, np.int64)]),
                                 np.stack([ident, perm, ident, perm]), np.array([0, 0, 1, 1], np.int32), maxK=cap)
    want = sorted(tuple(hand["labels"][b]) for b in hand["best"])
    assert sorted(tuple(p) for p in res.particles) == want
