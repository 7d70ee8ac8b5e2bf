"""rc_id_search_large (k_idlarge of csrc/visearch_large.inc.hip), n <= 32767: a run is integer arithmetic on the library's table, so it
equals tests/id_search_ref.py bit for bit and rc_id_search's bytes where both run, with F's table whole in LDS or behind its fence."""
import ctypes as C_
from types import SimpleNamespace

import numpy as np
import pytest

import id_search_ref as I
import redclust_amd as rc
from redclust_amd import _lib
from test_gpu_visearch import library_table
from test_gpu_visearch_large import ARRAYS, assert_runs, problem, skewed

pytestmark = pytest.mark.gpu


def references(S, init, order, **kw):
    return [I.id_search_ref(S, library_table(S.shape[1]), init[r], order[r], **kw) for r in range(len(init))]


def large_problem(n):                                                  # two runs in the identity order: empty labels, a sample
    S = skewed(n)
    return S, np.stack([np.zeros(n, np.int64), S[0]]), np.tile(np.arange(1, n + 1, dtype=np.int32), (2, 1))


@pytest.mark.parametrize("n,maxK,maxsweeps", [(1, 0, 100), (2, 0, 100), (5, 0, 100), (63, 0, 100), (257, 0, 100), (1027, 0, 100),
                                              (257, 2, 100), (257, 0, 1)])
def test_equals_the_reference_bit_for_bit(n, maxK, maxsweeps):
    S, init, order = problem(n)
    init = np.where(init > maxK, maxK, init) if maxK else init
    got = _lib.id_search_large(S, init, order, maxK=maxK, maxsweeps=maxsweeps)
    refs = references(S, init, order, maxK=maxK, maxsweeps=maxsweeps)
    assert_runs(got, refs)
    assert got["best"] == int(np.argmin([ref["loss_num"] for ref in refs]))


@pytest.mark.parametrize("n", [5, 257, 1027, 4099])
def test_equals_the_old_kernel_byte_for_byte(n):
    S, init, order = problem(n)
    new, old = _lib.id_search_large(S, init, order), _lib.id_search(S, init, order)
    for k in ARRAYS:
        assert np.array_equal(new[k], old[k]), k


@pytest.mark.parametrize("n,largest", [(8195, 7000), (24001, 22026)])
def test_above_the_old_capacity_with_every_high_word(n, largest):
    S, init, order = large_problem(n)
    got = _lib.id_search_large(S, init, order, maxsweeps=1)
    assert np.bincount(got["labels"][0]).max() > largest and np.bincount(got["labels"][1]).max() > largest
    assert_runs(got, references(S, init, order, maxsweeps=1))


@pytest.mark.parametrize("n,m", [(257, 7), (257, 1500), (8195, 3)])
def test_both_table_placements_return_the_same_bytes(n, m, monkeypatch):
    # forced fence: every 2nd Bq_s at m = 7 and 3, every 512th at m = 1500 (PQ = 4: two trips in LDS, nine in global memory)
    S, init, order = problem(n, m) if n < 8192 else large_problem(n)
    whole = _lib.id_search_large(S, init, order, maxsweeps=100 if n < 8192 else 1)
    monkeypatch.setenv("RC_ID_TABLE_GLOBAL", "1")                      # read by the library at every call
    fenced = _lib.id_search_large(S, init, order, maxsweeps=100 if n < 8192 else 1)
    for k in ARRAYS:
        assert np.array_equal(whole[k], fenced[k]), k
    if n == 257:
        assert_runs(fenced, references(S, init, order))


def test_capacity_is_refused_before_any_device_work():
    L = _lib.lib()
    n = 1030; S = np.arange(1, n + 1, dtype=np.int64)[None, :].copy()
    init, labels, order = np.zeros((1, n), np.int64), np.zeros((1, n), np.int64), np.arange(1, n + 1, dtype=np.int32)[None, :].copy()
    runs, best = (_lib.RcPsmRun * 1)(), C_.c_int32()
    p = lambda x: x.ctypes.data                # device 99 does not exist; refused before the samples are read, so the small buffers do
    for m_, n_, maxK, word in ((1, 32768, 0, "32767"), (2 ** 23 + 1, 8, 0, "2^26"), (1, n, 1025, "1024")):
        code = L.rc_id_search_large(99, p(S), m_, n_, 1, p(init), p(order), maxK, 5, p(labels), runs, C_.byref(best), None)
        assert code == -6 and word in L.rc_last_error(None).decode(), (word, L.rc_last_error(None).decode())


def test_searchid_runs_the_documented_starts():
    n, kw = 8195, dict(nruns=1, seed=3, maxsweeps=2)
    S = skewed(n); mc = SimpleNamespace(clusts=S)
    vi, _ = rc.searchvi(S, **kw)
    mpel = np.asarray(rc.getpointestimate(mc, "MPEL", "ID")[0])
    ident = np.arange(1, n + 1, dtype=np.int32)
    order = np.stack([np.random.Generator(np.random.Philox(key=3)).permutation(n).astype(np.int32) + 1, ident, ident])
    need, lmax = max(len(np.unique(mpel)), len(np.unique(vi))), max(len(np.unique(s)) for s in S)
    low = _lib.id_search_large(S, np.stack([np.zeros(n, np.int64), mpel, vi]), order, maxK=need if need > lmax else 0, maxsweeps=2)
    clust, info = rc.searchid(S, **kw)
    assert np.array_equal(clust, low["labels"][low["best"]]) and np.array_equal(info["loss_num"], low["loss_num"])
    small = SimpleNamespace(clusts=problem(100)[0])
    a, b = rc.searchid(small, nruns=2, seed=1), rc.searchpointestimate(small, "ID", nruns=2, seed=1)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in ARRAYS)
