"""rc_pear_search_large* (csrc/pointsearch_large.inc.hip, k_pear_large) and searchpear: the PEAR search for n <= 32767 with no
m·T² condition.  A run is an exact integer function of its inputs, so every run is held to tests/pear_search_ref.py (Python
integers and Fractions) bit for bit, and to rc_pear_search field by field where that runs.  RC_PSM_WINDOW forces many passes of the
accumulator window at small n."""
import ctypes as C_
import functools
from fractions import Fraction

import numpy as np
import pytest

import pear_search_ref as R
import redclust_amd as rc
from redclust_amd import _lib, pointestimate
from test_gpu_pointsearch import _Samples, _context_with_samples
from test_gpu_pointsearch_large import WINDOWS, problem, set_window

pytestmark = pytest.mark.gpu
FIELDS = ("num", "den", "sweeps", "moves", "converged", "K")


def assert_runs(got, refs):
    for r, ref in enumerate(refs):
        print(r, {k: int(got[k][r]) for k in FIELDS}, "pear", got["pear"][r])
        assert np.array_equal(got["labels"][r], ref["labels"]), r
        for k in FIELDS:
            assert got[k][r] == ref[k], (r, k, got[k][r], ref[k])
        assert got["pear"][r] == float(ref["num"]) / float(ref["den"])
        assert Fraction(*R.fraction_of(int(got["X"][r]), int(got["A"][r]), int(got["P"][r]), ref["m"], ref["T"])) == Fraction(ref["num"], ref["den"])
    assert got["best"] == R.best_run(refs)


def references(C, m, init, order, **kw):
    n = len(C)
    return [dict(R.pear_search_ref(C, m, init[r], order[r], **kw), m=int(m), T=n * (n - 1) // 2) for r in range(len(init))]


@functools.lru_cache(maxsize=None)
def small_refs(n, maxK, maxsweeps):
    _, C, init, order = problem(n)
    init = np.where(init > maxK, maxK, init) if maxK else init
    return init, references(C, 7, init, order, maxK=maxK, maxsweeps=maxsweeps)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n,maxK,maxsweeps", [(1, 0, 100), (2, 0, 100), (5, 0, 100), (63, 0, 100), (257, 0, 100), (1027, 0, 100),
                                              (257, 2, 100), (257, 0, 1)])
def test_runs_equal_the_reference_bit_for_bit(monkeypatch, n, maxK, maxsweeps, window):
    """the third and fourth starts sit in slots n and n − 1: hi far above a forced window, and negative numerators on the way"""
    set_window(monkeypatch, window)
    _, C, _, order = problem(n)
    init, refs = small_refs(n, maxK, maxsweeps)
    got = _lib.pear_search_large(C, 7, init, order, maxK=maxK, maxsweeps=maxsweeps)
    assert_runs(got, refs)
    old = _lib.pear_search(C, 7, init, order, maxK=maxK, maxsweeps=maxsweeps)
    for k in FIELDS + ("labels", "pear", "best"):
        assert np.array_equal(got[k], old[k]), k


@functools.lru_cache(maxsize=None)
def planted(n, m=3):
    """K = 5 planted, 5 % of the labels redrawn per sample; two starts: empty labels in a shuffled order, the first sample"""
    rng = np.random.default_rng(n)
    S = np.tile(rng.integers(1, 6, n), (m, 1)).astype(np.int64)
    flip = rng.random((m, n)) < 0.05
    S[flip] = rng.integers(1, 6, int(flip.sum()))
    init = np.stack([np.zeros(n, np.int64), S[0]])
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1)]).astype(np.int32)
    return S, rc.posterior_counts(S), init, order


@pytest.mark.parametrize("n", [4099, 8195, 16389])
def test_every_row_width(n):
    """Q4 = 2, 4, 8 quads per thread; n is no multiple of 4 or of 4096.  The reference is what takes the time: one sweep at 16389"""
    maxsweeps = 2 if n < 16000 else 1
    _, C, init, order = planted(n)
    assert_runs(_lib.pear_search_large(C, 3, init, order, maxsweeps=maxsweeps), references(C, 3, init, order, maxsweeps=maxsweeps))


def test_fractions_beyond_128_bits():
    """the m = 3 counts and m itself times 87 000: m·n < 2^31, the diagonal is m, and num and den pass 64 bits each"""
    n, scale = 8195, 87000
    _, C, init, order = planted(n)
    C, m = C * np.uint32(scale), 3 * scale
    assert m * n < 2 ** 31 and C[0, 0] == m
    refs = references(C, m, init, order, maxsweeps=2)
    assert any(ref["num"].bit_length() + ref["den"].bit_length() > 130 for ref in refs), [(ref["num"], ref["den"]) for ref in refs]
    got = _lib.pear_search_large(C, m, init, order, maxsweeps=2)
    assert got["num"].dtype == object
    assert_runs(got, refs)


def test_three_forms_agree_and_the_context_is_left_alone():
    n, m = 100, 5
    ctx, recorded = _context_with_samples(n, m)
    counts, before, layout = ctx.cocluster_counts(), ctx.get_state(), ctx.cocluster_device_buffer()
    order = np.stack([np.random.default_rng(2).permutation(n) + 1, np.arange(1, n + 1)]).astype(np.int32)
    init = np.stack([np.zeros(n, np.int64), recorded[0]])
    outs = [_lib.pear_search_large(counts, m, init, order), _lib.pear_search_large(None, m, init, order, ctx=ctx),
            _lib.pear_search_large_samples(np.stack(recorded), init, order)]
    for o in outs[1:]:
        for k in FIELDS + ("labels", "pear", "X", "A", "P"):
            assert o[k].tobytes() == outs[0][k].tobytes(), k
        assert o["best"] == outs[0]["best"]
    assert_runs(outs[0], references(counts, m, init, order))
    after = ctx.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert ctx.cocluster_device_buffer() == layout and np.array_equal(ctx.cocluster_counts(), counts)
    ctx.close()


def test_errors_and_their_precedence():
    L = _lib.lib()
    n, m = 8, 3
    _, C = R.planted_counts(n, m, 2, 0.2, seed=1)
    init, order = np.zeros((2, n), np.int64), np.tile(np.arange(1, n + 1, dtype=np.int32), (2, 1))
    labels, runs, best = np.zeros((2, n), np.int64), (_lib.RcPearLargeRun * 2)(), C_.c_int32()

    def call(m_=m, n_=n, init_=init, order_=order, maxsweeps=5):
        code = L.rc_pear_search_large(0, C.ctypes.data, m_, n_, 2, init_.ctypes.data, order_.ctypes.data, 0, maxsweeps, labels.ctypes.data,
                                      runs, C_.byref(best), None)
        return code, L.rc_last_error(None).decode()

    ARG, CAP = -1, -6
    bad_order, bad_label = order.copy(), init.copy()
    bad_order[1, 0], bad_label[1, 3] = 2, n + 1
    code, msg = call(n_=32768)
    assert code == CAP and "32767" in msg and msg.startswith("rc_pear_search_large:")
    assert call(m_=2 ** 31 // n)[0] == CAP
    code, msg = call(n_=32768, maxsweeps=0)
    assert code == ARG and "maxsweeps" in msg
    for kw, text in [(dict(order_=bad_order), "point search: the order of run 2"), (dict(init_=bad_label), "point search: label 9 of run 2")]:
        code, msg = call(**kw)
        assert code == ARG and text in msg, msg
    assert call()[0] == 0 and labels.min() >= 1


def test_searchpear_is_searchmaxpear_where_that_runs():
    S = problem(100)[0]
    (c1, i1), (c2, i2) = rc.searchpear(_Samples(S), nruns=3, seed=5), rc.searchmaxpear(_Samples(S), nruns=3, seed=5)
    assert np.array_equal(c1, c2) and set(i1) == set(i2)
    for k in set(i1) - {"kernel_ms", "counts_ms", "best"}:
        assert i1[k].dtype == i2[k].dtype and i1[k].tobytes() == i2[k].tobytes(), k
    assert i1["best"] == i2["best"]


def test_searchpear_above_the_lds_capacity():
    """the large entry's best run on the documented starts: two Philox orders from empty labels, then the sample of highest PEAR and
    the average-linkage cut of highest PEAR in the identity order; searchmaxpear still refuses"""
    n, m = 8195, 3
    S, C, _, _ = planted(n)
    clust, info = rc.searchpear(_Samples(S), nruns=2, maxsweeps=2, seed=4)
    rng = np.random.Generator(np.random.Philox(key=4))
    order = np.stack([rng.permutation(n).astype(np.int32) + 1 for _ in range(2)] + [np.arange(1, n + 1, dtype=np.int32)] * 2)
    draws = [Fraction(*R.pear_num_den(s, C, m)) for s in S]
    cuts, _, cnum, cden = pointestimate._pear_cuts(_Samples(S), "average", 0, None, None, 0, True)
    k = pointestimate._first_max_fraction(cnum, cden)
    assert len(cuts) == -(-n // 8) and (int(cnum[k]), int(cden[k])) == R.pear_num_den(cuts[k], C, m)
    init = np.stack([np.zeros(n, np.int64)] * 2 + [S[draws.index(max(draws))], cuts[k]])
    low = _lib.pear_search_large_samples(S, init, order, maxsweeps=2)
    for key in FIELDS + ("labels", "pear"):
        assert info[key].tobytes() == low[key].tobytes(), key
    assert np.array_equal(clust, low["labels"][low["best"]])
    best = Fraction(int(info["num"][info["best"]]), int(info["den"][info["best"]]))
    assert best == Fraction(*R.pear_num_den(clust, C, m)) and best >= max(draws) and best >= Fraction(int(cnum[k]), int(cden[k]))
    with pytest.raises(ValueError, match="n <= 8192"):
        rc.searchmaxpear(_Samples(S))
