"""rc_psm_search_large* (csrc/pointsearch_large.inc.hip): the Binder and VI-bound searches for n <= 32767.  Binder runs are exact
integers and must equal the NumPy restatement (psm_search_ref.py) bit for bit; VI runs must equal rc_psm_search's where both
kernels run (n <= 8192), and above that reproduce themselves and satisfy the loss identity.  RC_PSM_WINDOW forces many passes of
the accumulator window at small n."""
import ctypes as C_
import functools

import numpy as np
import pytest

import psm_search_ref as R
import redclust_amd as rc
from redclust_amd import _lib
from test_gpu_pointsearch import LOSS_TOL, _Samples, _context_with_samples

pytestmark = pytest.mark.gpu
WINDOWS = [None, "1", "16"]
KEYS = ("labels", "loss", "loss_num", "sweeps", "converged", "moves", "K")


def set_window(monkeypatch, window):
    if window is None:
        monkeypatch.delenv("RC_PSM_WINDOW", raising=False)
    else:
        monkeypatch.setenv("RC_PSM_WINDOW", window)                  # read by the library at every call


@functools.lru_cache(maxsize=None)
def problem(n, m=7, K=4, noise=0.15):
    """(samples, counts, init 4×n, order 4×n): empty labels in a shuffled order, a sample, and two starts in the highest slots —
    all points in slot n; slots n, n − 1 alternating — so that hi is far above a forced window and several passes run"""
    S, C = R.planted_counts(n, m, min(K, n), noise, seed=2000 + n)
    init = np.stack([np.zeros(n, np.int64), S[0], np.full(n, n), np.where(np.arange(n) % 2 == 0, n, n - 1)]).astype(np.int64)
    order = np.stack([np.random.default_rng(n).permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1),
                      np.arange(1, n + 1)]).astype(np.int32)
    return S, C, init, order


@functools.lru_cache(maxsize=None)
def binder_refs(n, maxK, maxsweeps):
    _, C, init, order = problem(n)
    init = np.where(init > maxK, maxK, init) if maxK else init
    return init, [R.psm_search_ref(C, 7, R.BINDER, init[r], order[r], maxK=maxK, maxsweeps=maxsweeps) for r in range(4)]


def assert_binder(got, refs):
    for r, ref in enumerate(refs):
        assert np.array_equal(got["labels"][r], ref["labels"]), r
        for k in ("loss_num", "sweeps", "moves", "converged", "K"):
            assert got[k][r] == ref[k], (r, k, got[k][r], ref[k])
    assert got["best"] == int(np.argmin([ref["loss"] for ref in refs]))


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n,maxK,maxsweeps", [(1, 0, 100), (2, 0, 100), (5, 0, 100), (63, 0, 100), (257, 0, 100), (1027, 0, 100),
                                              (257, 2, 100), (257, 0, 1)])
def test_binder_equals_the_reference_bit_for_bit(monkeypatch, n, maxK, maxsweeps, window):
    set_window(monkeypatch, window)
    _, C, _, order = problem(n)
    init, refs = binder_refs(n, maxK, maxsweeps)
    assert_binder(_lib.psm_search_large(C, 7, R.BINDER, init, order, maxK=maxK, maxsweeps=maxsweeps), refs)


@pytest.mark.parametrize("n", [4099, 8195, 16389])
def test_binder_on_every_row_width(n):
    """Q4 = 2, 4, 8 quads per thread; n is no multiple of 4 or of 4096.  The two above 8192 had no kernel before.  The NumPy
    restatement is what takes the time here (seconds per sweep at n = 8195, about ten at 16389), so the largest keeps to one sweep."""
    m, maxsweeps = 3, 2 if n < 16000 else 1
    rng = np.random.default_rng(n)
    S = np.tile(rng.integers(1, 6, n), (m, 1)).astype(np.int64)       # K = 5 planted, 5 % of the labels redrawn per sample
    flip = rng.random((m, n)) < 0.05
    S[flip] = rng.integers(1, 6, int(flip.sum()))
    C = rc.posterior_counts(S)
    init = np.stack([np.zeros(n, np.int64), S[0]])
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1)]).astype(np.int32)
    got = _lib.psm_search_large(C, m, R.BINDER, init, order, maxsweeps=maxsweeps)
    assert_binder(got, [R.psm_search_ref(C, m, R.BINDER, init[r], order[r], maxsweeps=maxsweeps) for r in range(2)])


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", [5, 257, 1027, 4099])
def test_vi_equals_the_lds_kernel(monkeypatch, n, window):
    _, C, init, order = problem(n)
    monkeypatch.delenv("RC_PSM_WINDOW", raising=False)
    old = _lib.psm_search(C, 7, R.VILB, init[:2], order[:2])
    set_window(monkeypatch, window)
    new = _lib.psm_search_large(C, 7, R.VILB, init[:2], order[:2])
    for k in KEYS:
        assert new[k].tobytes() == old[k].tobytes(), k
    assert new["best"] == old["best"]


def test_vi_above_the_lds_capacity():
    n, m = 8195, 3
    S, C, init, order = problem(n, m, 5, 0.05)
    got, again = (_lib.psm_search_large(C, m, R.VILB, init[:2], order[:2], maxsweeps=3) for _ in range(2))
    for k in KEYS:
        assert got[k].tobytes() == again[k].tobytes(), k
    for r in range(2):
        err = abs(got["loss"][r] - (R.vi_f(got["labels"][r], C) / n + 2.0 * np.log(m)))
        print("run", r, "loss", got["loss"][r], "err", err, "sweeps", got["sweeps"][r], "K", got["K"][r])
        assert err <= LOSS_TOL
    assert got["loss"][1] <= R.vi_f(S[0], C) / n + 2.0 * np.log(m) + LOSS_TOL


@pytest.mark.parametrize("loss", [R.BINDER, R.VILB])
def test_three_forms_agree_and_the_context_is_left_alone(loss):
    n, m = 100, 5
    ctx, recorded = _context_with_samples(n, m)
    counts, before = ctx.cocluster_counts(), ctx.get_state()
    order = np.stack([np.random.default_rng(2).permutation(n) + 1, np.arange(1, n + 1)]).astype(np.int32)
    init = np.stack([np.zeros(n, np.int64), recorded[0]])
    outs = [_lib.psm_search_large(counts, m, loss, init, order), _lib.psm_search_large(None, m, loss, init, order, ctx=ctx),
            _lib.psm_search_large_samples(np.stack(recorded), loss, init, order), _lib.psm_search(counts, m, loss, init, order)]
    for o in outs[1:]:
        for k in KEYS:
            assert o[k].tobytes() == outs[0][k].tobytes(), k
    after = ctx.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert np.array_equal(ctx.cocluster_counts(), counts)
    ctx.close()


def test_errors_and_their_precedence():
    L = _lib.lib()
    n, m = 8, 3
    _, C = R.planted_counts(n, m, 2, 0.2, seed=1)
    init, order = np.zeros((2, n), np.int64), np.tile(np.arange(1, n + 1, dtype=np.int32), (2, 1))
    labels, runs, best = np.zeros((2, n), np.int64), (_lib.RcPsmRun * 2)(), C_.c_int32()

    def call(m_=m, n_=n, loss=0, init_=init, order_=order, maxsweeps=5):
        code = L.rc_psm_search_large(0, C.ctypes.data, m_, n_, loss, 2, init_.ctypes.data, order_.ctypes.data, 0, maxsweeps,
                                     labels.ctypes.data, runs, C_.byref(best), None)
        return code, L.rc_last_error(None).decode()

    ARG, CAP = -1, -6
    bad_order, bad_label = order.copy(), init.copy()
    bad_order[1, 0], bad_label[1, 3] = 2, n + 1
    code, msg = call(n_=32768)
    assert code == CAP and "32767" in msg
    assert call(m_=2 ** 31 // n)[0] == CAP
    code, msg = call(n_=32768, maxsweeps=0)
    assert code == ARG and "maxsweeps" in msg
    assert call(loss=2)[0] == ARG
    for kw, text in [(dict(order_=bad_order), "point search: the order of run 2"), (dict(init_=bad_label), "point search: label 9 of run 2")]:
        code, msg = call(**kw)
        assert code == ARG and text in msg, msg
    assert call()[0] == 0 and labels.min() >= 1


@pytest.mark.parametrize("n,loss,entry", [(8195, "binder", "psm_search_large_samples"), (100, "VI", "psm_search_samples")])
def test_searchpointestimate_routes_by_n(n, loss, entry):
    """above 8192 the large entry's best run; at or below it today's entry, byte for byte"""
    S = problem(n, 3, 5, 0.05)[0]
    clust, info = rc.searchpointestimate(_Samples(S), loss, nruns=2, maxsweeps=2, seed=4)
    rng = np.random.Generator(np.random.Philox(key=4))
    order = np.stack([rng.permutation(n).astype(np.int32) + 1 for _ in range(2)] + [np.arange(1, n + 1, dtype=np.int32)])
    init = np.stack([np.zeros(n, np.int64)] * 2 + [rc.getpointestimate(_Samples(S), "MPEL", loss)[0]])
    low = getattr(_lib, entry)(S, {"binder": R.BINDER, "VI": R.VILB}[loss], init, order, maxsweeps=2)
    for k in KEYS:
        assert info[k].tobytes() == low[k].tobytes(), k
    assert np.array_equal(clust, low["labels"][low["best"]])
    for what in (lambda: rc.searchpointestimate(_Samples(S), "VI", exact=True), lambda: rc.searchpointestimate(_Samples(S), "ID"),
                 lambda: rc.searchmaxpear(_Samples(S)), lambda: rc.hclust(_Samples(S))) if n > 8192 else ():
        with pytest.raises(ValueError, match="n <= 8192"):
            what()
