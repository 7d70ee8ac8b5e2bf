"""The point-estimate search on the GPU (csrc/pointsearch.inc.hip through rc_psm_search / rc_psm_search_ctx and
searchpointestimate).  Binder runs are exact integers and are held to tests/psm_search_ref.py bit for bit; VI runs decide
on device logarithms, so they are held to properties evaluated in NumPy.

Shapes: the wave (63/64/65) and workgroup (1000/1025 around the 1024 threads) edges of the row reduction, n = 1 and 2.
Runs per shape: a random order from empty labels, the identity order from one cluster, the reverse order from labels of
which half are unallocated.

VI tolerances.  Every log term of a step is rounded once to 2^-40, at most 1025 terms per candidate: < 1e-9 on a
candidate's score, given a tenfold margin: MOVE_TOL = 1e-8.  The returned loss is a plain f64 sum of at most 1025·2 log
terms of magnitude <= log(m·n) ≈ 17 (each within an ulp or two of NumPy's), divided by n: far below LOSS_TOL = 1e-9."""
import functools
import os

import numpy as np
import pytest

import psm_search_ref as R
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 3, 1, 0.0), (2, 3, 2, 0.0), (63, 7, 3, 0.1), (64, 7, 4, 0.1), (65, 50, 5, 0.2), (257, 20, 16, 0.2),
          (1000, 20, 40, 0.3), (1025, 9, 10, 0.2)]
IDS = [f"n{s[0]}" for s in SHAPES]
LOSS_TOL, MOVE_TOL = 1e-9, 1e-8


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(samples, counts, init 3×n, order 3×n) of a shape; computed once and shared (never modified)."""
    n, m, K, noise = shape
    S, C = R.planted_counts(n, m, K, noise, seed=1000 + n)
    rng = np.random.default_rng(n)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]).astype(np.int32)
    mixed = rng.integers(1, min(K, n) + 1, n)
    mixed[rng.permutation(n)[: n // 2]] = 0
    init = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), mixed.astype(np.int64)])
    for a in (S, C, init, order):
        a.setflags(write=False)
    return S, C, init, order


@functools.lru_cache(maxsize=None)
def binder_reference(shape, maxK, maxsweeps):
    _, C, init, order = problem(shape)
    return [R.psm_search_ref(C, shape[1], R.BINDER, init[r], order[r], maxK=maxK, maxsweeps=maxsweeps) for r in range(3)]


def run_inits(shape, maxK):
    """the three runs; with a cap the mixed start is clipped to maxK clusters"""
    _, _, init, _ = problem(shape)
    if maxK:
        init = np.where(init > maxK, maxK, init)
    return init


@pytest.mark.parametrize("maxK,maxsweeps", [(0, 100), (2, 100), (0, 1)], ids=["free", "maxK2", "onesweep"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_binder_equals_the_reference_bit_for_bit(shape, maxK, maxsweeps):
    n, m = shape[0], shape[1]
    _, C, _, order = problem(shape)
    init = run_inits(shape, maxK)
    got = _lib.psm_search(C, m, R.BINDER, init, order, maxK=maxK, maxsweeps=maxsweeps)
    refs = [R.psm_search_ref(C, m, R.BINDER, init[r], order[r], maxK=maxK, maxsweeps=maxsweeps) for r in range(3)] if maxK \
        else binder_reference(shape, maxK, maxsweeps)
    pairs = n * (n - 1) // 2
    for r, ref in enumerate(refs):
        print(shape, r, "sweeps", got["sweeps"][r], "moves", got["moves"][r], "K", got["K"][r], "num", got["loss_num"][r])
        assert np.array_equal(got["labels"][r], ref["labels"]), r
        for k in ("loss_num", "sweeps", "moves", "converged", "K"):
            assert got[k][r] == ref[k], (r, k, got[k][r], ref[k])
        assert got["loss"][r] == ((int(got["loss_num"][r]) / (m * pairs)) if pairs else 0.0)
        if maxK:
            assert got["K"][r] <= maxK
        if maxsweeps == 1 and n > 1:
            assert got["sweeps"][r] == 1
    assert got["best"] == int(np.argmin([ref["loss"] for ref in refs]))
    if maxsweeps == 1 and n > 2:
        assert not got["converged"][0]          # a run from empty labels moves every point in its first sweep


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_vi_properties(shape):
    n, m = shape[0], shape[1]
    _, C, init, order = problem(shape)
    got = _lib.psm_search(C, m, R.VILB, init, order)
    again = _lib.psm_search(C, m, R.VILB, init, order)
    for k in ("labels", "loss", "loss_num", "sweeps", "converged", "moves", "K"):        # (d) identical bytes
        assert got[k].tobytes() == again[k].tobytes(), k
    assert got["best"] == again["best"] == int(np.argmin(got["loss"]))
    steps = [_lib.psm_search(C, m, R.VILB, init, order, maxsweeps=s) for s in (1, 2, 3)]
    for r in range(3):
        lab = got["labels"][r]
        assert lab.min() >= 1 and np.array_equal(lab, R.sortlabels(lab)) and got["K"][r] == lab.max() and got["loss_num"][r] == 0
        err = abs(got["loss"][r] - rc.expectedloss(lab, C, m, "VI"))
        gain = R.vi_best_move_gain(lab, C, m) if got["converged"][r] else float("nan")
        f0 = R.vi_f(init[r], C) if (init[r] > 0).all() else np.inf         # f of the start where every point has a cluster
        fs = [f0] + [R.vi_f(s["labels"][r], C) for s in steps]
        print(shape, r, "sweeps", got["sweeps"][r], "K", got["K"][r], "loss err", err, "best move gain", gain, "f per sweep", fs)
        assert err <= LOSS_TOL                                                           # (a)
        assert got["converged"][r]
        assert gain <= MOVE_TOL                                                          # (b)
        assert all(fs[s + 1] <= fs[s] + MOVE_TOL for s in range(3))                     # (c)
        for s, st in zip((1, 2, 3), steps):
            assert st["sweeps"][r] == min(s, got["sweeps"][r])


def test_windowed_passes_give_the_same_runs():
    """With fewer accumulator slots than clusters the occupied slots are covered in several passes (what VI needs beyond
    n = 8104): forced here at a small n, the Binder runs must still equal the reference bit for bit and
    the VI runs must equal the single-pass ones."""
    n, m = 65, 50
    _, C = R.planted_counts(n, m, 5, 0.2, seed=3)
    init = np.stack([np.arange(1, n + 1), np.arange(n, 0, -1), np.zeros(n, np.int64)])
    order = np.stack([np.arange(1, n + 1), np.arange(n, 0, -1), np.random.default_rng(0).permutation(n) + 1])
    outs, old = {}, os.environ.get("RC_PSM_WINDOW")
    try:
        for window in ("", "16"):
            os.environ["RC_PSM_WINDOW"] = window                    # read by the library at every call
            outs[window] = {f"{l}_{k}": np.asarray(v) for l in (0, 1) for k, v in _lib.psm_search(C, m, l, init, order).items()}
    finally:
        if old is None:
            os.environ.pop("RC_PSM_WINDOW", None)
        else:
            os.environ["RC_PSM_WINDOW"] = old
    for k in outs[""]:
        if not k.endswith("kernel_ms"):
            assert outs[""][k].tobytes() == outs["16"][k].tobytes(), k
    ref = R.psm_search_ref(C, m, R.BINDER, np.arange(1, n + 1), np.arange(1, n + 1))
    assert np.array_equal(outs["16"]["0_labels"][0], ref["labels"]) and outs["16"]["0_moves"][0] == ref["moves"]


class _Samples:
    def __init__(self, clusts):
        self.clusts = list(clusts)


@pytest.mark.parametrize("loss", ["binder", "VI"])
def test_never_worse_than_the_sample_search(loss):
    S, C = R.planted_counts(257, 50, 16, 0.2, seed=11)
    samples = _Samples(S)
    assert np.array_equal(rc.cocluster_counts(samples.clusts), C)
    clust, info = rc.searchpointestimate(samples, loss, nruns=4, seed=3)
    mpel = rc.getpointestimate(samples, "MPEL", loss)[0]
    bound = rc.expectedloss(mpel, C, 50, loss)
    print(loss, "search", info["loss"], "MPEL sample", bound)
    assert len(info["loss"]) == 5 and info["best"] == int(np.argmin(info["loss"]))
    assert info["loss"][info["best"]] <= bound
    assert abs(rc.expectedloss(clust, C, 50, loss) - info["loss"][info["best"]]) <= LOSS_TOL
    assert np.array_equal(clust, info["labels"][info["best"]])
    # the default orders are the documented Philox permutations: the same runs through the low-level entry
    rng = np.random.Generator(np.random.Philox(key=3))
    order = np.stack([rng.permutation(257).astype(np.int32) + 1 for _ in range(4)])
    low = _lib.psm_search(C, 50, {"binder": 0, "VI": 1}[loss], np.zeros((4, 257), np.int64), order)
    assert np.array_equal(low["labels"], info["labels"][:4])
    # counts + numsamples, and extra starts through init=
    c2, i2 = rc.searchpointestimate(C, loss, numsamples=50, nruns=4, seed=3, init=[mpel])
    assert np.array_equal(i2["labels"], info["labels"]) and np.array_equal(c2, clust)
    if loss == "VI":
        assert np.isfinite(info["vi_constant"])


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


@pytest.mark.parametrize("loss", [R.BINDER, R.VILB])
def test_context_form_equals_the_host_form_and_leaves_the_chain_alone(loss):
    n, m = 100, 5
    ctx, recorded = _context_with_samples(n, m)
    twin, _ = _context_with_samples(n, m)
    counts = ctx.cocluster_counts()
    assert np.array_equal(counts, rc.cocluster_counts(recorded))
    rng = np.random.default_rng(2)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1)]).astype(np.int32)
    init = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), recorded[0]])
    before = ctx.get_state()
    a = _lib.psm_search(None, m, loss, init, order, ctx=ctx)
    b = _lib.psm_search(counts, m, loss, init, order)
    for k in ("labels", "loss", "loss_num", "sweeps", "converged", "moves", "K"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best"] == b["best"]
    clust, info = rc.searchpointestimate(loss="binder" if loss == R.BINDER else "VI", nruns=2, numsamples=m, ctx=ctx)
    assert info["loss"][info["best"]] == info["loss"].min() and len(clust) == n
    after = ctx.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert np.array_equal(ctx.cocluster_counts(), counts)
    ctx.gibbs_sweep(1.25, 0.4, seed=9, sweep_index=m)
    twin.gibbs_sweep(1.25, 0.4, seed=9, sweep_index=m)
    assert np.array_equal(ctx.get_state()[0], twin.get_state()[0]) and ctx.loglik() == twin.loglik()
    ctx.close(); twin.close()


def test_errors_return_their_codes_and_the_process_goes_on():
    import ctypes as C_
    L = _lib.lib()
    n, m = 8, 3
    _, C = R.planted_counts(n, m, 2, 0.2, seed=1)
    init = np.zeros((1, n), np.int64)
    order = np.arange(1, n + 1, dtype=np.int32)[None, :].copy()
    labels = np.zeros((1, n), np.int64)
    runs = (_lib.RcPsmRun * 1)()
    best = C_.c_int32()

    def call(counts=C, m_=m, n_=n, loss=0, nruns=1, init_=init, order_=order, maxK=0, maxsweeps=5, labels_=labels, runs_=runs, best_=best):
        p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x)
        rc_ = L.rc_psm_search(0, p(counts), m_, n_, loss, nruns, p(init_), p(order_), maxK, maxsweeps, p(labels_), runs_,
                              None if best_ is None else C_.byref(best_), None)
        return rc_, L.rc_last_error(None).decode()

    ARG, STATE, CAP = -1, -5, -6
    asym = C.copy(); asym[0, 1] += 1
    diag = C.copy(); diag[2, 2] = m - 1
    big = C.copy(); big[0, 1] = big[1, 0] = m + 1
    bad_label = init.copy(); bad_label[0, 3] = n + 1
    neg_label = init.copy(); neg_label[0, 3] = -1
    not_perm = order.copy(); not_perm[0, 0] = 2
    zero_order = order.copy(); zero_order[0, 0] = 0
    three = np.array([[1, 2, 3, 0, 0, 0, 0, 0]], np.int64)
    cases = [("NULL counts", dict(counts=None)), ("NULL init", dict(init_=None)), ("NULL order", dict(order_=None)),
             ("NULL labels", dict(labels_=None)), ("NULL runs", dict(runs_=None)), ("NULL best", dict(best_=None)),
             ("m < 1", dict(m_=0)), ("n < 1", dict(n_=0)), ("nruns < 1", dict(nruns=0)), ("maxsweeps < 1", dict(maxsweeps=0)),
             ("maxK < 0", dict(maxK=-1)), ("unknown loss", dict(loss=2)), ("label above n", dict(init_=bad_label)),
             ("negative label", dict(init_=neg_label)), ("repeated order entry", dict(order_=not_perm)),
             ("order entry 0", dict(order_=zero_order)), ("asymmetric counts", dict(counts=asym)),
             ("diagonal not m", dict(counts=diag)), ("count above m", dict(counts=big)), ("wrong m", dict(m_=m + 1)),
             ("init beyond maxK", dict(init_=three, maxK=2))]
    for what, kw in cases:
        code, msg = call(**kw)
        assert code == ARG and msg, (what, code, msg)
    code, msg = call(n_=8193)
    assert code == CAP and "8192" in msg
    code, msg = call(m_=2 ** 31)
    assert code == CAP and msg
    # the context form: NULL context, nothing recorded yet
    args = (m, 0, 1, init.ctypes.data, order.ctypes.data, 0, 5, labels.ctypes.data, runs, C_.byref(best), None)
    assert L.rc_psm_search_ctx(None, *args) == ARG
    d = rc.generatemixture(n, 2, alpha=10, sigma=0.25, dim=2, seed=1)
    ctx = rc.Context(d["distancematrix"])
    assert L.rc_psm_search_ctx(ctx.h, *args) == STATE and b"recorded" in L.rc_last_error(ctx.h)
    ctx.set_params(**rc.likelihood_hyperparams(d["distancematrix"], d["clusts"]))
    ctx.set_state(d["clusts"])
    ctx.cocluster_reset()
    assert L.rc_psm_search_ctx(ctx.h, *args) == STATE
    ctx.record_sample()
    assert L.rc_psm_search_ctx(ctx.h, *((2,) + args[1:])) == ARG       # one sample recorded, two claimed
    assert L.rc_psm_search_ctx(ctx.h, *((1,) + args[1:])) == 0
    assert np.array_equal(labels[0], R.sortlabels(d["clusts"])) and runs[0].converged == 1
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.psm_search(asym, m, 0, init, order)
    ctx.close()
    # and a valid call afterwards
    code, msg = call()
    ref = R.psm_search_ref(C, m, R.BINDER, init[0], order[0], maxsweeps=5)
    assert code == 0 and np.array_equal(labels[0], ref["labels"]) and runs[0].loss_num == ref["loss_num"] and best.value == 0
