"""The grouped exact expected-VI search on the GPU (k_vigroups<PQ> of csrc/visearch_kernel.inc.hip through
rc_vi_search_groups).  Its whole contract is "run r is rc_vi_search on samples[group == run_group[r]]", so every run is held,
field by field and bit for bit (loss as a double included), to rc_vi_search on that sub-array and to tests/vi_search_ref.py
handed the library's table — at the sizes where the grouped indexing can go wrong: groups smaller and larger than the rows of
a pass, the label-staging boundaries sized by the largest group, slot caps that differ between the groups of one launch."""
import functools

import numpy as np
import pytest

import vi_search_ref as V
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

KEYS = ("loss_num", "sweeps", "moves", "converged", "K")


@functools.lru_cache(maxsize=None)
def library_table(n):
    G = _lib.vi_gtable(n)
    G.setflags(write=False)
    return G


def noisy(n, m, K, noise, seed):
    """m samples of a planted K-cluster partition of n points, a `noise` share of the points relabelled at random per sample"""
    rng = np.random.default_rng(seed)
    truth = rng.integers(1, K + 1, size=n)
    S = np.tile(truth, (m, 1)).astype(np.int64)
    flip = rng.random((m, n)) < noise
    S[flip] = rng.integers(1, K + 1, size=int(flip.sum()))
    return S


def groups_of(sizes, m, seed):
    """a group vector with sizes[g] samples in group g, the rest in no group, interleaved at random"""
    g = np.full(m, -1, np.int32)
    g[: sum(sizes)] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return np.random.default_rng(seed).permutation(g)


def starts(n, nruns, K, seed):
    """nruns starts and orders: from empty labels in a random order, from a random labelling in identity order, alternating"""
    rng = np.random.default_rng(seed)
    init = np.zeros((nruns, n), np.int64)
    order = np.tile(np.arange(1, n + 1, dtype=np.int32), (nruns, 1))
    for r in range(nruns):
        if r % 2 == 0:
            order[r] = rng.permutation(n) + 1
        else:
            init[r] = rng.integers(0, K + 1, n)
    return init, order


def check(S, group, run_group, init, order, maxK=0, maxsweeps=100, what="", reference=True):
    """the grouped call against rc_vi_search and vi_search_ref per run; returns the grouped result"""
    n = S.shape[1]
    run_group = np.asarray(run_group, np.int32)
    got = _lib.vi_search_groups(S, group, init, order, run_group, maxK=maxK, maxsweeps=maxsweeps)
    for r, g in enumerate(run_group):
        sub = S[group == g]
        one = _lib.vi_search(sub, init[r:r + 1], order[r:r + 1], maxK=maxK, maxsweeps=maxsweeps)
        print(what, "run", r, "group", g, "m_g", len(sub), "Q", got["loss_num"][r], "sweeps", got["sweeps"][r], "moves", got["moves"][r],
              "K", got["K"][r], "loss", got["loss"][r])
        assert np.array_equal(got["labels"][r], one["labels"][0]), (what, r)
        for k in KEYS + ("loss",):
            assert got[k][r] == one[k][0], (what, r, k, got[k][r], one[k][0])
        if reference:
            ref = V.vi_search_ref(sub, library_table(n), init[r], order[r], maxK=maxK, maxsweeps=maxsweeps)
            assert np.array_equal(got["labels"][r], ref["labels"]), (what, r)
            for k in KEYS:
                assert got[k][r] == ref[k], (what, r, k, got[k][r], ref[k])
    ngroups = max(int(group.max()) + 1, 1)
    assert len(got["best"]) == ngroups
    for g in range(ngroups):
        mine = np.flatnonzero(run_group == g)
        want = -1 if len(mine) == 0 else int(mine[np.argmin(got["loss_num"][mine])])
        assert got["best"][g] == want, (what, g, got["best"][g], want)
    return got


def test_groups_of_1_7_and_53_samples_and_a_group_without_a_run():
    n, m = 37, 61
    S = noisy(n, m, 4, 0.25, seed=1)
    group = groups_of([1, 7, 53], m, seed=2)
    # 61 = 1 + 7 + 53: take some samples out of the largest group again, into no group and into a fourth group without a run
    big = np.flatnonzero(group == 2)
    group[big[:3]] = -1
    group[big[3:8]] = 3
    assert [int((group == g).sum()) for g in (-1, 0, 1, 2, 3)] == [3, 1, 7, 45, 5]
    init, order = starts(n, 6, 2, seed=3)                               # two labels: within every group's cap
    got = check(S, group, [0, 0, 1, 1, 2, 2], init, order, what="n37")
    assert got["best"][3] == -1
    # the same with exactly 53 in the largest group
    group2 = groups_of([1, 7, 53], m, seed=4)
    check(S, group2, [2, 1, 0, 2, 1, 0], init, order, what="n37-full")


@pytest.mark.parametrize("n,big,small", [(12, 1030, 3), (10, 4100, 5)], ids=["past-1024", "past-4096"])
def test_label_staging_depth_is_the_largest_groups(n, big, small):
    m = big + small + 4
    S = noisy(n, m, 3, 0.2, seed=n)
    group = groups_of([big, small], m, seed=n + 1)
    init, order = starts(n, 4, 3, seed=n + 2)
    check(S, group, [0, 1, 1, 0], init, order, maxK=3, what=f"m{big}")
    # and the small group on its own, at its own staging depth, returns the same
    alone = np.where(group == 1, 0, -1).astype(np.int32)
    a = _lib.vi_search_groups(S, alone, init[1:3], order[1:3], [0, 0], maxK=3)
    b = _lib.vi_search_groups(S, group, init, order, [0, 1, 1, 0], maxK=3)
    assert np.array_equal(a["labels"], b["labels"][1:3]) and np.array_equal(a["loss_num"], b["loss_num"][1:3])


@pytest.mark.parametrize("cap,small,large", [(12, 100, 400), (20, 150, 260)], ids=["kpad12", "kpad20"])
def test_slot_caps_that_leave_threads_idle(cap, small, large):
    """kpad = 12 / 20: G = 3 / 5 threads per table row, R = 341 / 204 rows per pass, 1023 / 1020 active threads"""
    n, m = 30, small + large
    assert small < 1024 // (cap // 4) < large
    S = noisy(n, m, 5, 0.3, seed=cap)
    group = groups_of([small, large], m, seed=cap + 1)
    init, order = starts(n, 4, cap, seed=cap + 2)
    got = check(S, group, [0, 1, 0, 1], init, order, maxK=cap, what=f"cap{cap}")
    assert got["K"].max() <= cap


def test_every_group_has_its_own_default_cap():
    n, m = 36, 40
    S = np.concatenate([noisy(n, 14, 2, 0.2, seed=5), noisy(n, 26, 9, 0.2, seed=6)])
    group = np.repeat(np.array([0, 1], np.int32), [14, 26])
    assert V.relabel(S[:14])[1] == 2 and V.relabel(S[14:])[1] == 9
    init, order = starts(n, 4, 2, seed=7)
    got = check(S, group, [0, 1, 0, 1], init, order, what="caps-2-9")
    assert got["K"][0] <= 2 and got["K"][2] <= 2
    # a start with three clusters fits the second group's cap and not the first's
    three = np.array([[1, 2, 3] * 12], np.int64)
    ident = np.arange(1, n + 1, dtype=np.int32)[None, :]
    check(S, group, [1], three, ident, what="three-in-9")
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG.*run 1 starts with 3 clusters, more than the slot cap 2"):
        _lib.vi_search_groups(S, group, three, ident, [0])


def test_a_binding_cap():
    n, m = 37, 50
    S = noisy(n, m, 6, 0.2, seed=8)
    group = groups_of([20, 30], m, seed=9)
    init, order = starts(n, 4, 2, seed=10)
    got = check(S, group, [0, 0, 1, 1], init, order, maxK=2, what="maxK2")
    free = _lib.vi_search_groups(S, group, init, order, [0, 0, 1, 1])
    assert got["K"].max() <= 2 < free["K"].max()
    one = check(S, group, [0, 0, 1, 1], init, order, maxK=2, maxsweeps=1, what="maxK2-onesweep")
    assert (one["sweeps"] == 1).all()


def test_a_group_of_one_sample_returns_that_sample():
    n, m = 23, 9
    S = noisy(n, m, 4, 0.3, seed=11)
    group = np.full(m, 1, np.int32)
    group[4] = 0
    group[7] = 2
    init = np.zeros((2, n), np.int64)
    order = np.stack([np.random.default_rng(12).permutation(n) + 1, np.arange(1, n + 1)]).astype(np.int32)
    got = check(S, group, [0, 1], init, order, what="single")
    assert np.array_equal(got["labels"][0], V.sortlabels(S[4]))
    assert got["loss"][0] == 0.0 and got["loss_num"][0] == -V.constant(S[4:5], library_table(n))
    assert got["best"].tolist() == [0, 1, -1]
    labels, info = rc.searchvigroups(S, group, init, order, [0, 1])
    assert np.array_equal(labels[0], V.sortlabels(S[4])) and np.array_equal(labels[1], got["labels"][1]) and not labels[2].any()


def test_a_run_does_not_depend_on_what_shares_the_launch():
    n, m = 37, 61
    S = noisy(n, m, 4, 0.25, seed=1)
    group = groups_of([1, 7, 50], m, seed=13)
    init, order = starts(n, 6, 2, seed=14)
    run_group = np.array([0, 1, 2, 2, 1, 0], np.int32)
    whole = _lib.vi_search_groups(S, group, init, order, run_group)
    # the whole set searched by the existing entry, before and after
    before = _lib.vi_search(S, init, order)
    for r in range(6):
        # the run alone, its group renumbered and the other samples in no group
        alone = np.where(group == run_group[r], 0, -1).astype(np.int32)
        one = _lib.vi_search_groups(S, alone, init[r:r + 1], order[r:r + 1], [0])
        assert np.array_equal(one["labels"][0], whole["labels"][r])
        for k in KEYS + ("loss",):
            assert one[k][0] == whole[k][r], (r, k)
    # another order of the runs
    perm = np.array([5, 3, 1, 0, 2, 4])
    other = _lib.vi_search_groups(S, group, init[perm], order[perm], run_group[perm])
    assert np.array_equal(other["labels"], whole["labels"][perm])
    for k in KEYS + ("loss",):
        assert np.array_equal(other[k], whole[k][perm]), k
    after = _lib.vi_search(S, init, order)
    assert np.array_equal(before["labels"], after["labels"]) and before["best"] == after["best"]
    for k in KEYS + ("loss",):
        assert np.array_equal(before[k], after[k]), k
    refs = [V.vi_search_ref(S, library_table(n), init[r], order[r]) for r in range(6)]
    for r, ref in enumerate(refs):
        assert np.array_equal(after["labels"][r], ref["labels"]) and all(after[k][r] == ref[k] for k in KEYS), r


def test_errors_return_their_codes_before_any_device_work():
    L = _lib.lib()
    n, m = 8, 6
    S = noisy(n, m, 2, 0.2, seed=15)
    group = np.array([0, 0, 1, 1, -1, 1], np.int32)
    run_group = np.array([0, 1], np.int32)
    init = np.zeros((2, n), np.int64)
    order = np.tile(np.arange(1, n + 1, dtype=np.int32), (2, 1))
    labels = np.zeros((2, n), np.int64)
    runs = (_lib.RcPsmRun * 2)()
    best = np.zeros(3, np.int32)

    def call(samples=S, m_=m, n_=n, group_=group, ngroups=3, nruns=2, run_group_=run_group, init_=init, order_=order, maxK=0, maxsweeps=5,
             labels_=labels, runs_=runs, best_=best):
        p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x)
        code = L.rc_vi_search_groups(0, p(samples), m_, n_, p(group_), ngroups, nruns, p(run_group_), p(init_), p(order_), maxK, maxsweeps,
                                     p(labels_), runs_, p(best_), None)
        return code, L.rc_last_error(None).decode()

    ARG, CAP = -1, -6

    def changed(a, at, v):
        a = a.copy()
        a[at] = v
        return a
    assert V.relabel(S)[1] == 2
    three = changed(init, (1, slice(0, 3)), [5, 2, 7])
    cases = [("NULL samples", dict(samples=None)), ("NULL group", dict(group_=None)), ("NULL run_group", dict(run_group_=None)),
             ("NULL init", dict(init_=None)), ("NULL order", dict(order_=None)), ("NULL labels", dict(labels_=None)),
             ("NULL runs", dict(runs_=None)), ("NULL best", dict(best_=None)),
             ("m < 1", dict(m_=0)), ("n < 1", dict(n_=0)), ("nruns < 1", dict(nruns=0)), ("ngroups < 1", dict(ngroups=0)),
             ("maxsweeps < 1", dict(maxsweeps=0)), ("maxK < 0", dict(maxK=-1)),
             ("group id below -1", dict(group_=changed(group, 2, -2))), ("group id above", dict(group_=changed(group, 2, 3))),
             ("run_group negative", dict(run_group_=changed(run_group, 1, -1))), ("run_group above", dict(run_group_=changed(run_group, 1, 3))),
             ("run_group names an empty group", dict(run_group_=changed(run_group, 1, 2))),
             ("sample label 0", dict(samples=changed(S, (1, 2), 0))), ("sample label above n", dict(samples=changed(S, (2, 0), n + 1))),
             ("label of an ungrouped sample", dict(samples=changed(S, (4, 0), n + 1))),
             ("start label above n", dict(init_=changed(init, (1, 3), n + 1))), ("negative start label", dict(init_=changed(init, (0, 3), -1))),
             ("repeated order entry", dict(order_=changed(order, (1, 0), 2))), ("order entry 0", dict(order_=changed(order, (0, 0), 0))),
             ("start beyond maxK", dict(init_=three, maxK=2)), ("start beyond its group's cluster count", dict(init_=three))]
    for what, kw in cases:
        code, msg = call(**kw)
        print(what, "->", code, msg)
        assert code == ARG and msg.startswith("rc_vi_search_groups"), (what, code, msg)
    # capacities: checked before the arrays they do not need are read, so the small buffers do
    code, msg = call(n_=8193)
    assert code == CAP and "8192" in msg, msg
    code, msg = call(m_=2 ** 31 // n)                                    # m·n = 2^31
    assert code == CAP and "31 bits" in msg, msg
    huge = np.zeros(2 ** 26 // n + 1, np.int32)                          # one group of m_g·n = 2^26 + n; the samples are not read
    code, msg = call(m_=len(huge), group_=huge, ngroups=1, run_group_=np.zeros(2, np.int32))
    assert code == CAP and "2^26" in msg, msg
    wide = np.tile(np.arange(1, 1031, dtype=np.int64), (2, 1))           # a slot cap of 1030 in the group that is searched
    g2 = np.array([0, 1], np.int32)
    i2, o2 = np.zeros((1, 1030), np.int64), np.arange(1, 1031, dtype=np.int32)[None, :]
    code, msg = call(samples=wide, m_=2, n_=1030, group_=g2, ngroups=2, nruns=1, run_group_=np.zeros(1, np.int32), init_=i2, order_=o2)
    assert code == CAP and "1024" in msg, msg
    # the table budget: 40 runs × m_g·Lmax_g·Kcap4·2 B = 40 × 64·1024·1024·2 B = 5 GiB
    nb, mb = 1024, 64
    big = np.tile(np.arange(1, nb + 1, dtype=np.int64), (mb, 1))
    code, msg = call(samples=big, m_=mb, n_=nb, group_=np.zeros(mb, np.int32), ngroups=1, nruns=40, run_group_=np.zeros(40, np.int32),
                     init_=np.zeros((1, nb), np.int64), order_=o2)
    assert code == CAP and "budget" in msg, msg
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.vi_search_groups(changed(S, (1, 2), 0), group, init, order, run_group)
    # and a valid call afterwards
    code, msg = call()
    assert code == 0, msg
    for r, g in enumerate(run_group):
        ref = V.vi_search_ref(S[group == g], library_table(n), init[r], order[r], maxsweeps=5)
        assert np.array_equal(labels[r], ref["labels"]) and runs[r].loss_num == ref["loss_num"]
        assert (runs[r].sweeps, runs[r].moves, runs[r].K, bool(runs[r].converged)) == (ref["sweeps"], ref["moves"], ref["K"], ref["converged"])
    assert best.tolist() == [0, 1, -1]
