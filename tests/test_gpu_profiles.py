"""Cluster profiles on the device (-m gpu): rc_cluster_profiles through Context.profiles and the functions built on it.

Every integer output is compared with tests/profiles_ref.py on the quantised values get_matrix returns.  Shapes, labellings and
kinds of context are those of tests/test_gpu_score.py — the smallest at which the kernels can go wrong: n around the wave and
the 64-wide padding of a chunk of labellings, batch widths below and above a wave, one cluster, all singletons (K = n: more
slots than a wave has lanes at n > 64), two clusters split at a lane boundary, sparse label names, K ≈ √n — with a nonzero,
mixed-sign diagonal on the kinds of context that can hold one: it must count nowhere."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import profiles_ref as R
from score_ref import quantised
from test_gpu_score import SIZES, WIDTHS, batch, context, matrix, points

pytestmark = pytest.mark.gpu

INT_FIELDS = ("K", "within", "nearest", "neighbour")
LIST_FIELDS = ("labels", "sizes", "medoids", "medoid_within")


def check(ctx, labs, Dq=None):
    """ctx.profiles(labs) against profiles_ref on ctx's quantised matrix"""
    out = ctx.profiles(labs)
    if Dq is None:
        Dq = quantised(ctx.get_matrix(0), out["eD"])
    for l in range(len(labs)):
        assert R.mismatches(out, l, R.profile(Dq, labs[l])) == [], l
    assert out["kernel_ms"] > 0
    return out, Dq


def same(a, b, rows=slice(None)):
    """two Context.profiles dicts (a: all of it; b: its labellings `rows`) hold the same integers"""
    idx = np.arange(len(b["K"]))[rows]
    ok = all((a[f] is None and b[f] is None) or np.array_equal(a[f], b[f][idx]) for f in INT_FIELDS)
    return ok and a["eD"] == b["eD"] and all(len(a[f]) == len(idx) and all(np.array_equal(x, b[f][l]) for x, l in zip(a[f], idx))
                                             for f in LIST_FIELDS)


@pytest.mark.parametrize("L", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_every_integer_at_every_size_and_width(n, L):
    ctx = context("derived64", n)
    try:
        check(ctx, batch(n, L))
    finally:
        ctx.close()


@pytest.mark.parametrize("L", [3, 65])
@pytest.mark.parametrize("kind,diag", [("stored64", None), ("bits32", None), ("points", None), ("derived64", "mixed"),
                                       ("stored64", "mixed"), ("bits32", "mixed")])
def test_every_kind_of_context_and_a_nonzero_diagonal(kind, diag, L):
    n = 129
    ctx = context(kind, n, diag)
    try:
        _, Dq = check(ctx, batch(n, L, seed=7))
        if diag:   # the context holds it, of both signs, and it is in no sum
            assert Dq.diagonal().min() < 0 < Dq.diagonal().max()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def wide_batch():
    """one context with a mixed-sign diagonal, one batch of 65 labellings at n = 257 and its profiles, checked against the
    reference once and shared by the invariance tests"""
    ctx = context("derived64", 257, "mixed")
    labs = batch(257, 65, seed=5)
    out, _ = check(ctx, labs)
    yield ctx, labs, out
    ctx.close()


def test_rows_in_global_memory_give_the_same_integers(wide_batch, monkeypatch):
    ctx, labs, ref = wide_batch
    monkeypatch.setenv("RC_PROFILE_ROWS_GLOBAL", "1")
    assert same(ctx.profiles(labs), ref)
    assert same(ctx.profiles(labs[:3]), ref, slice(0, 3))


@pytest.mark.parametrize("kib", [64, 4096])
def test_chunks_of_rows_and_labellings_give_the_same_integers(wide_batch, kib, monkeypatch):
    """64 KiB: one labelling per chunk — 65 chunks of labellings — and its rows a dozen at a time or fewer; 4 MiB: the rows
    of a chunk at once, the labellings in several chunks that end where the all-singleton ones (257 slots each) fill it"""
    ctx, labs, ref = wide_batch
    monkeypatch.setenv("RC_PROFILE_WORKSPACE_KIB", str(kib))
    assert same(ctx.profiles(labs), ref)
    medoids_only = ctx.profiles(labs, points=False)
    assert medoids_only["within"] is None and all(np.array_equal(x, y) for x, y in zip(medoids_only["medoids"], ref["medoids"]))


def test_medoids_alone_are_the_same_medoids(wide_batch):
    ctx, labs, ref = wide_batch
    out = ctx.profiles(labs, points=False)
    assert out["within"] is None and out["nearest"] is None and out["neighbour"] is None
    assert np.array_equal(out["K"], ref["K"])
    for f in LIST_FIELDS:
        assert all(np.array_equal(x, y) for x, y in zip(out[f], ref[f])), f
    # one per-point output without the others: the raw call takes any subset
    L, n = labs.shape
    nearest = np.full((L, n), -7, np.int64)
    ctx._chk(ctx.L.rc_cluster_profiles(ctx.h, L, labs.ctypes.data, None, None, None, 0, None, nearest.ctypes.data, None, None, None))
    assert np.array_equal(nearest, ref["nearest"])


def test_a_labelling_profiles_the_same_alone_and_in_any_company(wide_batch):
    ctx, labs, ref = wide_batch
    for l in (0, 17, 64):
        assert same(ctx.profiles(labs[l]), ref, slice(l, l + 1))
    order = np.roll(np.arange(65), 23)                         # labelling order[l] is now at l, among the same others
    assert same(ctx.profiles(labs[order]), ref, order)


def test_1025_labellings_in_one_chunk_take_plain_stores_and_agree_with_batches_of_65(monkeypatch):
    """n = 65, L = 1025 in the default 1 GiB workspace is one chunk of labellings and all 65 rows at once: the planner's recorded
    plan "profiles,65,1025,<pattern>,1048576" is "1025:65*1" at every number of clusters (tests/golden/slab_plans.json, held in
    tests/test_slabplan_cpu.py).  1025 labellings pad to 1088, no fewer than the 1024 lanes of k_predict_sums' workgroup, so a
    lane owns a whole labelling: plain stores into a slab that was never zeroed.  Batches of 65 pad to 128 — 8 parts per
    labelling that add with atomics into zeros, the path the tests above hold against the reference.  Every output (same():
    K, within, nearest, neighbour, labels, sizes, medoids, medoid_within) must be equal."""
    monkeypatch.delenv("RC_PROFILE_WORKSPACE_KIB", raising=False)
    n, L = 65, 1025
    ctx = context("derived64", n, "mixed")
    try:
        labs = batch(n, L)
        whole = ctx.profiles(labs)
        assert whole["within"].shape == (L, n) and len(whole["medoids"]) == L
        for s in range(0, L, 65):
            rows = slice(s, min(s + 65, L))
            assert same(ctx.profiles(labs[rows]), whole, rows), s
    finally:
        ctx.close()


def test_ties_go_to_the_smaller_label_and_the_smallest_index():
    """all off-diagonal entries equal: every other cluster ties in mean, every member ties in within"""
    n = 131
    D = np.full((n, n), 3.0); np.fill_diagonal(D, 0.0)
    ctx = rc.Context(D)
    try:
        rng = np.random.default_rng(2)
        names = np.array([5, 9, 40, 77, 131])
        labs = np.stack([names[rng.integers(0, 5, n)], names[np.arange(n) % 5], rng.permutation(n) + 1,
                         np.where(np.arange(n) < 64, 131, 2)]).astype(np.int64)
        out, Dq = check(ctx, labs)
        q = int(Dq[0, 1])
        assert q > 0 and np.all(Dq[~np.eye(n, dtype=bool)] == q)
        for l, z in enumerate(labs):
            present = np.unique(z)
            for i in range(n):
                assert out["neighbour"][l][i] == present[present != z[i]].min()
            assert list(out["medoids"][l]) == [int(np.flatnonzero(z == k)[0]) + 1 for k in present]
    finally:
        ctx.close()


def test_means_closer_than_a_float_can_tell_are_told_apart():
    """A matrix equal everywhere but for one entry (i0, j0) raised by 2^-40 relative.  Point i0 sits in cluster 1; j0 in
    cluster 2 of 9000 points, whose mean distance to i0 is above that of cluster 3 by q·2^-40/9000 — less than half a float64
    ulp of the mean itself, asserted below from the Python integers: in float64 the two quotients are the same number, and a
    device that compared them would give the tie to cluster 2.  The exact answer is cluster 3.  (9000 > 2^13 members are what
    it takes for 2^-40 to fall below the 2^-53 of a rounding, hence n = 9080; one labelling, a few rows read back.)"""
    sizes = (40, 9000, 40)
    n, i0, j0 = sum(sizes), 7, 40 + 1234
    z = np.repeat([1, 2, 3], sizes).astype(np.int64)
    D = np.ones((n, n)); np.fill_diagonal(D, 0.0)
    D[i0, j0] = D[j0, i0] = 1.0 + 2.0 ** -40
    ctx = rc.Context(D)
    try:
        out = ctx.profiles(z)
        e = out["eD"]
        q = 1 << e
        Dq = np.full((n, n), q, np.int64); np.fill_diagonal(Dq, 0)
        Dq[i0, j0] = Dq[j0, i0] = q + (q >> 40)
        rows = np.array([0, i0, j0, n - 1])
        assert e >= 40 and np.array_equal(quantised(ctx.get_matrix_rows(0, rows), e), Dq[rows])
        S2, S3 = int(Dq[i0, z == 2].sum()), int(Dq[i0, z == 3].sum())
        gap = Fraction(S2, sizes[1]) - Fraction(S3, sizes[2])
        assert 0 < gap < Fraction(math.ulp(S3 / sizes[2])) / 2
        assert float(S2) / sizes[1] == float(S3) / sizes[2] and float(S2) * sizes[2] == float(S3) * sizes[1]
        assert R.mismatches(out, 0, R.profile(Dq, z)) == []
        assert out["neighbour"][0][i0] == 3 and out["nearest"][0][i0] == S3
        assert np.all(np.delete(out["neighbour"][0][:40], i0) == 2)          # exact ties beside it: the smaller label
    finally:
        ctx.close()


def test_cross_products_beyond_64_bits():
    """n = 600, all distances within 10 % of the largest, two clusters of about 300 and — because with two clusters a point has
    one candidate and nothing to compare it with — three of about 200 as well.  The cross-products S·n of the comparison pass
    2^63 (asserted from the quantised integers), so a 64-bit multiply on the device would wrap.  n = 600 is enough on a context
    with a stored logD, whose D uses every bit the int64 row sums allow (eD = 52 here: sums near 2^60); a context that derives
    its logarithms keeps D below 2^47 and reaches only 2^62.3 at this n."""
    n = 600
    rng = np.random.default_rng(12)
    D = rng.uniform(0.9, 1.0, (n, n)); D = np.maximum(D, D.T); np.fill_diagonal(D, 0.0)
    labs = np.stack([rng.integers(1, 3, n), rng.integers(1, 4, n) * 100]).astype(np.int64)
    off = D.copy(); np.fill_diagonal(off, 1.0)
    ctx = rc.Context(D, logD=np.log(off))
    try:
        out, Dq = check(ctx, labs)
        widest = 0
        for l in range(2):
            cnt = dict(zip(out["labels"][l], out["sizes"][l]))
            for i in range(n):
                others = [int(k) for k in cnt if k != labs[l][i] and k != out["neighbour"][l][i]]
                widest = max([widest] + [int(out["nearest"][l][i]) * int(cnt[k]) for k in others])
        assert widest >= 1 << 63, widest
        assert min(int(x) for x in out["nearest"][0]) * int(out["sizes"][0].min()) >= 1 << 63   # so would the two-cluster sums, if compared
    finally:
        ctx.close()


def test_a_context_in_mid_chain_is_left_as_it_was():
    n = 129
    ctx = context("derived64", n)
    try:
        init = np.random.default_rng(3).integers(1, 14, n).astype(np.int64)
        ctx.set_params(**rc.likelihood_hyperparams(matrix(n), points(n, want_truth=True)[1]))
        ctx.set_state(init)
        for t in range(20):
            ctx.gibbs_sweep(1.0 + 0.1 * (t % 3), 0.4, seed=11, sweep_index=t)
            ctx.record_sample(False)
        snapshot = lambda: (ctx.get_state(), ctx.layout_info(), ctx.cocluster_counts(), ctx.bulk_kernel_name())
        before = snapshot()
        assert before[1][0] >= 1 and before[0][2] > 1                   # the points were re-laid out: not the caller's order
        labs = batch(n, 65, seed=2)
        labs[4] = before[0][0]                                          # the chain's own state among them
        check(ctx, labs)
        after = snapshot()
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and before[0][2] == after[0][2]
        assert before[1] == after[1] and np.array_equal(before[2], after[2]) and before[3] == after[3]
    finally:
        ctx.close()


def test_no_state_and_no_params_are_needed():
    ctx = context("points", 65)
    try:
        with pytest.raises(rc.RedClustHIPError, match="RC_ERR_STATE"):
            ctx.score(batch(65, 3))                                     # scoring needs parameters; the profiles do not
        check(ctx, batch(65, 3))
    finally:
        ctx.close()


def test_errors_come_before_any_device_work_and_write_nothing(wide_batch):
    ctx, labs, ref = wide_batch
    n, L = ctx.n, rc.lib()
    ktot = int(ref["K"][:2].sum())

    def raw(nl=2, lab=labs[:2], mlen=ktot, h=ctx.h):
        bufs = [np.full(s, -7, np.int64) for s in (2, max(mlen, 1), max(mlen, 1), (2, n), (2, n), (2, n))]
        eD, ms = C.c_int32(-7), C.c_double(-7.0)
        lab = None if lab is None else np.ascontiguousarray(lab)
        rcode = L.rc_cluster_profiles(h, nl, None if lab is None else lab.ctypes.data, bufs[0].ctypes.data, bufs[1].ctypes.data,
                                      bufs[2].ctypes.data, mlen, bufs[3].ctypes.data, bufs[4].ctypes.data, bufs[5].ctypes.data,
                                      C.byref(eD), C.byref(ms))
        untouched = all(np.all(b == -7) for b in bufs) and eD.value == -7 and ms.value == -7.0
        return rcode, L.rc_last_error(h).decode(), untouched
    rcode, _, untouched = raw()
    assert rcode == 0 and not untouched
    bad = labs[:2].copy(); bad[1, 7] = n + 1
    zero = labs[:2].copy(); zero[0, 0] = 0
    for kw, code, text in ((dict(lab=zero), -1, "labelling 1 at position 1"), (dict(lab=bad), -1, "labelling 2 at position 8"),
                           (dict(nl=0), -1, "L >= 1"), (dict(lab=None), -1, "NULL"), (dict(mlen=ktot + 1), -1, "medoids_len"),
                           (dict(mlen=0), -1, "medoids_len")):
        rcode, msg, untouched = raw(**kw)
        assert rcode == code and text in msg and untouched, (kw, rcode, msg, untouched)
    assert L.rc_cluster_profiles(None, 2, labs.ctypes.data, None, None, None, 0, None, None, None, None, None) == -1
    assert L.rc_cluster_profiles(ctx.h, 2, labs.ctypes.data, None, None, None, 3, None, None, None, None, None) == -1   # 0 with NULL pointers
    with pytest.raises(rc.RedClustHIPError, match=r"RC_ERR_ARG.*label 258 of labelling 2 at position 8"):
        ctx.profiles(bad)


def test_capacity_is_4096_clusters():
    """4097 clusters at n = 4100: RC_ERR_CAPACITY, named, nothing written; 4096 clusters at the same n work"""
    n = 4100
    ctx = rc.Context.from_points(np.random.default_rng(8).normal(0, 1, (n, 2)))
    try:
        z = np.minimum(np.arange(1, n + 1), 4097).astype(np.int64)
        labs = np.stack([np.ones(n, np.int64), z])
        K = np.full(2, -7, np.int64)
        assert ctx.L.rc_cluster_profiles(ctx.h, 2, labs.ctypes.data, K.ctypes.data, None, None, 0, None, None, None, None, None) == -6
        assert "labelling 2 has 4097 clusters" in ctx.L.rc_last_error(ctx.h).decode() and np.all(K == -7)
        with pytest.raises(rc.RedClustHIPError, match="RC_ERR_CAPACITY"):
            ctx.profiles(labs)
        out = ctx.profiles(np.minimum(z, 4096), points=False)
        assert out["K"][0] == 4096 and list(out["medoids"][0][:4095]) == list(range(1, 4096)) and out["sizes"][0][-1] == 5
        assert not out["medoid_within"][0][:4095].any() and out["medoid_within"][0][4095] > 0
    finally:
        ctx.close()


# ---- the Python layer

@pytest.fixture(scope="module")
def planted():
    """the planted 5-cluster points of test_gpu_score.py at n = 96 (noise 1 against a centre spread of 4), a context of their
    distances and a short chain on it"""
    n = 96
    X, truth = points(n, want_truth=True)
    D = matrix(n)
    P = rc.likelihood_hyperparams(D, truth)
    params = rc.PriorHyperparamsList(**{k: P[k] for k in ("delta1", "delta2", "alpha", "beta", "zeta", "gamma")})
    options = rc.MCMCOptionsList(numiters=40, burnin=10, thin=1, numGibbs=1, numMH=1)
    init = np.random.default_rng(4).integers(1, 11, n).astype(np.int64)
    ctx = rc.Context(D)
    result = rc.runsampler(rc.MCMCData(D), options, params, rc.MCMCState(init, 1.0, 0.5), verbose=False, seed=3, ctx=ctx)
    yield D, truth, ctx, result
    ctx.close()


def test_clusterprofiles_of_a_result_is_the_raw_call(planted):
    D, truth, ctx, result = planted
    S = np.stack([np.asarray(c, np.int64) for c in result.clusts])
    raw = ctx.profiles(S)
    Dq = quantised(ctx.get_matrix(0), raw["eD"])
    for prof in (rc.clusterprofiles(ctx, result), rc.clusterprofiles(rc.MCMCData(D), result), rc.clusterprofiles(D, S)):
        assert len(prof) == len(S) == 30 and same(prof.raw, raw)
        assert np.array_equal(prof.neighbour, raw["neighbour"]) and all(np.array_equal(x, y) for x, y in zip(prof.medoids, raw["medoids"]))
        assert np.array_equal(prof.silhouette, rc.silhouettes_from_sums(raw["within"], raw["nearest"], raw["neighbour"], S))
    for l in (0, 29):
        ref = R.profile(Dq, S[l])
        exact = R.silhouette_exact(ref, S[l])
        assert R.mismatches(raw, l, ref) == []
        assert max(abs(Fraction(float(prof.silhouette[l, i])) - exact[i]) for i in range(96)) <= Fraction(1, 10 ** 12)
        assert abs(prof.mean_silhouette[l] - float(sum(exact) / 96)) <= 1e-12
        for k, name in enumerate(prof.labels[l]):
            members = np.flatnonzero(S[l] == name)
            assert abs(prof.cluster_silhouette[l][k] - float(sum(exact[i] for i in members) / len(members))) <= 1e-12
            pairs = len(members) * (len(members) - 1)
            mean = D[np.ix_(members, members)].sum() / pairs if pairs else 0.0
            assert abs(prof.within_mean[l][k] - mean) <= 1e-9 * max(mean, 1.0)          # D's units: quantisation is far below
    one = rc.clusterprofiles(ctx, S[3])
    assert len(one) == 1 and np.array_equal(one.silhouette[0], prof.silhouette[3])
    idx, s, nb = prof.worst(5, labelling=3)
    assert list(idx) == list(np.argsort(prof.silhouette[3], kind="stable")[:5]) and np.array_equal(s, prof.silhouette[3][idx])
    assert np.array_equal(nb, raw["neighbour"][3][idx]) and np.all(np.diff(s) >= 0)


def test_exemplars_count_every_medoid_once(planted):
    D, truth, ctx, result = planted
    ex = rc.exemplars(ctx, result)
    prof = rc.clusterprofiles(ctx, result)
    assert ex["frequency"].shape == (96,) and ex["frequency"].sum() == int(np.sum(result.K)) == int(prof.raw["K"].sum())
    assert np.array_equal(ex["frequency"], np.bincount(np.concatenate(prof.medoids) - 1, minlength=96))
    assert np.array_equal(ex["probability"], ex["frequency"] / 30) and ex["frequency"].max() <= 30
    assert np.array_equal(ex["silhouette"], prof.silhouette.mean(axis=0)) and ex["mean_silhouette"] == float(prof.mean_silhouette.mean())


def test_hclustpointestimate_by_silhouette_takes_the_best_separated_cut(planted):
    D, truth, ctx, result = planted
    maxK = 12
    cut, info = rc.hclustpointestimate(result, maxK=maxK, criterion="silhouette", data=ctx)
    cuts = [_lib.hclust_cut(info["merges"], 96, K) for K in range(2, maxK + 1)]
    Dq = quantised(ctx.get_matrix(0), ctx.profiles(cut)["eD"])
    ref = [R.mean_silhouette(Dq, z) for z in cuts]
    assert info["mean_silhouette"].shape == (maxK - 1,)
    assert max(abs(float(x) - y) for x, y in zip(ref, info["mean_silhouette"])) <= 1e-12
    best = max(range(len(ref)), key=lambda k: (ref[k], -k))            # the fewest clusters on a tie
    assert sorted(ref)[-1] - sorted(ref)[-2] > 1e-9                      # no near-tie that float and exact could settle apart
    assert info["K"] == best + 2 and np.array_equal(cut, cuts[best]) and len(np.unique(cut)) == info["K"]
    # every existing call keeps its behaviour
    old, oi = rc.hclustpointestimate(result, maxK=maxK)
    assert "mean_silhouette" not in oi and np.array_equal(old, _lib.hclust_cut(oi["merges"], 96, oi["K"]))


def test_the_planted_clusters_are_better_separated_than_random_ones(planted):
    D, truth, ctx, result = planted
    rand = np.random.default_rng(6).integers(1, 6, 96).astype(np.int64)
    prof = rc.clusterprofiles(ctx, np.stack([truth, rand]))
    assert prof.mean_silhouette[0] > 0 and prof.mean_silhouette[0] > prof.mean_silhouette[1]
