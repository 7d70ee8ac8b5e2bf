"""Scoring labellings on the device (-m gpu): rc_score_labellings through Context.score and the functions built on it.

Blocks are compared as integers with tests/score_ref.py on the quantised values get_matrix returns, and the log-likelihood and
log-prior bit for bit with set_state + loglik / logprior on a second context of the same data — the route that predates the
entry.  Shapes are the smallest at which the kernels can go wrong: n around the wave and the 64-wide padding of a chunk of
labellings, batch widths below and above a wave (fewer labellings than lanes cut every labelling into parts that add with
atomics; 65 is more than a wave), one cluster, all singletons, two clusters split at a lane boundary, sparse label names,
K ≈ √n.

rc_create refuses a matrix that is not symmetric (RC_ERR_DOMAIN, a rule older than this entry), so the asymmetric case of the
definition — rows in the smaller label, columns in the larger — is pinned on the reference in tests/test_score_cpu.py and here
only as far as a context can hold it: a nonzero, mixed-sign diagonal."""
import ctypes as C
import os

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import score_ref as R
from helpers import with_diagonal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0 = dict(delta1=1.3, delta2=0.9, alpha=4.0, beta=7.0, zeta=3.0, gamma=11.0, eta=2.0, sigma=1.5, u=2.0, v=3.0, repulsion=True, maxK=0)
SIZES = [1, 2, 63, 64, 65, 129, 257]
WIDTHS = [1, 3, 65]


def points(n, seed=0, want_truth=False):
    rng = np.random.default_rng(100 + seed)
    centres = rng.normal(0, 4, (5, 3))
    truth = rng.integers(0, 5, n)
    X = centres[truth] + rng.normal(0, 1, (n, 3))
    return (X, truth.astype(np.int64) + 1) if want_truth else X


def matrix(n, seed=0):
    X = points(n, seed)
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    D = np.maximum(D, D.T)
    np.fill_diagonal(D, 0.0)
    return D


def labelling(n, kind, rng):
    i = np.arange(n)
    if kind == 0:
        return np.ones(n, np.int64)                                              # K = 1
    if kind == 1:
        return rng.permutation(n).astype(np.int64) + 1                           # all singletons, names shuffled
    if kind == 2:
        cut = 64 if n > 64 else max(n // 2, 1)                                   # two clusters split at a lane boundary
        return np.where(i < cut, min(2, n), 1).astype(np.int64)
    if kind == 3:
        names = np.array(sorted({min(3, n), min(7, n), n}), np.int64)            # sparse names
        return names[rng.integers(0, len(names), n)]
    K = max(1, int(round(np.sqrt(n))))
    return rng.permutation(n)[rng.integers(0, K, n)].astype(np.int64) + 1        # K ≈ √n, arbitrary names


def batch(n, L, seed=0):
    rng = np.random.default_rng(1000 * n + L + seed)
    first = int(rng.integers(0, 5))                                              # a batch of one is not always K = 1
    return np.stack([labelling(n, (first + l) % 5, rng) for l in range(L)])


def context(kind, n, diag=None, seed=0):
    D = matrix(n, seed)
    if diag:
        D = with_diagonal(D, diag)
    if kind == "derived64":
        return rc.Context(D)
    off = D.copy(); np.fill_diagonal(off, 1.0)
    if kind == "stored64":
        return rc.Context(D, logD=np.log(off))
    if kind == "bits32":
        return rc.Context(D, logD=np.log(off), storage_bits=32)
    assert kind == "points" and not diag
    return rc.Context.from_points(points(n, seed))


def check(ctx, twin, labs, params=None, seed=0):
    """ctx.score(labs) against score_ref on ctx's quantised matrices and against set_state + loglik / logprior on twin"""
    L, n = labs.shape
    rng = np.random.default_rng(seed)
    r, p = rng.uniform(0.3, 3.0, L), rng.uniform(0.05, 0.95, L)
    out = ctx.score(labs, r, p, params=params, want_blocks=True)
    Dq, Lq = R.quantised(ctx.get_matrix(0), out["eD"]), R.quantised(ctx.get_matrix(1), out["eL"])
    assert not Lq.diagonal().any()
    for l in range(L):
        _, _, sizes = R.clusters(labs[l])
        assert out["K"][l] == len(sizes) and np.array_equal(out["sizes"][l], sizes)
        assert R.values(out["blocks"][l]) == R.block_sums(Dq, Lq, labs[l]), l
        assert np.array_equal(out["blocks"][l], R.halves(Dq, Lq, labs[l])), l
        twin.set_state(labs[l])
        assert out["loglik"][l] == twin.loglik(), (l, out["loglik"][l], twin.loglik())
        assert out["logprior"][l] == twin.logprior(r[l], p[l]), l
        assert out["logposterior"][l] == out["loglik"][l] + out["logprior"][l]
    assert out["kernel_ms"] > 0
    return out


@pytest.mark.parametrize("L", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_blocks_and_loglik_at_every_size_and_width(n, L):
    ctx, twin = context("derived64", n), context("derived64", n)
    try:
        ctx.set_params(**P0); twin.set_params(**P0)
        check(ctx, twin, batch(n, L))
    finally:
        ctx.close(); twin.close()


@pytest.mark.parametrize("L", [3, 65])
@pytest.mark.parametrize("kind,diag", [("stored64", None), ("bits32", None), ("points", None), ("derived64", "mixed"),
                                       ("stored64", "positive"), ("bits32", "mixed")])
def test_every_kind_of_context_and_a_nonzero_diagonal(kind, diag, L):
    n = 129
    ctx, twin = context(kind, n, diag), context(kind, n, diag)
    try:
        ctx.set_params(**P0); twin.set_params(**P0)
        out = check(ctx, twin, batch(n, L, seed=7))
        if diag:   # the diagonal is in the within blocks: dropped, the value would differ
            Dq = R.quantised(ctx.get_matrix(0), out["eD"])
            assert Dq.diagonal().any()
    finally:
        ctx.close(); twin.close()


def test_an_asymmetric_matrix_cannot_reach_a_context():
    D = matrix(8)
    D[1, 2] *= 1.5
    with pytest.raises(rc.RedClustDomainError, match="symmetric"):
        rc.Context(D)


def test_a_context_in_mid_chain_is_left_as_it_was():
    """20 sweeps with moving labels from a scattered start: the layout is not the caller's order, the row-sum pipeline is
    running.  Scoring must read through that layout and leave the state, the layout and the counts alone — and the chain must
    go on exactly as the one of a twin that never scored."""
    n = 129
    ctx, twin, ref = (context("derived64", n) for _ in range(3))
    try:
        init = np.random.default_rng(3).integers(1, 14, n).astype(np.int64)
        PL = rc.likelihood_hyperparams(matrix(n), points(n, want_truth=True)[1])    # the planted clusters are worth keeping
        for c in (ctx, twin):
            c.set_params(**PL)
            c.set_state(init)
            for t in range(20):
                c.gibbs_sweep(1.0 + 0.1 * (t % 3), 0.4, seed=11, sweep_index=t)
                c.record_sample(False)
        assert ctx.layout_info()[0] >= 1                       # scattered labels: the points were re-laid out
        before = (ctx.get_state(), ctx.layout_info(), ctx.cocluster_counts(), ctx.bulk_kernel_name(), ctx.capacity_info())
        assert before[0][2] > 1 and not np.array_equal(before[0][0], init)
        ref.set_params(**PL)
        labs = batch(n, 65, seed=2)
        labs[4] = before[0][0]                                 # the chain's own state among them
        check(ctx, ref, labs)
        after = (ctx.get_state(), ctx.layout_info(), ctx.cocluster_counts(), ctx.bulk_kernel_name(), ctx.capacity_info())
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and before[0][2] == after[0][2]
        assert before[1] == after[1] and np.array_equal(before[2], after[2]) and before[3:] == after[3:]
        for t in range(20, 24):
            for c in (ctx, twin):
                c.gibbs_sweep(1.2, 0.4, seed=11, sweep_index=t)
            assert np.array_equal(ctx.get_state()[0], twin.get_state()[0])
        assert ctx.loglik() == twin.loglik()
    finally:
        for c in (ctx, twin, ref):
            c.close()


def test_no_state_and_no_context_params_are_needed():
    ctx, twin = context("derived64", 65), context("derived64", 65)
    try:
        labs = batch(65, 3)
        with pytest.raises(rc.RedClustHIPError, match="RC_ERR_STATE"):
            ctx.score(labs)
        twin.set_params(**P0)
        check(ctx, twin, labs, params=P0)                      # ctx has neither parameters nor a state
    finally:
        ctx.close(); twin.close()


def test_params_given_are_those_of_a_fresh_context():
    n = 65
    ctx, twin = context("stored64", n), context("stored64", n)
    try:
        ctx.set_params(**P0)
        ctx.set_state(np.ones(n, np.int64))
        other = dict(P0, alpha=2.5, gamma=5.0, delta2=1.7, sigma=0.5, repulsion=False)
        twin.set_params(**other)
        labs = batch(n, 3, seed=1)
        out = check(ctx, twin, labs, params=other)
        own = ctx.score(labs)
        assert not np.array_equal(own["loglik"], out["loglik"])
        twin.set_params(**P0)
        for l in range(3):
            twin.set_state(labs[l])
            assert own["loglik"][l] == twin.loglik()
        # the blocks carry every parameter set: the host entry reproduces both
        for l in range(3):
            for P, ll in ((other, out["loglik"][l]), (P0, own["loglik"][l])):
                assert rc.loglik_from_blocks(out["blocks"][l], out["sizes"][l], n, out["eD"], out["eL"], P) == ll
    finally:
        ctx.close(); twin.close()


@pytest.fixture(scope="module")
def wide_batch():
    """one context, one batch of 65 labellings at n = 129 and its scores under the defaults, shared by the equivalence tests"""
    ctx = context("derived64", 129)
    ctx.set_params(**P0)
    labs = batch(129, 65, seed=5)
    yield ctx, labs, ctx.score(labs, want_blocks=True)
    ctx.close()


def same(a, b):
    return (np.array_equal(a["loglik"], b["loglik"]) and np.array_equal(a["K"], b["K"]) and
            all(np.array_equal(x, y) for x, y in zip(a["blocks"], b["blocks"])))


def test_rows_in_global_memory_give_the_same_integers(wide_batch, monkeypatch):
    ctx, labs, ref = wide_batch
    monkeypatch.setenv("RC_SCORE_ROWS_GLOBAL", "1")
    assert same(ctx.score(labs, want_blocks=True), ref)
    assert same(ctx.score(labs[:3], want_blocks=True), dict(loglik=ref["loglik"][:3], K=ref["K"][:3], blocks=ref["blocks"][:3]))


@pytest.mark.parametrize("kib", [64, 1024])
def test_chunks_of_rows_and_labellings_give_the_same_integers(wide_batch, kib, monkeypatch):
    """64 KiB: one labelling per chunk and a dozen rows at a time; 1 MiB: a few labellings per chunk, rows in several chunks"""
    ctx, labs, ref = wide_batch
    monkeypatch.setenv("RC_SCORE_WORKSPACE_KIB", str(kib))
    assert same(ctx.score(labs, want_blocks=True), ref)


def test_a_labelling_scores_the_same_alone_and_in_any_company(wide_batch):
    ctx, labs, ref = wide_batch
    for l in (0, 17, 64):
        alone = ctx.score(labs[l], want_blocks=True)
        assert alone["loglik"][0] == ref["loglik"][l] and np.array_equal(alone["blocks"][0], ref["blocks"][l])
    moved = np.roll(labs, 23, axis=0)                           # labelling l is now at (l + 23) % 65, among the same others
    out = ctx.score(moved, want_blocks=True)
    assert same(out, dict(loglik=np.roll(ref["loglik"], 23), K=np.roll(ref["K"], 23), blocks=ref["blocks"][-23:] + ref["blocks"][:-23]))


def test_1025_labellings_in_one_chunk_take_plain_stores_and_agree_with_batches_of_65(monkeypatch):
    """n = 65, L = 1025 in the default 1 GiB workspace is one chunk of labellings and all 65 rows at once: the planner's recorded
    plan "score,65,1025,<pattern>,1048576" is "1025:65*1" at every number of clusters (tests/golden/slab_plans.json, held in
    tests/test_slabplan_cpu.py).  1025 labellings pad to 1088, no fewer than the 1024 lanes of k_predict_sums' workgroup, so a
    lane owns a whole labelling: plain stores into a slab that was never zeroed.  Batches of 65 pad to 128 — 8 parts per
    labelling that add with atomics into zeros, the path the tests above hold against the reference.  Every output must be
    equal."""
    monkeypatch.delenv("RC_SCORE_WORKSPACE_KIB", raising=False)
    n, L = 65, 1025
    ctx = context("derived64", n)
    try:
        ctx.set_params(**P0)
        labs = batch(n, L)
        rng = np.random.default_rng(9)
        r, p = rng.uniform(0.3, 3.0, L), rng.uniform(0.05, 0.95, L)
        whole = ctx.score(labs, r, p, want_blocks=True)
        assert len(whole["blocks"]) == L and len(whole["sizes"]) == L
        for s in range(0, L, 65):
            e = min(s + 65, L)
            part = ctx.score(labs[s:e], r[s:e], p[s:e], want_blocks=True)
            for key in ("loglik", "logprior", "K"):
                assert np.array_equal(part[key], whole[key][s:e]), (key, s)
            for key in ("blocks", "sizes"):
                assert all(np.array_equal(x, y) for x, y in zip(part[key], whole[key][s:e])), (key, s)
    finally:
        ctx.close()


def test_argument_errors_come_before_any_device_work(wide_batch):
    ctx, labs, _ = wide_batch
    n = ctx.n
    L = rc.lib()
    ll = np.zeros(4)

    def raw(nl=2, lab=labs[:2], r=None, p=None, out=ll, lp=None, blocks=None, blen=0):
        keep = [np.ascontiguousarray(x, dtype=np.float64) if x is not None else None for x in (r, p)]
        rcode = L.rc_score_labellings(ctx.h, nl, None if lab is None else np.ascontiguousarray(lab).ctypes.data,
                                      None if keep[0] is None else keep[0].ctypes.data, None if keep[1] is None else keep[1].ctypes.data,
                                      None, None if out is None else out.ctypes.data, None if lp is None else lp.ctypes.data, None,
                                      None if blocks is None else blocks.ctypes.data, blen, None, None, None)
        return rcode, L.rc_last_error(ctx.h).decode()
    assert raw()[0] == 0
    bad = labs[:2].copy(); bad[1, 7] = n + 1
    zero = labs[:2].copy(); zero[0, 0] = 0
    for kw, code, text in ((dict(lab=None), -1, "NULL"), (dict(out=None), -1, "NULL"), (dict(nl=0), -1, "L >= 1"),
                           (dict(lab=bad), -1, "labelling 2 at position 8"), (dict(lab=zero), -1, "labelling 1 at position 1"),
                           (dict(r=[1.0, 0.0], p=[0.5, 0.5]), -1, "r of labelling 2"),
                           (dict(r=[np.inf, 1.0], p=[0.5, 0.5]), -1, "r of labelling 1"),
                           (dict(r=[1.0, 1.0], p=[0.5, 1.0]), -1, "p of labelling 2"),
                           (dict(lp=np.zeros(2)), -1, "needs r and p"),
                           (dict(blen=5), -1, "blocks_len"), (dict(blocks=np.zeros((4, 4), np.int64), blen=1), -1, "blocks_len")):
        rcode, msg = raw(**kw)
        assert rcode == code and text in msg, (kw, rcode, msg)
    with pytest.raises(rc.RedClustHIPError, match="must be positive"):
        ctx.score(labs[:2], params=dict(P0, zeta=-1.0))


def test_capacity_at_the_boundary():
    """4097 clusters: RC_ERR_CAPACITY, and nothing was launched (no kernel time is reported, the error names the labelling);
    4096 clusters work and agree with set_state + loglik"""
    X = np.random.default_rng(8).normal(0, 1, (4097, 2))
    ctx = rc.Context.from_points(X)
    try:
        ctx.set_params(**P0)
        labs = np.stack([np.ones(4097, np.int64), np.arange(1, 4098)])
        with pytest.raises(rc.RedClustHIPError, match=r"RC_ERR_CAPACITY.*labelling 2 has 4097 clusters"):
            ctx.score(labs)
    finally:
        ctx.close()
    ctx, twin = rc.Context.from_points(X[:4096]), rc.Context.from_points(X[:4096])
    try:
        ctx.set_params(**P0); twin.set_params(**P0)
        z = np.arange(1, 4097)
        out = ctx.score(z, 1.0, 0.5)
        twin.set_state(z)
        assert out["K"][0] == 4096 and out["loglik"][0] == twin.loglik() and out["logprior"][0] == twin.logprior(1.0, 0.5)
    finally:
        ctx.close(); twin.close()


def test_end_to_end_at_n96():
    d = np.load(os.path.join(ROOT, "tests", "golden", "paper_datasets.npz"))
    D, truth = np.ascontiguousarray(d["D1"][:96, :96]), d["labels1"][:96]
    P = rc.likelihood_hyperparams(D, truth)
    params = rc.PriorHyperparamsList(**{k: P[k] for k in ("delta1", "delta2", "alpha", "beta", "zeta", "gamma")})
    options = rc.MCMCOptionsList(numiters=40, burnin=10, thin=1, numGibbs=1, numMH=1)
    init = np.random.default_rng(4).integers(1, 11, 96).astype(np.int64)
    data = rc.MCMCData(D)
    ctx = rc.Context(D)
    try:
        result = rc.runsampler(data, options, params, rc.MCMCState(init, 1.0, 0.5), verbose=False, seed=3, ctx=ctx)
        assert len(result.clusts) == 30
        sc = rc.scorelabellings(ctx, result)                    # the context's parameters, the result's r and p
        assert np.array_equal(sc["loglik"], result.loglik) and np.array_equal(sc["logposterior"], result.logposterior)
        assert np.array_equal(sc["K"], result.K)
        # from the data instead of the context: a context of its own, the result's parameters
        sd = rc.scorelabellings(data, result)
        assert np.array_equal(sd["loglik"], result.loglik) and np.array_equal(sd["logposterior"], result.logposterior)
        # candidates of every kind: the MAP sample, a search result, 16 cuts of the dendrogram
        rbar, pbar = float(np.mean(result.r)), float(np.mean(result.p))
        mapc, _ = rc.getpointestimate(result, method="MAP")
        srch, _ = rc.searchpointestimate(result, "VI", nruns=2, seed=1)
        h = rc.hclust(result)
        cuts = [_lib.hclust_cut(h["merges"], 96, K) for K in range(1, 17)]
        cands = [mapc, srch] + cuts
        best, info = rc.mapestimate(ctx, cands, None, rbar, pbar)
        assert info["logposterior"].shape == (18,) and info["index"] == int(np.argmax(info["logposterior"]))
        assert np.array_equal(best, cands[info["index"]])
        for i, z in enumerate(cands):                           # the scores it reports are those of set_state + loglik
            ctx.set_state(z)
            assert info["loglik"][i] == ctx.loglik() and info["logprior"][i] == ctx.logprior(rbar, pbar)
        cut, hi = rc.hclustpointestimate(result, maxK=16, criterion="posterior", data=ctx, r=rbar, p=pbar)
        assert np.array_equal(hi["logposterior"], info["logposterior"][2:])
        assert hi["K"] == int(np.argmax(hi["logposterior"])) + 1 and np.array_equal(cut, cuts[hi["K"] - 1])
        # every existing call keeps its behaviour
        old, oi = rc.hclustpointestimate(result, maxK=16)
        assert np.array_equal(old, cuts[oi["K"] - 1]) and "logposterior" not in oi
        # reweighting: the same parameters change nothing; others agree with scoring under them
        w = rc.reweight(ctx, result, result.params)
        assert np.array_equal(w["weights"], np.full(30, 1 / 30)) and w["ess"] == 30
        other = rc.PriorHyperparamsList(**dict(params.as_dict(), alpha=params.alpha * 1.2, u=2.0))
        w = rc.reweight(ctx, result, other)
        so = rc.scorelabellings(ctx, result, other)
        lw = so["logposterior"] - result.logposterior
        ref = np.exp(lw - lw.max()); ref /= ref.sum()
        assert np.allclose(w["weights"], ref, rtol=1e-9, atol=0) and 1 <= w["ess"] <= 30
    finally:
        ctx.close()
