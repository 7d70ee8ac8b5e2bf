"""Co-clustering counts from samples on the GPU (csrc/samplecounts.inc.hip through rc_samples_counts,
rc_psm_search_samples, posterior_counts / posterior_coclustering and searchpointestimate's MCMCResult branch).

The counts are exact integers, so every comparison here is bit for bit: against the host NumPy cocluster_counts, against
closed forms, and — for the search entry — against rc_psm_search on the host-built counts.

The kernel's tile is TI × TJ = 128 × 128 and it stages its row labels SC = 32 samples at a time; the sizes below sit on
both sides of every one of those edges, and n = TJ + TI + 3 has three tiles per side, one of them off the diagonal's
neighbours."""
import functools
import types

import numpy as np
import pytest

import psm_search_ref as R
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

TI, TJ, SC = 128, 128, 32
NS = sorted({1, 2, 5, TI - 1, TI, TI + 1, TJ - 1, TJ + 1, TJ + TI + 3})
MS = [1, 2, SC - 1, SC, SC + 1, 2 * SC + 3]
assert max(NS) <= 1200 and max(MS) <= 300


@functools.lru_cache(maxsize=None)
def sparse_samples(n, m):
    """m×n labels drawn from a random subset of 1..n with (at most) 7 elements that includes n: not compact, top label used"""
    rng = np.random.default_rng(1000 * n + m)
    pool = np.append(rng.permutation(np.arange(1, n))[: min(6, n - 1)], n).astype(np.int64)
    S = pool[rng.integers(0, len(pool), size=(m, n))]
    S[rng.integers(0, m), rng.integers(0, n)] = n
    S.setflags(write=False)
    return S


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_counts_equal_the_numpy_reference_bit_for_bit(n, m):
    S = sparse_samples(n, m)
    got, ms = _lib.samples_counts(S)
    ref = rc.cocluster_counts(list(S))
    assert got.dtype == np.uint32 and got.shape == (n, n) and ms >= 0
    assert np.array_equal(got, ref)
    assert np.array_equal(got, got.T) and np.all(np.diag(got) == m)


@pytest.mark.parametrize("n,m", [(1, 3), (TI - 1, SC + 1), (TJ + 1, 2), (TJ + TI + 3, SC)])
def test_all_singletons_give_m_times_the_identity(n, m):
    rng = np.random.default_rng(n + m)
    S = np.stack([rng.permutation(n) + 1 for _ in range(m)]).astype(np.int64)
    got, _ = _lib.samples_counts(S)
    assert np.array_equal(got, m * np.eye(n, dtype=np.uint32))


@pytest.mark.parametrize("n,m,label", [(1, 1, 1), (TI, SC - 1, 1), (TJ + 1, SC + 1, TJ + 1), (TJ + TI + 3, 3, 77)])
def test_one_cluster_gives_m_everywhere(n, m, label):
    got, _ = _lib.samples_counts(np.full((m, n), label, np.int64))
    assert np.array_equal(got, np.full((n, n), m, np.uint32))


def test_counts_above_65535_need_wide_accumulators():
    m, n = 70_000, 8
    lab = np.array([1, 8, 1, 1, 8, 8, 1, 8], np.int64)
    got, _ = _lib.samples_counts(np.tile(lab, (m, 1)))
    ref = (m * (lab[:, None] == lab[None, :])).astype(np.uint32)
    assert ref.max() == m > 65_535
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("loss", [R.BINDER, R.VILB], ids=["binder", "VI"])
def test_search_entry_equals_the_search_of_the_host_counts(loss):
    n, m = 257, 37                                               # ld = 260 != n
    S, _ = R.planted_counts(n, m, 5, 0.2, seed=257)
    C = rc.cocluster_counts(list(S))
    rng = np.random.default_rng(5)
    init = np.stack([np.zeros(n, np.int64)] * 3 + [rng.integers(1, 9, n).astype(np.int64)])
    order = np.stack([rng.permutation(n) + 1 for _ in range(3)] + [np.arange(1, n + 1)]).astype(np.int32)
    ref = _lib.psm_search(C, m, loss, init, order)
    got = _lib.psm_search_samples(S, loss, init, order)
    for k in ("labels", "loss", "loss_num", "sweeps", "moves", "K", "converged"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["best"] == ref["best"]
    assert got["counts_ms"] >= 0 and got["kernel_ms"] >= 0


def test_searchpointestimate_no_longer_builds_counts_on_the_host(monkeypatch):
    n, m = 60, 25
    S, _ = R.planted_counts(n, m, 4, 0.2, seed=60)
    samples = types.SimpleNamespace(clusts=[s.copy() for s in S])
    counts = rc.cocluster_counts(samples.clusts)                 # the real one, before it is taken away

    def refuse(*a, **k):
        raise AssertionError("cocluster_counts was called: the counts were built on the host")

    import redclust_amd.pointestimate as pe
    monkeypatch.setattr(pe, "cocluster_counts", refuse)
    for loss in ("binder", "VI"):
        clust, info = rc.searchpointestimate(samples, loss, nruns=4, seed=11)
        mpel, _ = rc.getpointestimate(samples, "MPEL", loss)
        ref_clust, ref = rc.searchpointestimate(counts, loss, numsamples=m, nruns=4, seed=11, init=[mpel])
        assert np.array_equal(info["labels"], ref["labels"]) and np.array_equal(info["loss"], ref["loss"])
        assert info["best"] == ref["best"] and np.array_equal(clust, ref_clust)
        assert info["counts_ms"] >= 0
    clust, info = rc.searchpointestimate(samples, "VI", nruns=4, seed=11, exact=True)
    assert len(clust) == n and info["lower_bound"]["counts_ms"] >= 0


def test_posterior_of_a_sampler_result():
    n = 64
    rng = np.random.default_rng(64)
    truth = np.repeat(np.arange(1, 5), n // 4)
    pts = rng.normal(size=(n, 2)) + 4.0 * np.stack([np.cos(truth * 1.5), np.sin(truth * 1.5)], axis=1)
    D = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2))
    P = rc.likelihood_hyperparams(D, truth)
    params = rc.PriorHyperparamsList(**{k: P[k] for k in ("delta1", "delta2", "alpha", "beta", "zeta", "gamma")})
    options = rc.MCMCOptionsList(numiters=300, burnin=50, thin=2, numGibbs=1, numMH=0)
    init = rng.integers(1, 9, n).astype(np.int64)
    result = rc.runsampler(rc.MCMCData(D), options, params, rc.MCMCState(init, 1.0, 0.5), verbose=False, seed=5)
    assert len(result.clusts) > 100
    assert np.array_equal(rc.posterior_coclustering(result), result.posterior_coclustering)
    counts = rc.posterior_counts(result)
    assert counts.dtype == np.uint32 and np.array_equal(counts, rc.cocluster_counts(result.clusts))
    assert np.array_equal(rc.posterior_counts(np.stack(result.clusts)), counts)      # a plain label matrix


def test_errors_are_return_codes_and_the_process_goes_on():
    ok = np.array([[1, 2, 2], [3, 3, 1]], np.int64)
    init, order = np.zeros((1, 3), np.int64), np.array([[1, 2, 3]], np.int32)
    for bad in (0, 4):
        S = ok.copy()
        S[1, 2] = bad
        with pytest.raises(rc.RedClustHIPError, match=r"RC_ERR_ARG.*sample 2 at position 3") as e:
            _lib.samples_counts(S)
        assert e.value.code == -1
        with pytest.raises(rc.RedClustHIPError, match=r"RC_ERR_ARG.*sample 2 at position 3"):
            _lib.psm_search_samples(S, R.BINDER, init, order)
    wide = np.ones((1, 8193), np.int64)
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_CAPACITY") as e:
        _lib.psm_search_samples(wide, R.BINDER, np.zeros((1, 8193), np.int64), np.arange(1, 8194, dtype=np.int32)[None, :])
    assert e.value.code == -6
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_CAPACITY.*32767") as e:
        _lib.samples_counts(np.ones((1, 32768), np.int64))
    assert e.value.code == -6
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.samples_counts(ok, device=-1)
    got, _ = _lib.samples_counts(ok)
    assert np.array_equal(got, np.array([[2, 1, 0], [1, 2, 1], [0, 1, 2]], np.uint32))
    res = _lib.psm_search_samples(ok, R.BINDER, init, order)
    assert res["converged"][0] and res["labels"].shape == (1, 3)
