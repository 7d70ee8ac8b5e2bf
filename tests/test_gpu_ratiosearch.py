"""The ratio-loss search on the GPU (k_ratiosearch<PQ, LOSS> of csrc/ratiosearch.inc.hip through rc_ratio_search and searchratio):
omARI, NVI and NID.  A run is int64 state and one correctly rounded f64 division per sample and candidate, so the device is held
to tests/ratio_search_ref.py bit for bit, the reference being handed the library's own table."""
import functools

import numpy as np
import pytest

import psm_search_ref as R
import ratio_search_ref as Q
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

KEYS = ("sweeps", "converged", "moves", "K", "loss_num")
# (n, m, planted K, maxK): R > m with a cap of 37 slots (40 padded); m on both sides of the PQ 1 → 4 boundary at 1024, the second
# with maxK = 3 binding and no multiple of 4; PQ = 0
SHAPES = {"n37-m5": (37, 5, 4, 0), "n67-m1000": (67, 1000, 5, 0), "n67-m1030-maxK3": (67, 1030, 5, 3), "n12-m4100": (12, 4100, 3, 0)}


@functools.lru_cache(maxsize=None)
def problem(shape):
    """the samples — among them one of all singletons and one of a single cluster, which make den = 0 where a run stands at the
    same partition — and five runs: from empty labels, from one cluster, from singletons (where the cap allows), from a
    round-robin start, and the first again"""
    n, m, K, maxK = SHAPES[shape]
    S, _ = R.planted_counts(n, m, K, 0.25, seed=n + m)
    S[1], S[2] = np.arange(1, n + 1), 1
    rng = np.random.default_rng(n * m)
    order = np.stack([rng.permutation(n) + 1, np.arange(1, n + 1), np.arange(n, 0, -1), rng.permutation(n) + 1]).astype(np.int32)
    init = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), np.arange(n) % (maxK or n) + 1, np.arange(n) % 3 + 1])
    init, order = np.concatenate([init, init[:1]]), np.concatenate([order, order[:1]])
    for a in (S, init, order):
        a.setflags(write=False)
    return S, init, order, maxK


@functools.lru_cache(maxsize=None)
def library_table(n):
    return _lib.vi_gtable(n)


@pytest.mark.parametrize("loss", Q.LOSSES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_search_equals_the_reference_bit_for_bit(shape, loss):
    n = SHAPES[shape][0]
    S, init, order, maxK = problem(shape)
    got = _lib.ratio_search(S, loss, init, order, maxK=maxK)
    refs = [Q.ratio_search_ref(S, library_table(n), loss, init[r], order[r], maxK=maxK) for r in range(4)]
    refs.append(refs[0])
    for r, ref in enumerate(refs):
        print(shape, loss, r, "sweeps", got["sweeps"][r], "moves", got["moves"][r], "K", got["K"][r], "Q", got["loss_num"][r], ref["loss_num"])
        assert np.array_equal(got["labels"][r], ref["labels"]), (r, got["labels"][r], ref["labels"])
        for k in KEYS:
            assert got[k][r] == ref[k], (r, k, got[k][r], ref[k])
        assert got["loss"][r] == ref["loss_num"] / (2.0 ** 40 * S.shape[0])
        assert maxK == 0 or got["K"][r] <= maxK
    assert got["best"] == int(np.argmin([ref["loss_num"] for ref in refs])) != 4      # the first of two identical runs


@pytest.mark.parametrize("loss", Q.LOSSES)
def test_largest_n_returns_its_own_criterion_at_a_local_optimum(loss):
    n, m, K = 8192, 8, 50
    rng = np.random.default_rng(8192)
    truth = rng.integers(1, K + 1, n)
    S = np.tile(truth, (m, 1)).astype(np.int64)
    flip = rng.random((m, n)) < 0.2
    S[flip] = rng.integers(1, K + 1, int(flip.sum()))
    got = _lib.ratio_search(S, loss, np.zeros((1, n), np.int64), (rng.permutation(n) + 1).astype(np.int32)[None, :])
    c, G = got["labels"][0], library_table(n)
    q = Q.q_direct(c, S, G, loss)
    assert got["converged"][0] and q == int(got["loss_num"][0])
    Kc = int(c.max())
    for i in rng.choice(n, 32, replace=False):
        alone = int((c == c[i]).sum()) == 1
        for l in [l for l in range(1, Kc + 1) if l != c[i]] + ([Kc + 1] if Kc < K and not alone else []):
            x = c.copy()
            x[i] = l
            assert Q.q_direct(x, S, G, loss) >= q, (i, l)


@pytest.mark.parametrize("loss", Q.LOSSES)
def test_searchratio_is_never_worse_than_its_seeded_start(loss):
    n, m, nruns = 65, 40, 4
    S, _ = R.planted_counts(n, m, 6, 0.35, seed=65)
    clust, info = rc.searchratio(S, loss, nruns=nruns, seed=5, init=[np.arange(n) % 2 + 1])
    G = library_table(n)
    qbest = int(info["loss_num"][info["best"]])
    print(loss, "searchratio Q", qbest, "its seeded start's Q", info["start_loss_num"], "runs", info["loss_num"])
    assert len(info["loss_num"]) == nruns + 2 and np.array_equal(clust, info["labels"][info["best"]])
    assert qbest == Q.q_direct(clust, S, G, loss) == min(int(x) for x in info["loss_num"])
    start = info["start"]["labels"][info["start"]["best"]]                      # of searchmaxpear / the exact VI / the ID search
    assert info["start_loss_num"] == Q.q_direct(start, S, G, loss) and qbest <= info["start_loss_num"]


def test_omari_search_improves_on_the_pear_optimum():
    """n = 7, m = 7: by brute force over the 877 partitions (on the host, with pearfraction) PEAR has the single maximiser
    1112222, and tests/ratio_search_ref.py started there lowers Q from 4419410882230 to 4390662733383 — the two criteria differ"""
    S, _ = R.planted_counts(7, 7, 3, 0.35, seed=0)
    clust, info = rc.searchratio(S, "omARI", nruns=4, seed=0)
    start = info["start"]["labels"][info["start"]["best"]]
    assert np.array_equal(R.sortlabels(start), [1, 1, 1, 2, 2, 2, 2]) and info["start_loss_num"] == 4419410882230
    assert int(info["loss_num"][info["best"]]) <= 4390662733383 < info["start_loss_num"]
    assert int(info["loss_num"][info["best"]]) == Q.q_direct(clust, S, library_table(7), "omARI")
