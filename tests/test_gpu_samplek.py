"""sampleK on the device (rc_sample_k, csrc/samplek.inc.hip) against the NumPy restatement (tests/samplek_ref.py): the same
K for every sample whose restated top-two score gap is at least 1e-8 (the two evaluate lgamma and log with different
libraries), the law of the draw against softmax(lp), and independence from how the samples are split into launches."""
import numpy as np
import pytest

import samplek_ref as SR
import redclust_amd as rc
from redclust_amd._lib import sample_k

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,m", [(1, 500), (2, 3000), (37, 3000), (500, 3000), (4096, 2000)])
def test_device_draws_equal_restatement(n, m):
    seed = 2 ** 35 + n
    rng = np.random.default_rng(n)
    r = rng.gamma(2.0, 1 / 1.5, m)
    p = rng.beta(2.0, 3.0, m)
    K, ms = sample_k(n, r, p, seed=seed)
    assert K.dtype == np.int64 and K.shape == (m,) and K.min() >= 1 and K.max() <= n and ms > 0
    skipped = 0
    for i in range(m):
        k, gap = SR.draw(n, r[i], p[i], seed, i)
        if gap < 1e-8:
            skipped += 1
            continue
        assert K[i] == k, (i, K[i], k, gap)
    assert skipped <= 0.001 * m, skipped


def test_degenerate_rows():
    r = np.array([1.5, 1.5, 0.0, 2.0])
    p = np.array([1.0, 0.0, 0.4, 0.5])
    K, _ = sample_k(9, r, p, seed=1)
    assert list(K[:3]) == [1, 9, 9]                            # p = 1: no finite score; p = 0 / r = 0: only lp[n] is finite
    assert K[3] == SR.draw(9, 2.0, 0.5, 1, 3)[0]


def test_frequencies_follow_softmax():
    n, r0, p0, m = 12, 2.5, 0.35, 60000
    K, _ = sample_k(n, np.full(m, r0), np.full(m, p0), seed=77)
    lp = SR.logprobs(n, r0, p0)
    prob = np.exp(lp - lp.max())
    prob /= prob.sum()
    freq = np.bincount(K, minlength=n + 1)[1:] / m
    assert np.all(np.abs(freq - prob) < 4 * np.sqrt(prob * (1 - prob) / m) + 1e-4), (freq, prob)


def test_prefix_of_a_longer_call():
    n = 1 << 16                                                 # 16384 samples per launch: the long call takes three
    rng = np.random.default_rng(5)
    r, p = rng.gamma(1.0, 1.0, 40000), rng.beta(1.0, 4.0, 40000)
    long, _ = sample_k(n, r, p, seed=9)
    short, _ = sample_k(n, r[:1000], p[:1000], seed=9)
    assert np.array_equal(long[:1000], short)
    tail, _ = sample_k(n, r[:20000], p[:20000], seed=9)
    assert np.array_equal(long[:20000], tail)


def test_samplek_public_function():
    P = rc.PriorHyperparamsList(eta=3.0, sigma=2.0, u=2.0, v=5.0)
    a = rc.sampleK(P, 5000, 60, seed=4)
    b = rc.sampleK(3.0, 2.0, 2.0, 5.0, 5000, 60, seed=4)
    assert np.array_equal(a, b) and a.dtype == np.int64 and a.min() >= 1 and a.max() <= 60
    rng = np.random.default_rng(4)
    r, p = rng.gamma(3.0, 0.5, 5000), rng.beta(2.0, 5.0, 5000)
    assert np.array_equal(a, sample_k(60, r, p, seed=4)[0])
