"""generatemixture's oracle co-clustering matrix on the device (rc_oracle_coclustering, csrc/mixture.inc.hip) against the
NumPy restatement (tests/mixture_ref.py) with teacher-forced weights, its independence from the chunking, the matrices
the Julia package stored for the paper datasets (tests/golden/paper_oracle.npz) and generatemixture's flag."""
import os

import numpy as np
import pytest

import mixture_ref as MR
import redclust_amd as rc
from redclust_amd._lib import oracle_coclustering as device_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAPER = {1: (0.25, 0.012, 1.2e-4), 2: (0.2, 0.001, 6e-6), 3: (0.18, 4e-5, 1.6e-7)}   # as in the CPU test
PAPER_SEED = 3


def mixture(n, K, dim, sigma, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, K, n)
    pts = rng.normal(0.0, sigma, (n, dim))
    pts[np.arange(n), labels] += 1.0
    return pts


def forced_weights(T, K, seed):
    W = np.random.default_rng(seed + 1).dirichlet(np.full(K, 1.5), size=T)
    if K > 1:
        W[::3, 0] = 0.0                 # zero weights: log w = -inf on the device
        W[1::4] *= 7.0                  # rows need not sum to 1
    return W


CASES = [(n, K, T) for n in (1, 2, 17, 100, 129, 1000) for K in (1, 3, 10, 50) for T in (1, 7, 200)]


@pytest.mark.parametrize("n,K,T", CASES)
def test_device_equals_restatement(n, K, T):
    dim = K + 7 * ((n + K + T) % 2)
    pts = mixture(n, K, dim, 0.3, n * 1000 + K * 10 + T)
    W = forced_weights(T, K, n + K + T)
    R = rc.oracle_coclustering(pts, K, radius=1.0, sigma=0.3, weights=W)
    assert R.shape == (n, n) and R.dtype == np.float64
    assert np.array_equal(R, R.T)
    ref = MR.oracle(pts, K, W, 1.0, 0.3)
    assert np.abs(R - ref).max() <= 1e-12
    if K == 1:
        assert np.all(R == 1.0)


def test_rows_at_n8192():
    n, K, T = 8192, 50, 64
    pts = mixture(n, K, K, 0.1, 5)
    W = MR.dirichlet_weights(K, K, T, 11)
    R, ms = device_oracle(pts, K, 1.0, 0.1, W)
    assert ms > 0 and R.min() >= 0.0 and R.max() <= 1.0
    rows = np.random.default_rng(3).choice(n, 32, replace=False)
    assert np.abs(R[rows] - MR.oracle(pts, K, W, 1.0, 0.1, rows=rows)).max() <= 1e-12


@pytest.mark.parametrize("n,K,T", [(129, 3, 7), (2048, 128, 1030)])   # the second plans 512 iterations per chunk: 3 chunks
def test_chunking_and_repeats_give_the_same_bits(n, K, T):
    pts = mixture(n, K, K, 0.3, n)
    W = forced_weights(T, K, n)
    R0 = rc.oracle_coclustering(pts, K, sigma=0.3, weights=W)
    for ipc in (1, 3, 0):
        R = rc.oracle_coclustering(pts, K, sigma=0.3, weights=W, iters_per_chunk=ipc)
        assert np.array_equal(R, R0), ipc
    assert np.array_equal(R0, R0.T)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_paper_datasets_against_the_stored_matrices(d):
    g = np.load(os.path.join(ROOT, "tests", "golden", "paper_oracle.npz"))
    sigma, max_tol, mean_tol = PAPER[d]
    R = rc.oracle_coclustering(g[f"points{d}"], 10, alpha=10, radius=1.0, sigma=sigma, seed=PAPER_SEED)
    e = np.abs(R - g[f"oracle{d}"])
    assert e.max() <= max_tol and e.mean() <= mean_tol, (e.max(), e.mean())
    assert np.abs(R - MR.oracle(g[f"points{d}"], 10, MR.dirichlet_weights(10, 10, 5000, PAPER_SEED), 1.0, sigma)).max() <= 1e-12


def test_generatemixture_flag():
    off = rc.generatemixture(2000, 20, seed=17)
    on = rc.generatemixture(2000, 20, seed=17, oracle_coclustering=True)
    assert set(on) == set(off) | {"oracle_coclustering"}
    for k in off:
        assert np.array_equal(on[k], off[k]), k
    O = on["oracle_coclustering"]
    assert np.array_equal(O, rc.oracle_coclustering(on["points"], 20, alpha=20, radius=1.0, sigma=0.1, seed=17))
    assert O.shape == (2000, 2000) and np.array_equal(O, O.T)
    p = rc.generatemixture(300, 4, seed=2, points_only=True, oracle_coclustering=True, alpha=2.0, sigma=0.3, radius=1.5)
    assert np.array_equal(p["oracle_coclustering"],
                          rc.oracle_coclustering(p["points"], 4, alpha=2.0, radius=1.5, sigma=0.3, seed=2))


def test_library_reports_domain_errors():
    pts = mixture(10, 3, 3, 0.3, 0)
    with pytest.raises(rc.RedClustDomainError):
        device_oracle(pts, 3, 1.0, 0.3, np.zeros((2, 3)))
    with pytest.raises(rc.RedClustDomainError):
        device_oracle(np.where(np.eye(10, 3) > 0, np.nan, pts), 3, 1.0, 0.3, np.ones((2, 3)))
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        device_oracle(pts, 4, 1.0, 0.3, np.ones((2, 4)))
