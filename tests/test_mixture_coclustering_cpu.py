"""generatemixture's oracle co-clustering matrix without a GPU: the C ABI entry point and its ctypes binding, the resources of
the product kernel in the gfx950 ISA, the host checks of rc.oracle_coclustering, and the NumPy restatement
(tests/mixture_ref.py) against the reference's literal form and against the matrices the Julia package stored for the
paper datasets (tests/golden/paper_oracle.npz)."""
import os
import re

import numpy as np
import pytest

import isa
import mixture_ref as MR
import redclust_amd as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# paper dataset d: σ, and the bounds on max |Δ| / mean |Δ| against the stored matrix (twice the worst of ten seeds of
# the restatement; equal weights miss them)
PAPER = {1: (0.25, 0.012, 1.2e-4), 2: (0.2, 0.001, 6e-6), 3: (0.18, 4e-5, 1.6e-7)}
PAPER_SEED = 3


def test_header_and_signature_take_twelve_arguments():
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    m = re.search(r"int32_t\s+rc_oracle_coclustering\s*\(([^;]*)\)\s*;", hdr)
    assert m, "rc_oracle_coclustering is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert len(args) == 12, args
    res, argtypes = rc.SIGNATURES["rc_oracle_coclustering"]
    assert len(argtypes) == 12


def test_product_kernel_does_not_spill():
    res = isa.resources()
    hits = [k for k in res if "k_mix_syrk" in k]
    assert len(hits) == 1, sorted(k for k in res if "k_mix" in k)
    assert res[hits[0]]["private_segment_fixed_size"] == 0, res[hits[0]]


X = np.random.default_rng(1).normal(size=(6, 4))
W = np.full((3, 2), 0.5)


@pytest.mark.parametrize("args,kwargs", [
    ((np.zeros(6), 2), {}),                                     # not a matrix
    ((np.zeros((0, 4)), 2), {}),                                # no points
    ((np.zeros((6, 0)), 1), {}),
    ((np.full((6, 4), "a"), 2), {}),
    ((np.zeros(((1 << 16) + 1, 1)), 1), {}),                  # beyond the device bound (2^16)
    ((X, 0), {}), ((X, 5), {}), ((X, 2.0), {}), ((X, True), {}),
    ((np.where(np.eye(6, 4) > 0, np.nan, X), 2), {}),         # non-finite point
    ((np.where(np.eye(6, 4) > 0, np.inf, X), 2), {}),
    ((X * 1e300, 2), dict(sigma=1e-10)),                      # radius·x/σ² overflows
    ((X, 2), dict(alpha=0)), ((X, 2), dict(alpha=-1.0)), ((X, 2), dict(alpha=np.nan)),
    ((X, 2), dict(radius=0)), ((X, 2), dict(radius=-1.0)), ((X, 2), dict(radius=np.inf)),
    ((X, 2), dict(sigma=0)), ((X, 2), dict(sigma=-0.1)), ((X, 2), dict(sigma=np.nan)),
    ((X, 2), dict(numiters=0)), ((X, 2), dict(numiters=2.5)),
    ((X, 2), dict(seed=-1)), ((X, 2), dict(seed=1.5)),
    ((X, 2), dict(weights=np.full((3, 3), 0.5))),             # wrong K
    ((X, 2), dict(weights=np.full(2, 0.5))),
    ((X, 2), dict(weights=np.zeros((0, 2)))),
    ((X, 2), dict(weights=W, numiters=4)),                    # numiters differs from the rows
    ((X, 2), dict(weights=np.array([[0.5, -0.1], [0.5, 0.5], [1, 0]]))),
    ((X, 2), dict(weights=np.array([[0.5, 0.5], [0.0, 0.0], [1, 0]]))),
    ((X, 2), dict(weights=np.array([[0.5, np.nan], [0.5, 0.5], [1, 0]]))),
    ((X, 2), dict(weights=np.array([[0.5, np.inf], [0.5, 0.5], [1, 0]]))),
    ((X, 2), dict(weights=W, alpha=0)),
    ((X, 2), dict(iters_per_chunk=-1)), ((X, 2), dict(iters_per_chunk=1.0)),
    ((X, 2), dict(device=-1)),
])
def test_bad_arguments_raise_before_the_library(monkeypatch, args, kwargs):
    import redclust_amd._lib as L

    def untouched(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "oracle_coclustering", untouched)
    monkeypatch.setattr(L, "lib", untouched)
    with pytest.raises(ValueError):
        rc.oracle_coclustering(*args, **kwargs)


def test_generatemixture_checks_the_flag_path_on_the_host(monkeypatch):
    import redclust_amd._lib as L
    monkeypatch.setattr(L, "oracle_coclustering", lambda *a, **k: (_ for _ in ()).throw(AssertionError("reached")))
    with pytest.raises(ValueError):
        rc.generatemixture(50, 3, seed=1, oracle_coclustering=True, device=-1)
    out = rc.generatemixture(50, 3, seed=1)                  # flag off: no key, the library is never called
    assert "oracle_coclustering" not in out


@pytest.mark.parametrize("dim,sigma", [(8, 0.1), (50, 0.2), (400, 0.3), (500, 0.3), (500, 0.05)])
def test_restatement_equals_the_literal_form(dim, sigma):
    K = 8
    rng = np.random.default_rng(dim)
    labels = rng.integers(0, K, 40)
    pts = rng.normal(0.0, sigma, (40, dim))
    pts[np.arange(40), labels] += 1.0
    for t in range(3):
        w = rng.dirichlet(np.full(K, 2.0))
        if t == 2:
            w[1] = 0.0
        P = MR.posterior(MR.logits(pts, K, 1.0, sigma), w)
        lit = MR.literal_posterior(pts, K, w, 1.0, sigma)
        assert np.all(np.isfinite(P))
        np.testing.assert_allclose(P.sum(axis=1), 1.0, atol=1e-12)
        ok = np.all(np.isfinite(lit), axis=1)
        assert np.abs(P[ok] - lit[ok]).max(initial=0.0) <= 1e-12
        if sigma == 0.05:   # logpdf ≈ 788 at a point's own centre: exp overflows, the literal form is Inf/Inf
            assert not ok.any()
        else:
            assert ok.all()


@pytest.mark.parametrize("d", [1, 2, 3])
def test_restatement_matches_the_stored_paper_oracle(d):
    g = np.load(os.path.join(ROOT, "tests", "golden", "paper_oracle.npz"))
    X, O = g[f"points{d}"], g[f"oracle{d}"]
    sigma, max_tol, mean_tol = PAPER[d]
    R = MR.oracle(X, 10, MR.dirichlet_weights(10, 10.0, 5000, PAPER_SEED), 1.0, sigma)
    e = np.abs(R - O)
    assert e.max() <= max_tol and e.mean() <= mean_tol, (e.max(), e.mean())
    E = np.abs(MR.oracle(X, 10, np.full((5000, 10), 0.1), 1.0, sigma) - O)   # without the Dirichlet draws
    assert E.max() > max_tol and E.mean() > mean_tol, (E.max(), E.mean())
