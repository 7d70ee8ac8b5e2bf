"""CPU checks of the k-means layer: the NumPy restatement of the device k-means (tests/kmeans_ref.py) is a fixed point of
its own definitions (checked without its loop), Clustering.jl's rules (k = 1, maxiter = 0, the repicking of an empty
group, the failing draw with duplicate points), the C ABI of the new entry points and the unchanged refusal of the
string "k-means"."""
import os
import re

import numpy as np
import pytest

import kmeans_ref as KM
import redclust_amd as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The group of the first centre (point 1) loses both its members, points 1 and 7, in the first reassignment: the second
# update has to repick it
HAND = np.array([[2, 8], [1, 2], [1, 8], [6, 6], [3, 8], [1, 4], [2, 4], [3, 9], [5, 0]], dtype=np.float64)
HAND_INIT = [1, 3, 4, 5]


def blobs(rng, n, dim, K):
    return rng.normal(size=(n, dim)) + 6.0 * rng.integers(0, K, n)[:, None] * np.eye(dim)[rng.integers(0, dim)]


def check_fixed_point(X, res, k):
    """The result against the definitions, each computed here without kmeans_ref's helpers."""
    n, dim = X.shape
    M, a = res["centers"], res["assignments"] - 1
    assert M.shape == (k, dim) and a.shape == (n,)
    # distances: ascending coordinates, (x - m)·(x - m) added term by term
    d = np.zeros((n, k))
    for i in range(n):
        for j in range(k):
            acc = 0.0
            for c in range(dim):
                t = X[i, c] - M[j, c]
                acc = acc + t * t
            d[i, j] = acc
    for i in range(n):   # argmin with the lowest-index tie rule
        best, bi = d[i, 0], 0
        for j in range(1, k):
            if d[i, j] < best:
                best, bi = d[i, j], j
        assert a[i] == bi and res["costs"][i] == best
    assert np.array_equal(res["counts"], np.array([(a == g).sum() for g in range(k)]))
    p = [0.0] * 256   # the objective's order
    for i in range(n):
        p[i % 256] = p[i % 256] + res["costs"][i]
    h = 128
    while h:
        for i in range(h):
            p[i] = p[i] + p[i + h]
        h //= 2
    assert res["totalcost"] == p[0]
    if res["converged"] and res["repicks"] == 0:   # centres are the ordered means of the groups they produce
        for g in range(k):
            idx = [i for i in range(n) if a[i] == g]
            s = X[idx[0]].copy()
            for i in idx[1:]:
                s = s + X[i]
            assert np.array_equal(M[g], s / float(len(idx)))


@pytest.mark.parametrize("n,dim,k,seed", [(40, 2, 3, 0), (65, 3, 5, 1), (30, 1, 4, 2), (50, 5, 1, 3), (24, 2, 24, 4),
                                          (37, 4, 18, (1 << 40) + 5)])
def test_restatement_is_a_fixed_point_of_its_definitions(n, dim, k, seed):
    X = blobs(np.random.default_rng(seed % 1000), n, dim, 3)
    res = KM.kmeans(X, k, maxiter=200, seed=seed)
    assert res["converged"]
    check_fixed_point(X, res, k)


def test_k1_converges_at_t1_and_maxiter0_returns_the_initial_assignment():
    X = blobs(np.random.default_rng(7), 33, 3, 2)
    r = KM.kmeans(X, 1, seed=3)
    assert r["iterations"] == 1 and r["converged"]
    assert np.array_equal(r["centers"][0], np.cumsum(X, axis=0)[-1] / 33.0)
    r = KM.kmeans(X, 4, maxiter=0, seed=3)
    assert r["iterations"] == 0 and not r["converged"]
    assert all(any(np.array_equal(m, x) for x in X) for m in r["centers"])   # still the seed points
    check_fixed_point(X, r, 4)


def test_seeds_are_distinct_and_follow_the_stream():
    X = blobs(np.random.default_rng(8), 50, 2, 3)
    a = KM.kmeans(X, 50, maxiter=0, seed=11)
    assert sorted(a["assignments"]) == list(range(1, 51)) and a["totalcost"] == 0.0   # 50 distinct seeds
    b = KM.kmeans(X, 6, maxiter=0, seed=12)
    c = KM.kmeans(X, 6, maxiter=0, seed=12 + (1 << 32))   # the high key word matters
    assert not np.array_equal(b["centers"], c["centers"])


def test_empty_group_is_repicked_hand_case():
    res = KM.kmeans(HAND, 4, init=HAND_INIT, seed=0)
    assert res["repicks"] >= 1
    assert res["converged"] and np.all(res["counts"] > 0) and len(res["counts"]) == 4
    check_fixed_point(HAND, res, 4)
    # plain Lloyd from the same start does lose a group at the first reassignment
    M = HAND[np.array(HAND_INIT) - 1]
    a = np.argmin(((HAND[:, None, :] - M[None]) ** 2).sum(-1), axis=1)
    M = np.array([HAND[a == g].mean(0) for g in range(4)])
    a = np.argmin(((HAND[:, None, :] - M[None]) ** 2).sum(-1), axis=1)
    assert np.bincount(a, minlength=4).min() == 0


def test_identical_points_are_a_domain_error():
    X = np.ones((4, 2))
    with pytest.raises(ValueError):
        KM.kmeans(X, 2, seed=0)
    assert KM.kmeans(X, 1, seed=0)["totalcost"] == 0.0


def test_draw_shift_keeps_the_integer_weights_in_range():
    for scale in (1e-150, 1e-3, 1.0, 1e6, 1e150):
        X = blobs(np.random.default_rng(1), 100, 3, 3) * scale
        s = KM.draw_shift(X)
        w = KM.sqdist(X, X[:1])[:, 0]
        q = np.floor(np.ldexp(w, s))
        assert q.max() * len(X) < 2.0 ** 63 and q.max() >= 2.0 ** 40   # no overflow, and resolution to spare


def test_kmeans_prototypes_are_bound():
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    for name, nargs in (("rc_kmeans", 13), ("rc_kmeans_scan", 10), ("rc_kmeans_scan_split", 11)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        assert len(args) == nargs and len(rc.SIGNATURES[name][1]) == nargs, name


def test_public_names_and_result_type():
    for name in ("kmeans", "fitprior_kmeans", "fitprior2_kmeans", "KmeansResult"):
        assert hasattr(rc, name), name
    assert [f for f in rc.KmeansResult.__dataclass_fields__] == ["centers", "assignments", "costs", "counts", "totalcost",
                                                                  "iterations", "converged"]
    assert callable(rc.Context.kmeans) and callable(rc.Context.kmeans_scan)


def test_kmeans_string_still_raises_not_implemented():
    pts = np.random.default_rng(0).normal(size=(12, 2))
    for fn in (rc.fitprior, rc.fitprior2):
        with pytest.raises(NotImplementedError, match="k-medoids"):
            fn(pts, "k-means", verbose=False)


def test_new_fits_refuse_dissimilarities_before_touching_a_device():
    data = rc.MCMCData(np.abs(np.subtract.outer(np.arange(6.0), np.arange(6.0))))   # dissimilarities only
    for fn in (rc.fitprior_kmeans, rc.fitprior2_kmeans):
        with pytest.raises(ValueError, match="k-means"):
            fn(data, verbose=False)
    pts = np.random.default_rng(0).normal(size=(12, 2))
    for fn in (rc.fitprior_kmeans, rc.fitprior2_kmeans):
        with pytest.raises(ValueError, match="Kmin and Kmax"):
            fn(pts, Kmin=5, Kmax=3, verbose=False)
