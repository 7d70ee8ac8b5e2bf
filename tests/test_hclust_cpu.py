"""The hierarchical point estimates without a GPU: the NumPy restatement (tests/hclust_ref.py) against the definition
scanned literally, against psm_search_ref's Binder numerator and against SciPy where SciPy's answer does not depend on how
ties are broken; the host-only pieces of the library (rc_hclust_cut, the linkage matrix, the leaf order); and the
header / SIGNATURES / Julia consistency."""
import functools
import os

import numpy as np
import pytest

import hclust_ref as H
import psm_search_ref as R
import redclust_amd as rc
from redclust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, m, K, noise): ties everywhere (noise 0: every count is 0 or m), zero-similarity merges, singletons planted, a plain one
SHAPES = [(1, 3, 1, 0.0), (2, 3, 2, 0.0), (40, 7, 4, 0.0), (33, 5, 33, 0.5), (48, 3, 2, 0.4), (65, 50, 5, 0.2)]
LINKS = [H.AVERAGE, H.COMPLETE, H.SINGLE]
NAMES = {v: k for k, v in H.LINKAGES.items()}


@functools.lru_cache(maxsize=None)
def reference(shape, linkage):
    n, m, K, noise = shape
    _, C = R.planted_counts(n, m, K, noise, seed=2000 + n)
    C.setflags(write=False)
    return C, H.hclust_ref(C, m, linkage)


@pytest.mark.parametrize("linkage", LINKS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"n{s[0]}" for s in SHAPES])
def test_cached_reference_equals_the_literal_definition(shape, linkage):
    C, ref = reference(shape, linkage)
    naive = H.hclust_naive(C, shape[1], linkage)
    assert ref["merges"].tobytes() == naive["merges"].tobytes()
    assert np.array_equal(ref["binder_num"], naive["binder_num"])
    mg = ref["merges"]
    assert np.all(mg["a"] < mg["b"]) and len(mg) == shape[0] - 1
    if shape[0] > 1:
        assert mg["size"][-1] == shape[0] and mg["a"][-1] == 1


@pytest.mark.parametrize("linkage", LINKS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"n{s[0]}" for s in SHAPES])
def test_binder_curve_and_cuts(shape, linkage):
    n, m, K, _ = shape
    C, ref = reference(shape, linkage)
    for k in sorted({1, min(2, n), min(3, n), min(K, n), n // 2 + 1, n}):
        c = H.cut(ref["merges"], n, k)
        assert len(np.unique(c)) == k and np.array_equal(c, R.sortlabels(c))           # cuts come out sortlabels'd
        assert int(ref["binder_num"][n - k]) == R.binder_num(c, C, m) == H.binder_num_from_T(c, C, m), k
        assert np.array_equal(_lib.hclust_cut(ref["merges"], n, k), c), k              # the library's host-only cut
    if shape[3] == 0.0 and n > 2:                                                       # noise 0: the planted partition is a cut
        truth = R.sortlabels(R.planted_counts(n, m, K, 0.0, seed=2000 + n)[0][0])
        assert np.array_equal(H.cut(ref["merges"], n, int(truth.max())), truth)


def test_the_three_linkages_differ():
    C, _ = reference(SHAPES[-1], H.AVERAGE)
    runs = [reference(SHAPES[-1], l)[1]["merges"].tobytes() for l in LINKS]
    assert len(set(runs)) == 3


def test_cut_rejects_what_is_not_a_merge_sequence():
    _, ref = reference(SHAPES[-1], H.AVERAGE)
    n = SHAPES[-1][0]
    for K in (0, n + 1):
        with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
            _lib.hclust_cut(ref["merges"], n, K)
    bad = ref["merges"].copy()
    bad[1] = bad[0]                                                                     # b is no longer active
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.hclust_cut(bad, n, 1)
    swapped = ref["merges"].copy()
    swapped["a"][0], swapped["b"][0] = swapped["b"][0], swapped["a"][0]
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.hclust_cut(swapped, n, 1)
    assert np.array_equal(_lib.hclust_cut(ref["merges"], n, n), np.arange(1, n + 1))


@pytest.mark.parametrize("linkage", LINKS)
def test_linkage_matrix_and_leaf_order(linkage):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    shape = SHAPES[-1]
    n, m = shape[0], shape[1]
    _, ref = reference(shape, linkage)
    Z = rc.linkage_matrix(ref["merges"], m, NAMES[linkage])
    assert hier.is_valid_linkage(Z) and hier.is_monotonic(Z)
    assert np.array_equal(Z[:, 2], H.heights(ref["merges"], m, linkage)) and np.array_equal(Z[:, 3], ref["merges"]["size"])
    order = rc.leaf_order(Z)
    assert np.array_equal(order, hier.leaves_list(Z)) and sorted(order) == list(range(n))


@pytest.mark.parametrize("shape", SHAPES[2:], ids=[f"n{s[0]}" for s in SHAPES[2:]])
def test_single_linkage_heights_equal_scipys_as_a_multiset(shape):
    """Single-linkage merge heights are those of a minimum spanning tree's edges: independent of how ties are broken.  (Complete
    and average heights do depend on it, which is why SciPy is not the oracle for them.)"""
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    n, m = shape[0], shape[1]
    C, ref = reference(shape, H.SINGLE)
    D = 1.0 - C.astype(np.float64) / m
    np.fill_diagonal(D, 0.0)
    Zs = hier.linkage(squareform(D, checks=False), "single")
    assert np.array_equal(np.sort(Zs[:, 2]), np.sort(H.heights(ref["merges"], m, H.SINGLE)))


def test_python_surface_rejects_bad_specifiers_before_any_device_work():
    C = np.array([[2, 1], [1, 2]], np.uint32)
    with pytest.raises(ValueError, match="linkage"):
        rc.hclust(C, "ward", numsamples=2)
    with pytest.raises(ValueError, match="linkage"):
        rc.hclustpointestimate(C, "VI", "centroid", numsamples=2)
    for loss in ("ID", "omARI"):
        with pytest.raises(ValueError, match="loss"):
            rc.hclustpointestimate(C, loss, numsamples=2)
        with pytest.raises(ValueError, match="loss"):
            rc.expectedlosses([[1, 2]], C, 2, loss)
    with pytest.raises(ValueError, match="numsamples"):
        rc.hclust(C)


def test_header_signatures_and_julia_glue_agree():
    import test_oracle_cpu as T
    new = {"rc_hclust", "rc_hclust_samples", "rc_hclust_ctx", "rc_hclust_cut", "rc_psm_expected_loss", "rc_psm_expected_loss_ctx"}
    assert new <= set(rc.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    protos = T._header_prototypes(hdr)
    for name in new:
        assert name in protos and len(protos[name][1]) == len(rc.SIGNATURES[name][1]), name
    fields = dict(T._header_structs(hdr))["rc_hclust_merge_t"]
    assert [f[0] for f in fields] == list(_lib.HCLUST_MERGE.names) and _lib.HCLUST_MERGE.itemsize == 24 == H.MERGE.itemsize
    T.test_abi_library_exports_every_declared_symbol()
    T.test_julia_glue_ccalls_match_the_header()
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    used = {c[0] for c in T._julia_ccalls(jl)}
    assert {"rc_hclust", "rc_hclust_samples", "rc_hclust_cut"} <= used
    assert "function hclustpointestimate(b::HIPBackend, counts::Matrix{UInt32}, numsamples::Integer" in jl
    assert "function hclustpointestimate(b::HIPBackend, result" in jl
