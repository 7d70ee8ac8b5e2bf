"""Relabelling without a GPU: the NumPy restatement (tests/relabel_ref.py) against SciPy's linear_sum_assignment in optimum
value, its structural properties, Prediction.allocation on hand-made maps, the Relabelling summaries, and the interface —
header / SIGNATURES / Julia agreement for rc_relabel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import relabel_ref as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the reference's assignment
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("high", [2, 3, 50], ids=["01", "012", "0to49"])
def test_matching_is_optimal_injective_and_of_full_size(high):
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(high)
    seen = set()
    for _ in range(120):
        Kp, Ks = (int(x) for x in rng.integers(1, 14, 2))
        N = rng.integers(0, high, (Kp, Ks)).astype(np.int64)
        for M in (N, np.ascontiguousarray(N.T)):                      # both orientations
            to = RL.match(M)
            kp, ks = M.shape
            seen.add(np.sign(kp - ks))
            matched = to[to >= 0]
            assert len(to) == ks and len(matched) == min(kp, ks) and len(set(matched)) == len(matched)
            assert matched.max() < kp
            value = sum(int(M[to[l], l]) for l in range(ks) if to[l] >= 0)
            r, c = linear_sum_assignment(M, maximize=True)
            assert value == int(M[r, c].sum()), (M, to)
    assert seen == {-1, 0, 1}


def test_ties_go_to_the_smallest_column():
    # one row, every column equal: the first column; the first of two maxima
    assert np.array_equal(RL.assign_rows(np.ones((1, 5), np.int64)), [0])
    assert np.array_equal(RL.assign_rows(np.array([[3, 7, 7, 1]])), [1])
    # Two equal rows.  Row 1 takes column 1.  Row 2 sees equal reduced costs everywhere and steps to column 1 (the smallest id),
    # which is taken; from row 1 the unused columns cost no less than they already do from the root (not strictly less: their
    # predecessor stays the root), the smallest of them, column 2, is free, and the path root -> column 2 gives it to row 2.
    assert np.array_equal(RL.assign_rows(np.ones((2, 3), np.int64)), [0, 1])
    # a table of ones: every step is a tie, and the matching is still a permutation
    assert sorted(RL.match(np.ones((6, 6), np.int64))) == [0, 1, 2, 3, 4, 5]


def test_a_renamed_pivot_is_recovered():
    rng = np.random.default_rng(5)
    n = 97
    c = rng.integers(1, 9, n) * 7                                     # names spread out, all <= n
    names = np.unique(c)
    perm = rng.permutation(n)[:len(names)] + 1                        # other names for the same clusters
    z = perm[np.searchsorted(names, c)]
    out = RL.relabel_ref(np.stack([z, c]), c)
    assert np.array_equal(out["overlap"], [n, n])
    assert np.array_equal(out["labels"][0], c) and np.array_equal(out["labels"][1], c)
    assert np.array_equal(out["pivot_labels"], names)
    assert np.array_equal(out["counts"].sum(1), [2] * n) and np.all(out["counts"][:, 0] == 0)
    assert np.array_equal(out["counts"][np.arange(n), np.searchsorted(names, c) + 1], [2] * n)


def test_more_sample_clusters_than_pivot_clusters_leaves_the_surplus_at_zero():
    rng = np.random.default_rng(6)
    n = 120
    c = rng.integers(1, 4, n)                                         # K_p = 3
    S = np.stack([rng.integers(1, 8, n), rng.integers(10, 15, n), c])  # K_s = 7, 5, 3
    out = RL.relabel_ref(S, c)
    for s, Ks in enumerate([7, 5, 3]):
        row = out["maps"][s]
        assert np.sum(row[:Ks] == 0) == Ks - 3 and np.all(row[Ks:] == -1) and np.all(row[:Ks] >= 0)
        assert sorted(row[:Ks][row[:Ks] > 0]) == [1, 2, 3]
        assert np.sum(out["labels"][s] == 0) == sum(np.sum(S[s] == l) for l, to in zip(np.unique(S[s]), row) if to == 0)
    assert out["maps"].shape == (3, 7)
    assert np.array_equal(out["counts"].sum(1), [3] * n)
    # and the reverse: fewer sample clusters than pivot clusters, everything matched
    out = RL.relabel_ref(c[None, :], S[0])
    assert np.all(out["maps"][0] > 0) and len(set(out["maps"][0])) == 3 and np.all(out["labels"] > 0)


# ---------------------------------------------------------------------------------------------------------------
# the host layer
# ---------------------------------------------------------------------------------------------------------------
def test_relabelling_summaries():
    counts = np.array([[0, 3, 1], [2, 1, 1], [0, 2, 2], [4, 0, 0]], np.uint32)
    r = rc.Relabelling(labels=np.zeros((4, 4), np.int64), maps=np.zeros((4, 2), np.int64), overlap=np.zeros(4, np.int64), counts=counts,
                       pivot_labels=np.array([2, 9]))
    assert np.array_equal(r.probabilities(), counts / 4.0) and r.probabilities().shape == (4, 3)
    assert np.array_equal(r.allocation(), [2, 0, 2, 0])              # ties to the smaller column; 0 is possible
    assert np.array_equal(r.uncertainty(), [0.25, 0.5, 0.5, 0.0])


def test_prediction_allocation_on_hand_made_maps():
    S = np.array([[2, 2, 5, 5, 1], [3, 3, 3, 3, 3], [1, 2, 3, 4, 5]], np.int64)      # sorted names: (1,2,5), (3), (1,2,3,4,5)
    maps = np.array([[0, 7, 4, -1, -1], [4, -1, -1, -1, -1], [4, 0, 7, 0, 0]], np.int64)
    rel = rc.Relabelling(labels=np.zeros_like(S), maps=maps, overlap=np.zeros(3, np.int64), counts=np.zeros((5, 3), np.uint32),
                         pivot_labels=np.array([4, 7]))
    labels = np.array([[2, 5, 0, 1],          # -> 7, 4, own, unmatched
                       [3, 3, 0, 3],          # -> 4, 4, own, 4
                       [3, 1, 5, 2]], np.int64)   # -> 7, 4, unmatched, unmatched
    pred = rc.Prediction(labels=labels, map_labels=labels.copy())
    A = pred.allocation(rel, S)
    assert A.shape == (4, 3)
    assert np.array_equal(A * 3, [[0, 1, 2], [0, 3, 0], [3, 0, 0], [2, 1, 0]])
    assert np.allclose(A.sum(1), 1.0)
    with pytest.raises(ValueError, match="3 samples"):
        pred.allocation(rel, S[:2])
    short = rc.Relabelling(labels=S[:2], maps=maps[:2], overlap=np.zeros(2, np.int64), counts=np.zeros((5, 3), np.uint32),
                           pivot_labels=np.array([4, 7]))
    with pytest.raises(ValueError, match="3 samples"):
        pred.allocation(short, S)
    bad = rc.Prediction(labels=np.array([[4, 5, 0, 1], [3, 3, 0, 3], [3, 1, 5, 2]], np.int64), map_labels=labels)
    with pytest.raises(ValueError, match="sample 1"):
        bad.allocation(rel, S)


def test_relabel_argument_errors_raise_before_any_device_work():
    S = np.array([[1, 1, 2], [3, 3, 3]], np.int64)
    with pytest.raises(ValueError, match="as many labels"):
        rc.relabel(S, [1, 2])
    with pytest.raises(ValueError, match="no samples"):
        rc.relabel([], [1, 2, 3])
    with pytest.raises(TypeError, match="integers"):
        rc.relabel(S, [1.0, 2.0, 1.0])


# ---------------------------------------------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_julia_agree_on_rc_relabel():
    import test_oracle_cpu as T
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    ret, args = T._header_prototypes(hdr)["rc_relabel"]
    assert ret == "int32_t" and len(args) == 12
    assert args == ["int32_t", "int64_t*", "int64_t", "int64_t", "int64_t*", "int64_t", "int64_t*", "int64_t*", "int64_t", "int64_t*",
                    "void*", "double*"]
    res, sig = rc.SIGNATURES["rc_relabel"]
    assert res is C.c_int32 and len(sig) == 12
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for k, (ct, py) in enumerate(zip(args, sig)):
        if ct in scalars:
            assert py is scalars[ct], (k, ct, py)
        else:
            assert py in (C.c_void_p, C.POINTER(C.c_double)), (k, ct, py)
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    calls = [c for c in T._julia_ccalls(jl) if c[0] == "rc_relabel"]
    assert len(calls) == 1
    _, jret, jargs, npassed = calls[0]
    assert jret == "Int32" and len(jargs) == npassed == 12
    for jt, ct in zip(jargs, args):
        assert ct in T._JL2C[jt], (jt, ct)
    assert re.search(r"function relabel\(b::HIPBackend, result, pivot::AbstractVector\{<:Integer\}\)", jl)
    assert re.search(r"^export relabel$", jl, flags=re.M)
    T.test_julia_glue_ccalls_match_the_header()


def test_the_source_is_part_of_the_build():
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    assert '#include "relabel.inc.hip"' in open(os.path.join(csrc, "redclust_hip.hip")).read()
    assert os.path.join(csrc, "relabel.inc.hip") in _lib._sources()  # build() watches it
    src = re.sub(r"//.*", "", open(os.path.join(csrc, "relabel.inc.hip")).read())
    assert "asm" not in src                                          # plain C++ only
    assert not re.search(r"\b(float|double)\b", src.split('extern "C"')[0])       # no floating point in the kernel
    assert hasattr(rc, "relabel") and hasattr(rc.Prediction, "allocation")
