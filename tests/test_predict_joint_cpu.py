"""Joint predict without a GPU: every visit of the NumPy reference (tests/predict_joint_ref.py) against the C oracle, the decision
gaps of every fixed input the GPU tests use and what those inputs claim to cover, the reference's draw frequencies against the
exact sequential probabilities, the planted hold-out, and the interface — header / SIGNATURES / Julia agreement, the argument
errors of rc.predict_joint that need no device, JointPrediction's methods."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import oracle_lib as O
import predict_ref as R
import predict_joint_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_visit(i, z, y, Dq_i, Lq_i, eD, eL, r, p, P):
    """orc_point_scores_stable for the visit of new point i, on the embedded problem of the allocated points alone: the n
    training points, the other allocated new points and, last, point i (under its own label, or under the smallest unused
    one when it is unallocated); the fixed-point matrices are zero except that last row."""
    n = len(z)
    others = [j for j in range(len(y)) if j != i and y[j] > 0]
    cols = list(range(n)) + [n + j for j in others]
    N = len(cols) + 1
    Dq, Lq = np.zeros((N, N), np.int64), np.zeros((N, N), np.int64)
    Dq[N - 1, :N - 1], Lq[N - 1, :N - 1] = Dq_i[cols], Lq_i[cols]
    rest = np.concatenate([z, y[others]]).astype(np.int64)
    own = int(y[i]) if y[i] > 0 else int(np.setdiff1d(np.arange(1, N + 1), rest)[0])
    clusts = np.concatenate([rest, [own]]).astype(np.int64)
    assert clusts.max() <= N                                         # a state the sampler can reach (see the test below)
    sizes = np.bincount(clusts, minlength=N + 1)[1:].astype(np.int64)
    cands, sc = np.zeros(N + 1, np.int64), np.zeros(N + 1)
    k = O.lib().orc_point_scores_stable(N, Dq.reshape(-1), Lq.reshape(-1), int(eD), int(eL), O.size_table(P, N), clusts, sizes,
                                        C.byref(O.params(P)), float(r), float(p), N - 1, cands, sc)
    return cands[:k], sc[:k]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_each_visit_equals_the_oracle_bit_for_bit(n):
    """States with clusters of new points alone, a visit whose removal kills such a cluster (its label is the one a new cluster
    takes again) and maxK reached by a cluster born in the call.  Labels of new clusters are lowest free ones, so with a
    allocated new points none exceeds n + a + 1: the embedded problem can name them."""
    q = 4
    rng = np.random.default_rng(300 + n)
    Dnew = rng.gamma(2.0, 1.0, size=(q, n)) + 0.05
    U = rng.gamma(2.0, 1.0, size=(q, q)) + 0.05
    Dnn = np.triu(U, 1) + np.triu(U, 1).T
    Dq, Lq, eD, eL = J.quantise_rows(Dnew, Dnn, *J.log_blocks(Dnew, Dnn))
    assert np.all(Dq[np.arange(q), n + np.arange(q)] == 0) and np.all(Lq[np.arange(q), n + np.arange(q)] == 0)
    kk = min(n, 5)
    names = rng.choice(n, size=kk, replace=False) + 1
    z = names[rng.integers(0, kk, size=n)].astype(np.int64)
    Ktr = len(np.unique(z))
    free = np.setdiff1d(np.arange(1, n + q + 1), z)
    L1, L2, T = int(free[0]), int(free[1]), int(z[0])
    # (labels of the new points, visited point, maxK, is the new cluster offered, does the removal kill a cluster)
    cases = [([L1, L1, T, 0], 3, 0, True, False),                   # a cluster of new points alone is a candidate
             ([L1, 0, 0, 0], 0, 0, True, True),                     # its only member leaves: the label is free again
             ([L1, L2, L2, T], 0, 0, True, True),                   # ... with another new cluster alive
             ([L1, L2, L2, T], 1, 0, True, False),
             ([L1, L1, T, 0], 3, Ktr + 1, False, False),            # maxK reached by the cluster born in the call
             ([L1, L1, T, 0], 3, Ktr + 2, True, False),
             ([L1, L2, L2, T], 0, Ktr + 1, False, True),            # the removal does not reopen the offer: L2 still counts
             ([L1, L2, T, T], 0, Ktr + 2, True, True)]              # ... but here it does
    for y, i, maxK, offered, dies in cases:
        y = np.array(y, np.int64)
        P = dict(J.PARAMS, maxK=maxK)
        r, p = float(rng.uniform(0.5, 3.0)), float(rng.uniform(0.1, 0.9))
        cands, newlab, sums, scores = J.visit_scores(i, z, y, Dq[i], Lq[i], eD[i], eL[i], r, p, P, O.size_table(P, n + q))
        oc, osc = _oracle_visit(i, z, y, Dq[i], Lq[i], eD[i], eL[i], r, p, P)
        alive = len(np.unique(np.concatenate([z, np.delete(y, i)[np.delete(y, i) > 0]])))
        assert len(cands) == len(oc) == alive + offered, (y, i, maxK)
        assert (cands[-1] == 0) == offered
        assert np.array_equal(cands[:alive], oc[:alive])
        if offered:
            assert oc[alive] == newlab                              # the oracle names the new cluster by the smallest empty label
        if dies:
            assert newlab == y[i] == L1 and L1 not in cands         # the dead label is the one taken again
        assert np.array_equal(scores, osc), np.abs(scores - osc).max()
        assert sums.shape == (alive, 2)


def _fixed_refs():
    refs = {f"edge{s}": J.edge_ref(*s) for s in J.EDGE_SHAPES}
    refs["split"] = J.split_ref()
    refs["holdout"] = J.holdout_ref()
    return refs


def test_gap_guard_of_every_fixed_gpu_input():
    """The device's scores deviate from the reference's by about 1e-12; exact label equality is a fair demand of it only if
    no decision of the reference is closer than that.  A seed that violates this is replaced here, not tolerated there."""
    for name, ref in _fixed_refs().items():
        print(name, ref["min_gap_noisy"])
        assert ref["min_gap_noisy"] > 1e-6, name
    assert J.frequency_ref()[3] > 1e-6
    # the input of "the library takes the logarithms itself": its gap also clears that test's slack cL·(n+q)·2^(1-eL)
    shape = (63, 3, 2, 1)
    c, ref = J.edge_case(*shape), J.edge_ref(*shape)
    P = c["P"]
    cL = abs((P["delta1"] - 1) - (P["delta2"] - 1))
    slack = cL * (shape[0] + shape[1]) * float(np.ldexp(2.0, -int(ref["eL"].min())))
    print("slack", slack)
    assert ref["min_gap_noisy"] > 1e-6 + slack


def test_fixed_inputs_cover_what_they_claim():
    for shape in J.EDGE_SHAPES[2:]:                                 # a sample of all singletons and one of a single cluster
        K = np.array([len(np.unique(z)) for z in J.edge_case(*shape)["samples"][:2]])
        assert K[0] == shape[0] and K[1] == 1
    c, ref = J.edge_case(65, 65, 5, 2), J.edge_ref(65, 65, 5, 2)
    assert c["P"]["repulsion"] is False                             # repulsion off
    assert c["sample_offset"] < 2 ** 32 <= c["sample_offset"] + 5 - 1      # a sample counter crossing 2^32
    assert c["P"]["maxK"] == 9 and ref["closed_midway"].any()       # maxK closes the new-cluster offer inside a pass ...
    Ktr = np.array([len(np.unique(z)) for z in c["samples"]])
    assert ((Ktr < 9) & (ref["K"] == 9)).any()                      # ... through clusters born in the call
    ref = J.edge_ref(64, 64, 3, 2)
    assert ref["reused"].any() and (ref["moves"][ref["reused"], 1:] > 0).all()     # a Gibbs pass with moves, a death, a reuse
    assert ref["new_only"].all()
    assert (ref["first"] != ref["labels"]).any()
    ref = J.edge_ref(257, 3, 1025, 2)
    assert ref["closed_midway"].any() and ref["reused"].any() and ref["new_only"].any() and not ref["new_only"].all()
    assert J.edge_case(40, 257, 2, 1)["Dnew"].shape[0] > 256        # more new points than a workgroup has threads
    assert J.split_ref()["new_only"].any() and (J.split_ref()["moves"][:, 1:] > 0).any()


def test_sequential_draw_frequencies():
    outcomes, prob, counts, _ = J.frequency_ref()
    m = J.frequency_case()["m"]
    assert abs(prob.sum() - 1) < 1e-12 and counts.sum() == m
    assert (4, 4) in outcomes and m * prob[outcomes.index((4, 4))] >= 100   # together in a new cluster
    assert np.count_nonzero(m * prob >= 100) >= 4
    print(dict(zip(outcomes, zip(np.round(m * prob, 1), counts))))
    assert R.within_4_sigma(counts, prob, m)


def test_planted_holdout_reference():
    c, ref = J.holdout_case(), J.holdout_ref()
    unseen, truth = c["unseen"], c["truth_new"]
    assert unseen.sum() == 12 and len(truth) == 30 and c["samples"].shape == (5, 120)
    for lab in ref["labels"]:
        group = np.unique(lab[unseen])
        assert len(group) == 1 and group[0] not in c["samples"][0] and not np.any(lab[~unseen] == group[0])
        assert np.array_equal(lab[~unseen], truth[~unseen])
    assert np.all(ref["K"] == 4)
    # independent predict can only make singletons of them
    ind = R.predict_ref(c["Dnew"], c["logDnew"], c["samples"], c["r"], c["p"], c["P"], c["seed"])
    assert np.all(ind["labels"][:, unseen] == 0)


# ---------------------------------------------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_julia_agree_on_rc_predict_joint():
    import test_oracle_cpu as T
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    ret, args = T._header_prototypes(hdr)["rc_predict_joint"]
    assert ret == "int32_t" and len(args) == 23
    assert args == ["int32_t", "int64_t", "int64_t", "double*", "double*", "double*", "double*", "int64_t", "int64_t*", "double*", "double*",
                    "rc_params*", "int64_t", "uint64_t", "uint64_t", "int64_t*", "int64_t*", "int64_t*", "int64_t*", "int64_t*",
                    "int32_t*", "int32_t*", "double*"]
    res, sig = rc.SIGNATURES["rc_predict_joint"]
    assert res is C.c_int32 and len(sig) == 23
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    for k, (ct, py) in enumerate(zip(args, sig)):
        if ct in scalars:
            assert py is scalars[ct], (k, ct, py)
        else:
            assert py in (C.c_void_p, C.POINTER(rc._lib.RcParams), C.POINTER(C.c_double)), (k, ct, py)
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    calls = [c for c in T._julia_ccalls(jl) if c[0] == "rc_predict_joint"]
    assert len(calls) == 1
    _, jret, jargs, npassed = calls[0]
    assert jret == "Int32" and len(jargs) == npassed == 23
    for jt, ct in zip(jargs, args):
        assert ct in T._JL2C[jt], (jt, ct)
    assert re.search(r"function predict_joint\(b::HIPBackend, result, Dnew::Matrix\{Float64\}, Dnn::Matrix\{Float64\}; sweeps\s*=\s*2, seed\s*=\s*0\)", jl)
    T.test_julia_glue_ccalls_match_the_header()


def test_the_source_is_part_of_the_build():
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    assert '#include "predictjoint.inc.hip"' in open(os.path.join(csrc, "redclust_hip.hip")).read()
    assert os.path.join(csrc, "predictjoint.inc.hip") in _lib._sources()   # build() watches it
    src = open(os.path.join(csrc, "predictjoint.inc.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # plain C++ and vector memory operations only
    assert "rc_predict_joint" in rc.SIGNATURES and callable(rc.predict_joint) and rc.JointPrediction is not None


def test_argument_errors_raise_before_any_device_work():
    S = np.array([[1, 1, 2], [3, 3, 3]], np.int64)
    D = np.ones((2, 3))
    Dn = np.array([[0.0, 1.0], [1.0, 0.0]])
    P = dict(J.PARAMS)
    ok = dict(r=[1.0, 1.0], p=[0.5, 0.5], params=P)
    with pytest.raises(ValueError, match="r, p and params"):
        rc.predict_joint(S, D, Dn)
    with pytest.raises(ValueError, match="either Dnew with Dnn or new_points"):
        rc.predict_joint(S, **ok)
    with pytest.raises(ValueError, match="either Dnew with Dnn or new_points"):
        rc.predict_joint(S, D, Dn, new_points=np.ones((1, 2)), points=np.ones((3, 2)), **ok)
    with pytest.raises(ValueError, match="needs Dnn"):
        rc.predict_joint(S, D, **ok)
    with pytest.raises(ValueError, match="q×n"):
        rc.predict_joint(S, np.ones((2, 4)), Dn, **ok)
    with pytest.raises(ValueError, match="Dnew must be finite and positive"):
        rc.predict_joint(S, np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 1.0]]), Dn, **ok)
    with pytest.raises(ValueError, match="q×q"):
        rc.predict_joint(S, D, np.ones((3, 3)), **ok)
    with pytest.raises(ValueError, match="off the diagonal"):
        rc.predict_joint(S, D, np.zeros((2, 2)), **ok)
    with pytest.raises(ValueError, match="off the diagonal"):
        rc.predict_joint(S, D, np.array([[0.0, np.inf], [np.inf, 0.0]]), **ok)
    with pytest.raises(ValueError, match="symmetric"):
        rc.predict_joint(S, D, np.array([[0.0, 1.0], [2.0, 0.0]]), **ok)
    with pytest.raises(ValueError, match="sweeps"):
        rc.predict_joint(S, D, Dn, sweeps=-1, **ok)
    with pytest.raises(ValueError, match="sweeps"):
        rc.predict_joint(S, D, Dn, sweeps=1.5, **ok)
    with pytest.raises(ValueError, match="1..n"):
        rc.predict_joint(np.array([[1, 4, 1]]), D, Dn, r=[1.0], p=[0.5], params=P)
    with pytest.raises(ValueError, match="integer labels"):
        rc.predict_joint(np.ones((2, 3)), D, Dn, **ok)
    with pytest.raises(ValueError, match="one value per sample"):
        rc.predict_joint(S, D, Dn, r=[1.0], p=[0.5, 0.5], params=P)
    with pytest.raises(ValueError, match="r must be positive"):
        rc.predict_joint(S, D, Dn, r=[1.0, 0.0], p=[0.5, 0.5], params=P)
    with pytest.raises(ValueError, match=r"p must lie in \(0, 1\)"):
        rc.predict_joint(S, D, Dn, r=[1.0, 1.0], p=[0.5, 1.0], params=P)
    with pytest.raises(ValueError, match="alpha"):
        rc.predict_joint(S, D, Dn, r=[1.0, 1.0], p=[0.5, 0.5], params=dict(P, alpha=0.0))
    with pytest.raises(ValueError, match="Dnn goes with Dnew"):
        rc.predict_joint(S, None, Dn, new_points=np.ones((1, 2)), points=np.ones((3, 2)), **ok)
    with pytest.raises(ValueError, match="needs the training points"):
        rc.predict_joint(S, new_points=np.ones((1, 2)), **ok)
    with pytest.raises(ValueError, match="training observations"):
        rc.predict_joint(S, new_points=np.ones((1, 2)), points=np.ones((4, 2)), **ok)
    with pytest.raises(ValueError, match="dimension"):
        rc.predict_joint(S, new_points=np.ones((1, 3)), points=np.ones((3, 2)), **ok)
    with pytest.raises(ValueError, match="coincides with a training point"):
        rc.predict_joint(S, new_points=np.zeros((1, 2)), points=np.zeros((3, 2)), **ok)
    with pytest.raises(ValueError, match="two new points coincide"):
        rc.predict_joint(S, new_points=np.ones((2, 2)), points=np.zeros((3, 2)), **ok)
    with pytest.raises(ValueError, match="no samples"):
        rc.predict_joint([], D, Dn, **ok)


class _Relabelling:
    """what JointPrediction.allocation reads of a pointestimate.Relabelling"""
    def __init__(self, maps, pivot_labels):
        self.maps, self.pivot_labels = np.asarray(maps, np.int64), np.asarray(pivot_labels, np.int64)


def test_joint_prediction_methods_on_hand_written_inputs():
    S = np.array([[2, 2, 5, 5, 1], [3, 3, 3, 3, 3], [1, 2, 3, 4, 5]], np.int64)
    labels = np.array([[3, 5, 3, 2], [1, 1, 3, 2], [6, 4, 6, 7]], np.int64)        # 3 | 1, 2 | 6, 7: names the samples do not use
    jp = rc.JointPrediction(labels=labels, first_labels=labels.copy(), K=np.array([4, 3, 7]), moves=np.zeros((3, 1), np.int64))
    E = jp.extended_samples(S)
    assert E.shape == (3, 9) and E.dtype == np.int64
    assert np.array_equal(E[:, :5], S) and np.array_equal(E[:, 5:], labels)         # a plain concatenation
    assert [len(np.unique(e)) for e in E] == [4, 3, 7]
    assert np.allclose(jp.new_cluster_frequency(S), [1.0, 1 / 3, 2 / 3, 2 / 3])
    with pytest.raises(ValueError, match="samples of the prediction"):
        jp.extended_samples(S[:2])
    with pytest.raises(ValueError, match="samples of the prediction"):
        jp.new_cluster_frequency(S[:2])
    # the pivot has clusters 10 and 20; maps[s][t]: the pivot cluster the t-th smallest name of sample s became (0: none)
    rel = _Relabelling([[10, 20, 0, 0, 0], [20, 0, 0, 0, 0], [10, 10, 20, 20, 0]], [10, 20])
    alloc = jp.allocation(rel, S)
    assert alloc.shape == (4, 3) and np.allclose(alloc.sum(axis=1), 1)
    # point 0: 3 (unknown) | 1 (unknown) | 6 (unknown) -> column 0 thrice; point 1: 5 -> rank 2 -> none | 1 unknown | 4 -> 20
    assert np.allclose(alloc[0], [1, 0, 0])
    assert np.allclose(alloc[1], [2 / 3, 0, 1 / 3])
    # point 2: 3 unknown | 3 -> 20 | 6 unknown; point 3: 2 -> 20 | 2 unknown | 7 unknown
    assert np.allclose(alloc[2], [2 / 3, 0, 1 / 3])
    assert np.allclose(alloc[3], [2 / 3, 0, 1 / 3])
    # Prediction.allocation keeps raising on a name that is not the sample's
    pred = rc.Prediction(labels=labels, map_labels=labels.copy())
    with pytest.raises(ValueError, match="not a label of sample 1"):
        pred.allocation(rel, S)
    zeros = rc.Prediction(labels=np.array([[0, 5, 0, 2], [0, 0, 3, 0], [0, 4, 0, 0]], np.int64), map_labels=labels.copy())
    assert np.allclose(zeros.allocation(rel, S), [[1, 0, 0], [2 / 3, 0, 1 / 3], [2 / 3, 0, 1 / 3], [2 / 3, 0, 1 / 3]])
