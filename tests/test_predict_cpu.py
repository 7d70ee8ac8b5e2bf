"""Predict without a GPU: the NumPy reference (tests/predict_ref.py) against the C oracle, the decision gaps of every fixed
input the GPU tests use, the reference's draw frequencies, and the interface — header / SIGNATURES / Julia agreement, the
argument errors of rc.predict that need no device, Prediction.extended_samples."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import oracle_lib as O
import predict_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_scores(z, Dq_i, Lq_i, eD, eL, r, p, P):
    """orc_point_scores_stable for the new point embedded as point n+1, under the smallest unused label, of an (n+1)-point
    problem whose fixed-point matrices are zero except that row."""
    n = len(z)
    N = n + 1
    Dq, Lq = np.zeros((N, N), np.int64), np.zeros((N, N), np.int64)
    Dq[n, :n], Lq[n, :n] = Dq_i, Lq_i
    own = int(np.setdiff1d(np.arange(1, N + 1), z)[0])
    clusts = np.concatenate([z, [own]]).astype(np.int64)
    sizes = np.bincount(clusts, minlength=N + 1)[1:].astype(np.int64)
    cands, sc = np.zeros(N + 1, np.int64), np.zeros(N + 1)
    k = O.lib().orc_point_scores_stable(N, Dq.reshape(-1), Lq.reshape(-1), int(eD), int(eL), O.size_table(P, N), clusts, sizes,
                                        C.byref(O.params(P)), float(r), float(p), n, cands, sc)
    return cands[:k], sc[:k], own


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_reference_equals_the_oracle_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    Dnew = rng.gamma(2.0, 1.0, size=(1, n)) + 0.05
    Dq, Lq, eD, eL = R.quantise_rows(Dnew, np.log(Dnew), n)
    kk = min(n, 5)
    names = rng.choice(n, size=kk, replace=False) + 1
    random = names[rng.integers(0, kk, size=n)].astype(np.int64)
    K_random = len(np.unique(random))
    cases = [(rng.permutation(n).astype(np.int64) + 1, 0),          # all singletons: K_s = n
             (np.full(n, n, np.int64), 0),                          # a single cluster
             (random, 0),
             (random, K_random),                                    # maxK = K_s: no new cluster
             (random, K_random + 1)]
    for z, maxK in cases:
        P = dict(R.PARAMS, maxK=maxK)
        r, p = float(rng.uniform(0.5, 3.0)), float(rng.uniform(0.1, 0.9))
        cands, _, scores, _ = R.score_point(Dq[0], Lq[0], eD[0], eL[0], z, r, p, P, O.size_table(P, n))
        oc, osc, own = _oracle_scores(z, Dq[0], Lq[0], eD[0], eL[0], r, p, P)
        K = len(np.unique(z))
        offered = maxK == 0 or K < maxK
        assert len(cands) == len(oc) == K + offered
        assert np.array_equal(cands[:K], oc[:K])
        if offered:
            assert cands[K] == 0 and oc[K] == own                   # the oracle names the new cluster by the smallest empty label
        assert np.array_equal(scores, osc), np.abs(scores - osc).max()


def test_gap_guard_of_every_fixed_gpu_input():
    """The device may deviate from the reference by 2^-49 of a score's terms (about 1e-12 here); exact label equality is a
    fair demand of it only if no decision of the reference is closer than that.  A seed that violates this is replaced
    here, not tolerated there."""
    refs = {f"edge{s}": R.edge_ref(*s) for s in R.EDGE_SHAPES}
    refs["independence"] = R.independence_ref()
    refs["holdout"] = R.holdout_ref()
    for name, ref in refs.items():
        print(name, ref["min_gap_noisy"], ref["min_gap_map"])
        assert ref["min_gap_noisy"] > 1e-6 and ref["min_gap_map"] > 1e-6, name
    assert R.frequency_ref()[3] > 1e-6


def test_edge_inputs_cover_what_they_claim():
    for shape in R.EDGE_SHAPES[1:]:
        c = R.edge_case(*shape)
        K = np.array([len(np.unique(z)) for z in c["samples"]])
        assert K[0] == shape[0] and K[1] == 1
    c, ref = R.edge_case(257, 3, 1025), R.edge_ref(257, 3, 1025)
    K = ref["K"]
    assert c["P"]["maxK"] == 4 and (K < 4).any() and (K == 4).any() and (K > 4).any()
    new = ref["scores"][:, :, ref["Kmax"]]
    assert np.all(np.isneginf(new[K >= 4])) and np.all(np.isfinite(new[K < 4]))
    assert (ref["labels"] != ref["map"]).any()
    for shape in ((64, 2, 65), (65, 2, 63)):                         # the two whose draws open clusters, and not always
        lab = R.edge_ref(*shape)["labels"]
        assert (lab == 0).any() and (lab != 0).any() and (R.edge_ref(*shape)["map"] == 0).any()
    assert R.edge_case(65, 2, 63)["P"]["repulsion"] is False


def test_frequency_input_and_the_references_draws():
    cands, prob, counts, _ = R.frequency_ref()
    assert list(cands) == [1, 2, 3, 0]
    assert np.allclose(prob, [0.0159, 0.9694, 0.0147, 3.9e-5], atol=1e-4), prob      # the input is the one the numbers belong to
    assert list(counts) == [290, 19402, 306, 2]
    assert R.within_4_sigma(counts, prob, 20000)
    z = [(c - 20000 * q) / math.sqrt(20000 * q * (1 - q)) for c, q in zip(counts[:3], prob[:3])]
    assert np.allclose(z, [-1.60, 0.60, 0.72], atol=0.01), z


def test_holdout_reference():
    c, ref = R.holdout_case(), R.holdout_ref()
    assert np.array_equal(ref["labels"][:, :30], np.stack([c["truth_new"]] * 2))
    assert np.array_equal(ref["map"][:, :30], np.stack([c["truth_new"]] * 2))
    assert np.all(ref["labels"][:, 30] == 0) and np.all(ref["map"][:, 30] == 0)
    assert ref["min_gap_noisy"] > 100


# ---------------------------------------------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_julia_agree_on_rc_predict():
    import test_oracle_cpu as T
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    ret, args = T._header_prototypes(hdr)["rc_predict"]
    assert ret == "int32_t" and len(args) == 21
    assert args == ["int32_t", "int64_t", "int64_t", "double*", "double*", "int64_t", "int64_t*", "double*", "double*", "rc_params*",
                    "uint64_t", "uint64_t", "uint64_t", "int64_t*", "int64_t*", "int64_t", "double*", "int64_t*", "int32_t*",
                    "int32_t*", "double*"]
    res, sig = rc.SIGNATURES["rc_predict"]
    assert res is C.c_int32 and len(sig) == 21
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    for k, (ct, py) in enumerate(zip(args, sig)):
        if ct in scalars:
            assert py is scalars[ct], (k, ct, py)
        else:
            assert py in (C.c_void_p, C.POINTER(rc._lib.RcParams), C.POINTER(C.c_double)), (k, ct, py)
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    calls = [c for c in T._julia_ccalls(jl) if c[0] == "rc_predict"]
    assert len(calls) == 1
    _, jret, jargs, npassed = calls[0]
    assert jret == "Int32" and len(jargs) == npassed == 21
    for jt, ct in zip(jargs, args):
        assert ct in T._JL2C[jt], (jt, ct)
    assert re.search(r"function predict\(b::HIPBackend, result, Dnew::Matrix\{Float64\}; seed\s*=\s*0\)", jl)
    T.test_julia_glue_ccalls_match_the_header()


def test_the_source_is_part_of_the_build():
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    assert '#include "predict.inc.hip"' in open(os.path.join(csrc, "redclust_hip.hip")).read()
    assert os.path.join(csrc, "predict.inc.hip") in _lib._sources()  # build() watches it
    src = open(os.path.join(csrc, "predict.inc.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # plain C++ and vector memory operations only
    assert '#include "slab.inc.hip"' in open(os.path.join(csrc, "redclust_hip.hip")).read()   # ... k_predict_sums' file too
    assert "asm" not in re.sub(r"//.*", "", open(os.path.join(csrc, "slab.inc.hip")).read())


def test_argument_errors_raise_before_any_device_work():
    S = np.array([[1, 1, 2], [3, 3, 3]], np.int64)
    D = np.ones((2, 3))
    P = dict(R.PARAMS)
    ok = dict(r=[1.0, 1.0], p=[0.5, 0.5], params=P)
    with pytest.raises(ValueError, match="r, p and params"):
        rc.predict(S, D)
    with pytest.raises(ValueError, match="either Dnew or new_points"):
        rc.predict(S, **ok)
    with pytest.raises(ValueError, match="either Dnew or new_points"):
        rc.predict(S, D, new_points=np.ones((1, 2)), points=np.ones((3, 2)), **ok)
    with pytest.raises(ValueError, match="q×n"):
        rc.predict(S, np.ones((2, 4)), **ok)
    with pytest.raises(ValueError, match="finite and positive"):
        rc.predict(S, np.array([[1.0, 0.0, 1.0]]), **ok)
    with pytest.raises(ValueError, match="finite and positive"):
        rc.predict(S, np.array([[1.0, np.inf, 1.0]]), **ok)
    with pytest.raises(ValueError, match="1..n"):
        rc.predict(np.array([[1, 4, 1]]), np.ones((1, 3)), r=[1.0], p=[0.5], params=P)
    with pytest.raises(ValueError, match="integer labels"):
        rc.predict(np.ones((2, 3)), D, **ok)
    with pytest.raises(ValueError, match="one value per sample"):
        rc.predict(S, D, r=[1.0], p=[0.5, 0.5], params=P)
    with pytest.raises(ValueError, match="r must be positive"):
        rc.predict(S, D, r=[1.0, 0.0], p=[0.5, 0.5], params=P)
    with pytest.raises(ValueError, match=r"p must lie in \(0, 1\)"):
        rc.predict(S, D, r=[1.0, 1.0], p=[0.5, 1.0], params=P)
    with pytest.raises(ValueError, match="alpha"):
        rc.predict(S, D, r=[1.0, 1.0], p=[0.5, 0.5], params=dict(P, alpha=0.0))
    with pytest.raises(ValueError, match="maxK"):
        rc.predict(S, D, r=[1.0, 1.0], p=[0.5, 0.5], params=dict(P, maxK=-1))
    with pytest.raises(ValueError, match="needs the training points"):
        rc.predict(S, new_points=np.ones((1, 2)), **ok)
    with pytest.raises(ValueError, match="training observations"):
        rc.predict(S, new_points=np.ones((1, 2)), points=np.ones((4, 2)), **ok)
    with pytest.raises(ValueError, match="dimension"):
        rc.predict(S, new_points=np.ones((1, 3)), points=np.ones((3, 2)), **ok)
    with pytest.raises(ValueError, match="coincides"):
        rc.predict(S, new_points=np.zeros((1, 2)), points=np.zeros((3, 2)), **ok)
    with pytest.raises(ValueError, match="no samples"):
        rc.predict([], D, **ok)


def test_extended_samples():
    S = np.array([[2, 2, 5, 5, 1], [3, 3, 3, 3, 3], [1, 2, 3, 4, 5]], np.int64)
    labels = np.array([[0, 5, 0, 2], [0, 0, 3, 0], [0, 4, 0, 0]], np.int64)
    pred = rc.Prediction(labels=labels, map_labels=labels.copy())
    E = pred.extended_samples(S)
    assert E.shape == (3, 9) and E.dtype == np.int64
    assert np.array_equal(E[:, :5], S)                              # the training columns are unchanged
    assert E.min() >= 1 and E.max() <= 9                            # the range posterior_counts and the searches accept
    assert np.array_equal(E[0, 5:], [3, 5, 4, 2])                   # the a-th own cluster gets the a-th smallest unused label
    assert np.array_equal(E[1, 5:], [1, 2, 3, 4])
    assert np.array_equal(E[2, 5:], [6, 4, 7, 8])
    for s in range(3):
        own = E[s, 5:][labels[s] == 0]
        assert len(set(own)) == len(own) and not set(own) & set(S[s])      # distinct, and no existing cluster's name
        assert np.array_equal(E[s, 5:][labels[s] != 0], labels[s][labels[s] != 0])
    assert np.allclose(pred.new_cluster_frequency(), [1.0, 1 / 3, 2 / 3, 2 / 3])
    with pytest.raises(ValueError, match="samples of the prediction"):
        pred.extended_samples(S[:2])
