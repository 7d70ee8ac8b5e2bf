"""Scoring labellings, the parts that need no GPU: the reference of the block sums (tests/score_ref.py) against the definition,
rc_loglik_from_blocks — host only — against the C oracle's loglik_stable on the oracle's own quantised matrices, the argument
errors of both entries, the host-only helpers built on the block sums (reweight, mapestimate) and the three declarations of the
interface (header, SIGNATURES, Julia)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import oracle_lib as O
import score_ref as R
from test_gpu_parity import LL_RTOL          # what the parity tests allow between rc_loglik and the oracle's stable mode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def paper():
    d = np.load(os.path.join(ROOT, "tests", "golden", "paper_datasets.npz"))
    D, truth = d["D1"], d["labels1"].astype(np.int64)
    P = rc.likelihood_hyperparams(D, truth)
    return D, truth, P, O.Oracle(D, P)


def labellings_of(n, truth):
    rng = np.random.default_rng(5)
    sparse = np.where(np.arange(n) % 3 == 0, 3, np.where(np.arange(n) % 3 == 1, 7, n))
    return dict(truth=truth, one=np.ones(n, np.int64), singletons=np.arange(1, n + 1), sparse=sparse,
                random=rng.integers(1, 11, n), reversed_names=n + 1 - truth)


def test_reference_matches_the_definition_at_n7():
    rng = np.random.default_rng(1)
    Dq = rng.integers(1, 1 << 40, (7, 7))                      # not symmetric, a nonzero diagonal
    Lq = rng.integers(-(1 << 40), 1 << 40, (7, 7))
    np.fill_diagonal(Lq, 0)
    for z in ([1, 1, 1, 1, 1, 1, 1], [1, 2, 3, 4, 5, 6, 7], [7, 3, 3, 7, 5, 5, 3], [2, 2, 6, 6, 6, 2, 6]):
        ref = R.block_sums_bruteforce(Dq, Lq, z)
        assert R.block_sums(Dq, Lq, z) == ref
        h = R.halves(Dq, Lq, z)
        assert R.values(h) == ref
        assert np.all((h[:, 1] >= 0) & (h[:, 3] >= 0))         # the low halves are sums of non-negative 24-bit pieces
    # rows in the smaller label, columns in the larger: an asymmetric matrix tells the two apart
    z = [5, 2, 5, 2, 2, 5, 5]
    rows, cols = [i for i in range(7) if z[i] == 2], [j for j in range(7) if z[j] == 5]
    assert R.block_sums(Dq, Lq, z)[1][0] == sum(int(Dq[i][j]) for i in rows for j in cols)
    assert R.block_sums(Dq, Lq, z)[1][0] != sum(int(Dq[j][i]) for i in rows for j in cols)


@pytest.mark.parametrize("repulsion", [True, False])
def test_loglik_from_blocks_agrees_with_the_oracle(paper, repulsion):
    D, truth, P, orc = paper
    P = dict(P, repulsion=repulsion)
    orc.set_params(P)
    try:
        for name, z in labellings_of(len(truth), truth).items():
            orc.set_state(z)
            ref = orc.loglik_stable()
            _, _, sizes = R.clusters(z)
            ll = rc.loglik_from_blocks(R.halves(orc.Dq, orc.Lq, z), sizes, orc.n, orc.eD, orc.eL, P)
            print(name, ll, ref, abs(ll - ref) / max(1.0, abs(ll)))
            assert abs(ll - ref) <= LL_RTOL * max(1.0, abs(ll)), name
    finally:
        orc.set_params(paper[2])


def test_loglik_from_blocks_depends_on_the_value_not_on_the_halves(paper):
    """hi·2^24 + lo is what counts: moving 2^24 from a low half into its high half changes nothing"""
    _, truth, P, orc = paper
    _, _, sizes = R.clusters(truth)
    h = R.halves(orc.Dq, orc.Lq, truth)
    g = h.copy()
    g[:, 0] += 1; g[:, 1] -= 1 << 24
    g[:, 2] -= 3; g[:, 3] += 3 << 24
    a, b = (rc.loglik_from_blocks(x, sizes, orc.n, orc.eD, orc.eL, P) for x in (h, g))
    assert a == b


def test_python_logprior_agrees_with_the_oracle(paper):
    from redclust_amd.score import logprior
    _, truth, P, orc = paper
    P = dict(P, eta=2.5, sigma=1.5, u=2.0, v=3.0)
    orc.set_params(P)
    try:
        for z in labellings_of(len(truth), truth).values():
            orc.set_state(z)
            _, _, sizes = R.clusters(z)
            lp, ref = logprior(sizes, orc.n, 1.3, 0.4, P), orc.logprior(1.3, 0.4)
            assert abs(lp - ref) <= 1e-12 * max(1.0, abs(ref))
    finally:
        orc.set_params(paper[2])


def test_argument_errors_of_the_host_entry(paper):
    _, truth, P, orc = paper
    L = rc.lib()
    prm = _lib._params_struct(P)
    sizes = np.array([2, 1], np.int64)
    blocks = np.zeros((3, 4), np.int64)
    out = C.c_double()

    def call(n=3, K=2, sz=sizes, b=blocks, p=prm, o=out):
        return L.rc_loglik_from_blocks(n, K, None if sz is None else sz.ctypes.data, None if b is None else b.ctypes.data, 40, 40,
                                       None if p is None else C.byref(p), None if o is None else C.byref(o))
    assert call() == 0
    for kw, text in ((dict(sz=None), "NULL"), (dict(b=None), "NULL"), (dict(p=None), "NULL"), (dict(o=None), "NULL"),
                     (dict(n=0), "n >= 1"), (dict(K=0), "K <= n"), (dict(K=4), "K <= n"), (dict(n=4), "sum to 3"),
                     (dict(sz=np.array([3, 0], np.int64)), "size 0 of cluster 2"),
                     (dict(p=_lib._params_struct(dict(P, beta=0.0))), "must be positive")):
        assert call(**kw) == -1, kw
        assert text in L.rc_last_error(None).decode(), (kw, L.rc_last_error(None).decode())
    with pytest.raises(ValueError, match=r"K\(K\+1\)/2"):
        rc.loglik_from_blocks(np.zeros((2, 4), np.int64), sizes, 3, 40, 40, P)


def test_argument_errors_of_the_device_entry_come_before_any_device_work():
    """without a context nothing else can be reached on a machine without a GPU; tests/test_gpu_score.py has the rest"""
    L = rc.lib()
    lab = np.ones((1, 3), np.int64)
    ll = np.zeros(1)
    assert L.rc_score_labellings(None, 1, lab.ctypes.data, None, None, None, ll.ctypes.data, None, None, None, 0, None, None, None) == -1
    assert "NULL ctx" in L.rc_last_error(None).decode()
    ctx = rc.Context.__new__(rc.Context)                        # the wrapper's own checks need no library call either
    ctx.n, ctx.h, ctx.L = 3, None, L
    with pytest.raises(ValueError, match="n columns"):
        ctx.score(np.ones((2, 4), np.int64))
    with pytest.raises(ValueError, match="both r and p"):
        ctx.score(lab, r=1.0)


def fake_result(paper, m=6):
    _, truth, P, orc = paper
    rng = np.random.default_rng(9)
    n = len(truth)
    clusts = [truth] + [np.where(rng.random(n) < 0.1, rng.integers(1, 11, n), truth) for _ in range(m - 1)]
    res = SimpleNamespace(clusts=clusts, r=rng.uniform(0.5, 2.0, m), p=rng.uniform(0.2, 0.8, m), params=dict(P))
    sizes = [R.clusters(z)[2] for z in clusts]
    scores = dict(blocks=[R.halves(orc.Dq, orc.Lq, z) for z in clusts], sizes=sizes, eD=orc.eD, eL=orc.eL)
    return res, scores


def test_reweight_under_the_same_params_is_uniform(paper):
    res, scores = fake_result(paper)
    m = len(res.clusts)
    w = rc.reweight(None, res, dict(res.params), scores=scores)
    assert np.array_equal(w["weights"], np.full(m, 1.0 / m)) and w["ess"] == m
    assert np.array_equal(w["logweights"], np.full(m, -np.log(m)))
    with pytest.raises(ValueError, match="want_blocks"):
        rc.reweight(None, res, res.params, scores=dict(scores, blocks=None))


def test_reweight_follows_the_oracle_under_other_params(paper):
    _, _, P, orc = paper
    res, scores = fake_result(paper)
    new = [dict(P, alpha=P["alpha"] * 1.5, sigma=2.0, u=3.0), dict(P, delta2=P["delta2"] * 0.8)]
    ws = rc.reweight(None, res, new, scores=scores)
    assert len(ws) == 2
    try:
        for Pn, w in zip(new, ws):
            lw = []
            for z, r, p in zip(res.clusts, res.r, res.p):
                orc.set_state(z)
                orc.set_params(Pn); a = orc.loglik_stable() + orc.logprior(r, p)
                orc.set_params(P); b = orc.loglik_stable() + orc.logprior(r, p)
                lw.append(a - b)
            lw = np.array(lw)
            ref = np.exp(lw - lw.max()); ref /= ref.sum()
            assert np.allclose(w["weights"], ref, rtol=1e-6, atol=0)
            assert abs(w["weights"].sum() - 1) < 1e-12 and 1 <= w["ess"] <= len(lw)
            assert np.isclose(w["ess"], 1.0 / (w["weights"] ** 2).sum(), rtol=1e-12)
    finally:
        orc.set_params(P)


def test_mapestimate_takes_the_first_of_tied_candidates():
    cands = np.array([[1, 1, 2], [1, 2, 2], [1, 2, 3], [3, 3, 3]], np.int64)
    sc = dict(loglik=np.array([0.0, 2.0, 2.0, 1.0]), logprior=np.array([1.0, 1.0, 1.0, 1.0]),
              logposterior=np.array([1.0, 3.0, 3.0, 2.0]), K=np.array([2, 2, 3, 1]), kernel_ms=0.0)
    clust, info = rc.mapestimate(None, cands, scores=sc)
    assert info["index"] == 1 and np.array_equal(clust, cands[1])
    with pytest.raises(ValueError, match="r and p"):
        rc.mapestimate(None, cands, scores=dict(sc, logposterior=None))


def test_hclustpointestimate_checks_the_new_criterion_first():
    with pytest.raises(ValueError, match="criterion"):
        rc.hclustpointestimate(np.zeros((2, 2), np.uint32), numsamples=1, criterion="likelihood")
    with pytest.raises(ValueError, match="needs data"):
        rc.hclustpointestimate(np.zeros((2, 2), np.uint32), numsamples=1, criterion="posterior", r=1.0, p=0.5)


def test_header_signatures_and_julia_agree():
    import test_oracle_cpu as T
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    protos = T._header_prototypes(hdr)
    want = {"rc_score_labellings": ["rc_ctx*", "int64_t", "int64_t*", "double*", "double*", "rc_params*", "double*", "double*", "int64_t*",
                                    "int64_t*", "int64_t", "int32_t*", "int32_t*", "double*"],
            "rc_loglik_from_blocks": ["int64_t", "int64_t", "int64_t*", "int64_t*", "int32_t", "int32_t", "rc_params*", "double*"]}
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for name, args in want.items():
        assert protos[name] == ("int32_t", args), protos[name]
        res, sig = rc.SIGNATURES[name]
        assert res is C.c_int32 and len(sig) == len(args)
        for k, (ct, py) in enumerate(zip(args, sig)):
            if ct in scalars:
                assert py is scalars[ct], (name, k, ct, py)
            else:
                assert py in (C.c_void_p, C.POINTER(_lib.RcParams), C.POINTER(C.c_double), C.POINTER(C.c_int32)), (name, k, ct, py)
        assert hasattr(rc.lib(), name)
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    calls = [c for c in T._julia_ccalls(jl) if c[0] == "rc_score_labellings"]
    assert len(calls) == 1
    _, jret, jargs, npassed = calls[0]
    assert jret == "Int32" and len(jargs) == npassed == 14
    for jt, ct in zip(jargs, want["rc_score_labellings"]):
        assert ct in T._JL2C[jt], (jt, ct)
    assert re.search(r"function scorelabellings\(b::HIPBackend, data::MCMCData,", jl) and "function mapestimate(b::HIPBackend" in jl
    assert "export scorelabellings, mapestimate" in jl
    T.test_julia_glue_ccalls_match_the_header()


def test_the_source_is_part_of_the_build():
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    assert '#include "score.inc.hip"' in open(os.path.join(csrc, "redclust_hip.hip")).read()
    assert os.path.join(csrc, "score.inc.hip") in _lib._sources()     # build() watches it
    src = re.sub(r"//.*", "", open(os.path.join(csrc, "score.inc.hip")).read())
    assert "asm" not in src                                           # plain C++ and vector memory operations only
    assert "slab::run_rows" in src and "rc_bin_add" in src            # the two halves are shared, not copied:
    assert "k_predict_sums" not in src and "launch_sums" not in src   # the sums come through the slab driver, which launches them
    slab = re.sub(r"//.*", "", open(os.path.join(csrc, "slab.inc.hip")).read())
    assert "asm" not in slab and "launch_sums" in slab.split("run_rows(", 1)[1]
