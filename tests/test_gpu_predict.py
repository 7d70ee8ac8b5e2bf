"""Predict on the GPU (csrc/predict.inc.hip through rc_predict and rc.predict) against the NumPy reference of
tests/predict_ref.py, whose decision gaps on exactly these inputs tests/test_predict_cpu.py keeps above 1e-6: integers and
labels must be equal, scores within tau = 2^-49·T (T: the sum of the absolute values of the score's terms — two logarithms
held to 2 ulp by test_gpu_logs.py are 2^-51 of their terms, about six roundings of 2^-53 follow: < 3.5·2^-51·T)."""
import ctypes as C

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import predict_ref as R

pytestmark = pytest.mark.gpu

TAU = 2.0 ** -49


def _run(c, Kmax, logD=True, **kw):
    args = dict(seed=c["seed"], sample_offset=c["sample_offset"], point_offset=c["point_offset"], Kmax=Kmax, want_scores=True,
                want_sums=True, logDnew=c["logDnew"] if logD else None)
    args.update(kw)
    return _lib.predict(c["Dnew"], c["samples"], c["r"], c["p"], c["P"], **args)


def _same_outputs(a, b):
    for k in ("labels", "map", "sums", "eD", "eL"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["scores"], b["scores"], equal_nan=True)


def _check_against_reference(out, ref):
    assert np.array_equal(out["eD"], ref["eD"]) and np.array_equal(out["eL"], ref["eL"])
    assert np.array_equal(out["sums"], ref["sums"])
    sc, rs = out["scores"], ref["scores"]
    assert sc.shape == rs.shape
    assert np.array_equal(np.isnan(sc), np.isnan(rs)) and np.array_equal(np.isneginf(sc), np.isneginf(rs))
    fin = np.isfinite(rs)
    assert np.all(np.isfinite(sc[fin]))
    err = np.abs(sc[fin] - rs[fin])
    print("largest score deviation / (2^-49 T):", float((err / (TAU * ref["T"][fin])).max()))
    assert np.all(err <= TAU * ref["T"][fin])
    assert np.array_equal(out["labels"], ref["labels"])
    assert np.array_equal(out["map"], ref["map"])


@pytest.mark.parametrize("shape", R.EDGE_SHAPES)
def test_exactness_at_the_edges(shape):
    c, ref = R.edge_case(*shape), R.edge_ref(*shape)
    out = _run(c, ref["Kmax"])
    _check_against_reference(out, ref)
    assert out["kernel_ms"] > 0
    # without the optional outputs Kmax is not read and the draws are the same
    bare = _lib.predict(c["Dnew"], c["samples"], c["r"], c["p"], c["P"], seed=c["seed"], sample_offset=c["sample_offset"],
                        point_offset=c["point_offset"], logDnew=c["logDnew"], Kmax=-5)
    assert np.array_equal(bare["labels"], ref["labels"]) and np.array_equal(bare["map"], ref["map"])


@pytest.mark.parametrize("shape", [(65, 2, 63), (257, 3, 1025)])     # samples cut into parts (atomic adds) / one part (stores)
def test_both_row_paths_give_the_same_bits(shape, monkeypatch):
    c, ref = R.edge_case(*shape), R.edge_ref(*shape)
    lds = _run(c, ref["Kmax"])
    monkeypatch.setenv("RC_PREDICT_ROWS_GLOBAL", "1")
    glob = _run(c, ref["Kmax"])
    _same_outputs(lds, glob)
    _check_against_reference(glob, ref)


def test_a_point_does_not_depend_on_its_company():
    c, ref = R.independence_case(), R.independence_ref()
    Kmax = ref["Kmax"]
    whole = _run(c, Kmax)
    _check_against_reference(whole, ref)
    m, q = 70, 5
    parts = {k: np.zeros_like(v) for k, v in whole.items() if isinstance(v, np.ndarray)}
    for s0, s1 in ((0, 64), (64, 70)):
        for i0, i1 in ((0, 2), (2, 5)):
            sub = dict(c, Dnew=c["Dnew"][i0:i1], logDnew=c["logDnew"][i0:i1], samples=c["samples"][s0:s1], r=c["r"][s0:s1], p=c["p"][s0:s1])
            o = _run(sub, Kmax, sample_offset=s0, point_offset=i0)
            for k in ("labels", "map", "sums", "scores"):
                parts[k][s0:s1, i0:i1] = o[k]
            parts["eD"][i0:i1], parts["eL"][i0:i1] = o["eD"], o["eL"]
    _same_outputs(whole, parts)


@pytest.mark.parametrize("kib", [4, 32])     # 4: one sample and one new point per launch; 32: a few samples, all points
def test_chunks_of_samples_and_points_give_the_same_bits(kib, monkeypatch):
    c, ref = R.independence_case(), R.independence_ref()
    whole = _run(c, ref["Kmax"])
    monkeypatch.setenv("RC_PREDICT_WORKSPACE_KIB", str(kib))
    chunked = _run(c, ref["Kmax"])
    _same_outputs(whole, chunked)
    _check_against_reference(chunked, ref)


def test_the_library_takes_the_logarithms_itself():
    shape = (63, 3, 2)
    c, ref = R.edge_case(*shape), R.edge_ref(*shape)
    given, own = _run(c, ref["Kmax"]), _run(c, ref["Kmax"], logD=False)
    assert np.array_equal(own["eD"], given["eD"]) and np.array_equal(own["eL"], given["eL"])
    assert np.array_equal(own["sums"][..., 0], given["sums"][..., 0])
    P = c["P"]
    cL = abs((P["delta1"] - 1) - (P["delta2"] - 1))
    # libm against NumPy in the last bit moves each of the n addends of S_L by at most one quantum 2^-eL
    slack = cL * shape[0] * np.ldexp(2.0, -given["eL"].astype(np.int64))[None, :, None]
    fin = np.isfinite(ref["scores"])
    bound = np.broadcast_to(TAU * ref["T"] + slack, ref["scores"].shape)
    assert np.array_equal(np.isnan(own["scores"]), np.isnan(given["scores"]))
    assert np.all(np.abs(own["scores"][fin] - given["scores"][fin]) <= bound[fin])
    assert np.max(np.abs(own["sums"][..., 1] - given["sums"][..., 1])) <= shape[0]


def test_draw_frequencies():
    c = R.frequency_case()
    cands, prob, ref_counts, _ = R.frequency_ref()
    m = c["m"]
    pred = rc.predict(np.tile(c["labels"], (m, 1)), c["Dnew"], r=np.full(m, c["r"]), p=np.full(m, c["p"]), params=c["P"], seed=c["seed"])
    assert pred.labels.shape == (m, 1)
    counts = np.array([(pred.labels[:, 0] == k).sum() for k in cands])
    print("drawn counts", counts, "reference", ref_counts, "expected", m * prob)
    assert counts.sum() == m
    assert R.within_4_sigma(counts, prob, m)
    assert np.array_equal(counts, ref_counts)                       # the gap guard makes every single draw a fair demand
    assert np.all(pred.map_labels == 2)
    assert abs(pred.new_cluster_frequency()[0] - ref_counts[3] / m) < 1e-12


def test_planted_holdout_through_the_public_surface():
    c, ref = R.holdout_case(), R.holdout_ref()
    pred = rc.predict(c["samples"], new_points=c["new_points"], points=c["points"], r=c["r"], p=c["p"], params=c["P"], scores=True)
    truth = c["truth_new"]
    assert np.array_equal(pred.labels[:, :30], np.stack([truth, truth])) and np.array_equal(pred.map_labels[:, :30], np.stack([truth, truth]))
    assert np.all(pred.labels[:, 30] == 0) and np.all(pred.map_labels[:, 30] == 0)
    assert np.array_equal(pred.labels, ref["labels"]) and np.array_equal(pred.map_labels, ref["map"])
    assert pred.scores.shape == (2, 31, 4) and np.all(np.isfinite(pred.scores))
    assert np.array_equal(pred.new_cluster_frequency(), np.r_[np.zeros(30), 1.0])
    E = pred.extended_samples(c["samples"])
    assert E.shape == (2, 151)
    counts = rc.posterior_counts(E)
    full = np.r_[c["samples"][0], truth]                            # the truth of training and held-out points together
    for i in range(30):
        mates = np.flatnonzero(full == truth[i])
        assert np.all(counts[120 + i, mates] == 2)
        assert np.all(counts[120 + i, np.flatnonzero(full != truth[i])] == 0)
    assert np.all(counts[150, :150] == 0) and counts[150, 150] == 2
    # chunked distances: the same result whatever the chunk
    import importlib
    M = importlib.import_module("redclust_amd.predict")
    old = M._DIST_CHUNK_BYTES
    try:
        M._DIST_CHUNK_BYTES = 8 * 120 * 3 * 7                       # seven new points per call
        again = rc.predict(c["samples"], new_points=c["new_points"], points=c["points"], r=c["r"], p=c["p"], params=c["P"], scores=True)
    finally:
        M._DIST_CHUNK_BYTES = old
    assert np.array_equal(again.labels, pred.labels) and np.array_equal(again.map_labels, pred.map_labels)
    assert np.array_equal(again.scores, pred.scores)


# ---------------------------------------------------------------------------------------------------------------
# errors: one case per class, all before any device work
# ---------------------------------------------------------------------------------------------------------------
def _raw(n=3, q=1, m=1, D=None, logD=None, S=None, r=None, p=None, P=None, device=0, Kmax=0, scores=False, null=()):
    D = np.ones((1, 3)) if D is None else np.ascontiguousarray(D, dtype=np.float64)
    S = np.array([[1, 1, 2]], np.int64) if S is None else np.ascontiguousarray(S, dtype=np.int64)
    r = np.array([1.0]) if r is None else np.ascontiguousarray(r, dtype=np.float64)
    p = np.array([0.5]) if p is None else np.ascontiguousarray(p, dtype=np.float64)
    P = dict(R.PARAMS, **(P or {}))
    prm = _lib.RcParams(P["delta1"], P["delta2"], P["alpha"], P["beta"], P["zeta"], P["gamma"], 1.0, 1.0, 1.0, 1.0, int(P["maxK"]), 1)
    labels = np.zeros((max(m, 1), max(q, 1)), np.int64)
    sc = np.zeros((max(m, 1), max(q, 1), Kmax + 1)) if scores else None
    Lg = None if logD is None else np.ascontiguousarray(logD, dtype=np.float64)
    ptr = dict(D=D.ctypes.data, logD=None if Lg is None else Lg.ctypes.data, S=S.ctypes.data, r=r.ctypes.data, p=p.ctypes.data,
               prm=C.byref(prm), labels=labels.ctypes.data)
    for k in null:
        ptr[k] = None
    L = rc.lib()
    code = L.rc_predict(device, n, q, ptr["D"], ptr["logD"], m, ptr["S"], ptr["r"], ptr["p"], ptr["prm"], 0, 0, 0, ptr["labels"], None,
                        Kmax, None if sc is None else sc.ctypes.data, None, None, None, None)
    return _lib.ERRORS.get(code, code), L.rc_last_error(None).decode()


def test_the_plain_call_of_the_error_helper_succeeds():
    assert _raw()[0] == 0


@pytest.mark.parametrize("kw", [dict(null=("D",)), dict(null=("S",)), dict(null=("r",)), dict(null=("p",)), dict(null=("prm",)),
                                dict(null=("labels",)), dict(n=0), dict(q=0), dict(m=0), dict(S=[[1, 4, 2]]), dict(S=[[0, 1, 2]]),
                                dict(r=[0.0]), dict(r=[np.inf]), dict(r=[np.nan]), dict(p=[0.0]), dict(p=[1.0]), dict(P=dict(alpha=0.0)),
                                dict(P=dict(gamma=-1.0)), dict(P=dict(maxK=-1)), dict(device=99), dict(scores=True, Kmax=1)])
def test_argument_errors(kw):
    code, msg = _raw(**kw)
    assert code == "RC_ERR_ARG" and msg.startswith("rc_predict"), (code, msg)


@pytest.mark.parametrize("kw", [dict(D=[[1.0, 0.0, 1.0]]), dict(D=[[1.0, -2.0, 1.0]]), dict(D=[[1.0, np.inf, 1.0]]), dict(D=[[np.nan, 1.0, 1.0]]),
                                dict(logD=[[0.0, np.inf, 0.0]]), dict(logD=[[0.0, 0.0, np.nan]])])
def test_domain_errors(kw):
    code, msg = _raw(**kw)
    assert code == "RC_ERR_DOMAIN" and msg.startswith("rc_predict"), (code, msg)


@pytest.mark.parametrize("kw", [dict(n=32768), dict(n=32767, m=65539)])
def test_capacity_errors_come_first_and_need_no_large_allocation(kw):
    code, msg = _raw(**kw)                                           # the arrays are the three-point ones: nothing of them is read
    assert code == "RC_ERR_CAPACITY" and msg.startswith("rc_predict"), (code, msg)
