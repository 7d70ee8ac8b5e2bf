"""Joint predict on the GPU (csrc/predictjoint.inc.hip through rc_predict_joint and rc.predict_joint) against the NumPy reference
of tests/predict_joint_ref.py, whose decision gaps on exactly these inputs tests/test_predict_joint_cpu.py keeps above 1e-6 (the
device's scores deviate by about 1e-12): labels, counts and integer sums must be equal."""
import ctypes as C

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import predict_ref as R
import predict_joint_ref as J

pytestmark = pytest.mark.gpu

KEYS = ("labels", "first", "K", "moves", "sums", "eD", "eL")


def _run(c, logD=True, **kw):
    args = dict(sweeps=c["sweeps"], seed=c["seed"], sample_offset=c["sample_offset"], want_sums=True,
                logDnew=c["logDnew"] if logD else None, logDnn=c["logDnn"] if logD else None)
    args.update(kw)
    return _lib.predict_joint(c["Dnew"], c["Dnn"], c["samples"], c["r"], c["p"], c["P"], **args)


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", J.EDGE_SHAPES)
def test_exactness_at_the_edges(shape):
    c, ref = J.edge_case(*shape), J.edge_ref(*shape)
    out = _run(c)
    _same(out, ref)
    assert out["kernel_ms"] > 0
    bare = _run(c, want_sums=False, want_first=False, want_moves=False)      # without the optional outputs: the same draws
    assert bare["first"] is None and bare["moves"] is None
    _same(bare, ref, ("labels", "K"))


def test_splitting_the_samples_changes_no_bit():
    c, ref = J.split_case(), J.split_ref()
    whole = _run(c)
    _same(whole, ref)
    parts = {k: np.zeros_like(whole[k]) for k in KEYS}
    for s0, s1 in ((0, 64), (64, 70)):
        sub = dict(c, samples=c["samples"][s0:s1], r=c["r"][s0:s1], p=c["p"][s0:s1])
        o = _run(sub, sample_offset=s0)
        for k in ("labels", "first", "K", "moves", "sums"):
            parts[k][s0:s1] = o[k]
        parts["eD"], parts["eL"] = o["eD"], o["eL"]
    _same(whole, parts)


def test_one_sample_per_launch_gives_the_same_bits(monkeypatch):
    shape = (65, 65, 5, 2)
    c, ref = J.edge_case(*shape), J.edge_ref(*shape)
    whole = _run(c)
    # the base sums of one sample take q·16·K_s >= 1040 bytes here: a workspace of 1 KiB holds one sample, which always goes
    monkeypatch.setenv("RC_PREDICT_WORKSPACE_KIB", "1")
    chunked = _run(c)
    _same(whole, chunked)
    _same(chunked, ref)


def test_the_library_takes_the_logarithms_itself():
    shape = (63, 3, 2, 1)
    c, ref = J.edge_case(*shape), J.edge_ref(*shape)
    given, own = _run(c), _run(c, logD=False)
    assert np.array_equal(own["eD"], given["eD"]) and np.array_equal(own["eL"], given["eL"])
    assert np.array_equal(own["sums"][..., 0], given["sums"][..., 0])
    # libm against NumPy in the last bit moves each of the n + q addends of S_L by at most one quantum 2^-eL: the scores by
    # cL·(n+q)·2^(1-eL), which tests/test_predict_joint_cpu.py holds the reference's gap on this input above
    _same(own, given, ("labels", "first", "K", "moves"))
    assert np.max(np.abs(own["sums"][..., 1] - given["sums"][..., 1])) <= shape[0] + shape[1]


def test_draw_frequencies():
    c = J.frequency_case()
    outcomes, prob, ref_counts, _ = J.frequency_ref()
    m = c["m"]
    jp = rc.predict_joint(np.tile(c["labels"], (m, 1)), c["Dnew"], c["Dnn"], sweeps=0, r=np.full(m, c["r"]), p=np.full(m, c["p"]),
                          params=c["P"], seed=c["seed"])
    assert jp.labels.shape == (m, 2) and np.array_equal(jp.labels, jp.first_labels)
    counts = np.array([np.count_nonzero((jp.labels[:, 0] == a) & (jp.labels[:, 1] == b)) for a, b in outcomes])
    print("drawn counts", counts, "reference", ref_counts)
    assert counts.sum() == m
    assert R.within_4_sigma(counts, prob, m)
    assert np.array_equal(counts, ref_counts)                       # the gap guard makes every single draw a fair demand
    assert np.all(jp.moves == 2)


def test_planted_holdout_through_the_public_surface():
    c, ref = J.holdout_case(), J.holdout_ref()
    jp = rc.predict_joint(c["samples"], new_points=c["new_points"], points=c["points"], sweeps=c["sweeps"], r=c["r"], p=c["p"],
                          params=c["P"], seed=c["seed"])
    assert np.array_equal(jp.labels, ref["labels"]) and np.array_equal(jp.first_labels, ref["first"])
    assert np.array_equal(jp.K, ref["K"]) and np.array_equal(jp.moves, ref["moves"])
    m = len(c["samples"])
    E = jp.extended_samples(c["samples"])
    assert E.shape == (m, 150)
    counts = rc.posterior_counts(E)
    unseen = 120 + np.flatnonzero(c["unseen"])
    assert len(unseen) == 12 and np.all(counts[np.ix_(unseen, unseen)] == m)
    assert np.all(counts[unseen, :120] == 0)
    assert np.array_equal(jp.new_cluster_frequency(c["samples"]), c["unseen"].astype(float))


# ---------------------------------------------------------------------------------------------------------------
# errors: one case per class, all before any device work
# ---------------------------------------------------------------------------------------------------------------
def _raw(n=3, q=2, m=1, D=None, Dn=None, logD=None, logDn=None, S=None, r=None, p=None, P=None, device=0, sweeps=1, null=()):
    D = np.ones((2, 3)) if D is None else np.ascontiguousarray(D, dtype=np.float64)
    Dn = np.array([[0.0, 2.0], [2.0, 0.0]]) if Dn is None else np.ascontiguousarray(Dn, dtype=np.float64)
    S = np.array([[1, 1, 2]], np.int64) if S is None else np.ascontiguousarray(S, dtype=np.int64)
    r = np.array([1.0]) if r is None else np.ascontiguousarray(r, dtype=np.float64)
    p = np.array([0.5]) if p is None else np.ascontiguousarray(p, dtype=np.float64)
    P = dict(R.PARAMS, **(P or {}))
    prm = _lib.RcParams(P["delta1"], P["delta2"], P["alpha"], P["beta"], P["zeta"], P["gamma"], 1.0, 1.0, 1.0, 1.0, int(P["maxK"]), 1)
    labels = np.full((max(m, 1), max(q, 1)), -7, np.int64)
    K = np.zeros(max(m, 1), np.int64)
    Lg = None if logD is None else np.ascontiguousarray(logD, dtype=np.float64)
    Ln = None if logDn is None else np.ascontiguousarray(logDn, dtype=np.float64)
    ptr = dict(D=D.ctypes.data, Dn=Dn.ctypes.data, logD=None if Lg is None else Lg.ctypes.data, logDn=None if Ln is None else Ln.ctypes.data,
               S=S.ctypes.data, r=r.ctypes.data, p=p.ctypes.data, prm=C.byref(prm), labels=labels.ctypes.data, K=K.ctypes.data)
    for k in null:
        ptr[k] = None
    L = rc.lib()
    code = L.rc_predict_joint(device, n, q, ptr["D"], ptr["Dn"], ptr["logD"], ptr["logDn"], m, ptr["S"], ptr["r"], ptr["p"], ptr["prm"],
                              sweeps, 0, 0, ptr["labels"], None, ptr["K"], None, None, None, None, None)
    return _lib.ERRORS.get(code, code), L.rc_last_error(None).decode(), labels


def test_the_plain_call_of_the_error_helper_succeeds():
    code, _, labels = _raw()
    assert code == 0 and labels.min() >= 1 and labels.max() <= 5


@pytest.mark.parametrize("kw", [dict(null=("D",)), dict(null=("Dn",)), dict(null=("S",)), dict(null=("r",)), dict(null=("p",)),
                                dict(null=("prm",)), dict(null=("labels",)), dict(null=("K",)), dict(n=0), dict(q=0), dict(m=0),
                                dict(S=[[1, 4, 2]]), dict(S=[[0, 1, 2]]), dict(r=[0.0]), dict(r=[np.inf]), dict(r=[np.nan]),
                                dict(r=[1e-310]), dict(p=[0.0]), dict(p=[1.0]), dict(P=dict(alpha=0.0)), dict(P=dict(maxK=-1)),
                                dict(device=99), dict(sweeps=-1), dict(sweeps=2 ** 31 - 1), dict(logD=np.zeros((2, 3))),
                                dict(logDn=np.zeros((2, 2)))])
def test_argument_errors(kw):
    code, msg, _ = _raw(**kw)
    assert code == "RC_ERR_ARG" and msg.startswith("rc_predict_joint"), (code, msg)


@pytest.mark.parametrize("kw", [dict(D=[[1.0, 0.0, 1.0], [1.0, 1.0, 1.0]]), dict(D=[[1.0, 1.0, 1.0], [1.0, np.inf, 1.0]]),
                                dict(D=[[np.nan, 1.0, 1.0], [1.0, 1.0, 1.0]]), dict(Dn=[[0.0, 2.0], [3.0, 0.0]]),
                                dict(Dn=[[0.0, 0.0], [0.0, 0.0]]), dict(Dn=[[0.0, -1.0], [-1.0, 0.0]]),
                                dict(Dn=[[0.0, np.inf], [np.inf, 0.0]]), dict(Dn=[[0.0, np.nan], [np.nan, 0.0]]),
                                dict(logD=[[0.0, np.inf, 0.0], [0.0, 0.0, 0.0]], logDn=np.zeros((2, 2))),
                                dict(logD=np.zeros((2, 3)), logDn=[[0.0, np.nan], [np.nan, 0.0]])])
def test_domain_errors(kw):
    code, msg, _ = _raw(**kw)
    assert code == "RC_ERR_DOMAIN" and msg.startswith("rc_predict_joint"), (code, msg)


def test_the_diagonal_of_dnn_is_ignored():
    a = _raw(logD=np.zeros((2, 3)), logDn=[[np.nan, 0.7], [0.7, np.inf]], Dn=[[np.nan, 2.0], [2.0, -1.0]])
    b = _raw(logD=np.zeros((2, 3)), logDn=[[0.0, 0.7], [0.7, 0.0]])
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("kw", [dict(n=32768), dict(n=32767, m=65539), dict(q=4096), dict(q=4095), dict(q=5000, sweeps=0)])
def test_capacity_errors_launch_nothing_and_need_no_large_allocation(kw):
    code, msg, labels = _raw(**kw)                                   # the arrays are the small ones: nothing of them is read
    assert code == "RC_ERR_CAPACITY" and msg.startswith("rc_predict_joint"), (code, msg)
    assert np.all(labels == -7)                                      # nothing ran


def test_a_capacity_error_names_the_sample():
    S = np.stack([np.ones(4000, np.int64), np.arange(1, 4001)])      # K = 1 fits with q = 96, K = 4000 does not
    code, msg, _ = _raw(n=4000, q=97, m=2, S=S, r=[1.0, 1.0], p=[0.5, 0.5])
    assert code == "RC_ERR_CAPACITY" and "sample 2" in msg, (code, msg)


def test_determinism_and_isolation():
    c = J.edge_case(64, 64, 3, 2)
    pc = R.independence_case()

    def indep():
        return _lib.predict(pc["Dnew"], pc["samples"], pc["r"], pc["p"], pc["P"], seed=pc["seed"], logDnew=pc["logDnew"])

    before = indep()
    a = _run(c)
    after = indep()
    b = _run(c)
    _same(a, b)
    for k in ("labels", "map", "eD", "eL"):
        assert np.array_equal(before[k], after[k]), k
    assert np.array_equal(before["labels"], R.independence_ref()["labels"])
