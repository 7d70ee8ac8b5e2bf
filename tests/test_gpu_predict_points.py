"""Predict from points on the GPU (csrc/predictpoints.inc.hip through rc_predict_points and rc.predict_points): the distances
bit for bit against the restatement of tests/predict_points_ref.py, the logarithms against the resolver's own, everything
after them against rc_predict on those distances and logarithms, the chunking, the counts against the host's allocation
table, and the errors."""
import ctypes as C

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import predict_points_ref as R

pytestmark = pytest.mark.gpu

ONE = dict(r=np.array([1.0]), p=np.array([0.5]), params=R.PR.PARAMS)


def _dist_log(X, Y):
    S = np.ones((1, len(X)), np.int64)
    out = _lib.predict_points(X, Y, S, ONE["r"], ONE["p"], ONE["params"], want_dist=True, want_log=True)
    return out["dist"], out["log"]


# ---------------------------------------------------------------------------------------------------------------
# distances and logarithms, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.DIST_SHAPES)
def test_distances_equal_the_restatement_and_logs_the_resolvers(shape):
    X, Y, ref = R.dist_case(*shape)
    D, L = _dist_log(X, Y)
    assert D.shape == ref.shape
    bad = np.flatnonzero(D.view(np.uint64).ravel() != ref.view(np.uint64).ravel())
    print("distances that differ:", len(bad), "of", ref.size)
    assert len(bad) == 0, (bad[:5], D.ravel()[bad[:5]], ref.ravel()[bad[:5]])
    ctx = rc.Context(np.array([[0.0, 1.0], [1.0, 0.0]]))
    try:
        own = ctx.debug_flog(0, D)
    finally:
        ctx.close()
    assert np.array_equal(L.view(np.uint64), own.view(np.uint64))


@pytest.mark.parametrize("e", [100, -100])
def test_scaling_by_a_power_of_two_scales_every_distance_exactly(e):
    X, Y, ref = R.dist_case(65, 17, 65)
    s = np.ldexp(1.0, e)
    D, _ = _dist_log(X * s, Y * s)
    assert np.array_equal(D, ref * s)


# ---------------------------------------------------------------------------------------------------------------
# equals rc_predict on its own distances and logarithms
# ---------------------------------------------------------------------------------------------------------------
def _points(c, counts=None, sl=slice(None), point_offset=None, **kw):
    args = dict(seed=c["seed"], sample_offset=c["sample_offset"], point_offset=c["point_offset"] if point_offset is None else point_offset,
                Kmax=c["Kmax"], want_scores=True, want_sums=True, want_dist=True, want_log=True)
    if counts is not None:
        args.update(maps=counts["maps"], pivot_labels=counts["pivot_labels"], want_counts=True, want_mapcounts=True)
    args.update(kw)
    return _lib.predict_points(c["X"], c["Y"][sl], c["samples"], c["r"], c["p"], c["P"], **args)


def _same(a, b, keys=("labels", "map", "sums", "eD", "eL", "dist", "log", "counts", "mapcounts")):
    for k in keys:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["scores"], b["scores"], equal_nan=True)


@pytest.mark.parametrize("repulsion", [True, False])
def test_equals_rc_predict_on_its_distances_and_logs(repulsion):
    c = R.predict_case(repulsion)
    out = _points(c)
    assert out["kernel_ms"] > 0
    assert np.array_equal(out["dist"][:3].view(np.uint64), R.distances(c["Y"][:3], c["X"]).view(np.uint64))
    ref = _lib.predict(out["dist"], c["samples"], c["r"], c["p"], c["P"], seed=c["seed"], sample_offset=c["sample_offset"],
                       point_offset=c["point_offset"], logDnew=out["log"], Kmax=c["Kmax"], want_scores=True, want_sums=True)
    for k in ("labels", "map", "sums", "eD", "eL"):
        assert np.array_equal(out[k], ref[k]), k
    assert np.array_equal(out["scores"].view(np.uint64), ref["scores"].view(np.uint64))
    # the case does what it is for: a new cluster is offered for some samples and not for others, and both kinds of label are drawn
    offered = np.isfinite(out["scores"][:, 0, -1])
    assert offered.any() and not offered.all()
    assert np.array_equal(offered, c["K"] < 4)
    assert (out["labels"] > 0).any()


# ---------------------------------------------------------------------------------------------------------------
# chunking
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def relabelling():
    c = R.predict_case()
    out = _lib.relabel(c["samples"], R.pivot_of_case())
    return dict(maps=out["maps"], pivot_labels=out["pivot_labels"])


@pytest.fixture(scope="module")
def whole(relabelling):
    return _points(R.predict_case(), relabelling)


@pytest.mark.parametrize("kib", [64, 512])       # 64: one sample and about eight new points per launch; 512: a few samples, all points
def test_chunks_of_samples_and_points_give_the_same_bits(kib, whole, relabelling, monkeypatch):
    monkeypatch.setenv("RC_PREDICT_WORKSPACE_KIB", str(kib))
    _same(whole, _points(R.predict_case(), relabelling))


def test_rows_from_global_memory_give_the_same_bits(whole, relabelling, monkeypatch):
    monkeypatch.setenv("RC_PREDICT_ROWS_GLOBAL", "1")
    _same(whole, _points(R.predict_case(), relabelling))


def test_two_halves_with_point_offset_give_the_same_bits(whole, relabelling):
    c = R.predict_case()
    a = _points(c, relabelling, slice(0, 33))
    b = _points(c, relabelling, slice(33, None), point_offset=c["point_offset"] + 33)
    for k in ("labels", "map", "sums", "scores"):
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), whole[k], equal_nan=True), k
    for k in ("eD", "eL", "dist", "log", "counts", "mapcounts"):
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=0), whole[k]), k


# ---------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------
def test_counts_equal_the_hosts_allocation_table(whole):
    c = R.predict_case()
    m, q = c["m"], c["q"]
    rel = rc.relabel(c["samples"], R.pivot_of_case())
    assert len(rel.pivot_labels) == 3 and (c["K"] > 3).any()
    for key, lab in (("counts", whole["labels"]), ("mapcounts", whole["map"])):
        host = rc.Prediction(lab, lab).allocation(rel, c["samples"])
        assert whole[key].dtype == np.uint32 and whole[key].shape == (q, 4)
        assert np.array_equal(whole[key], np.rint(host * m).astype(np.uint32)), key
        assert np.all(whole[key].sum(axis=1) == m)
    assert whole["counts"][:, 0].sum() > 0 and whole["counts"][:, 1:].sum() > 0          # column 0 and the pivot's are both populated
    # counts only: no labels, no map
    bare = _points(c, dict(maps=rel.maps, pivot_labels=rel.pivot_labels), want_labels=False, want_map=False, want_scores=False,
                   want_sums=False, want_dist=False, want_log=False, Kmax=0)
    assert bare["labels"] is None and bare["map"] is None
    assert np.array_equal(bare["counts"], whole["counts"]) and np.array_equal(bare["mapcounts"], whole["mapcounts"])


def test_the_public_surface(whole):
    c = R.predict_case()
    rel = rc.relabel(c["samples"], R.pivot_of_case() + 1000)        # a pivot whose names lie above n
    kw = dict(r=c["r"], p=c["p"], params=c["P"], seed=c["seed"])
    plain = _points(c, sample_offset=0, point_offset=0)
    pred = rc.predict_points(c["samples"], c["X"], c["Y"], **kw)
    assert pred.counts is None and np.array_equal(pred.labels, plain["labels"]) and np.array_equal(pred.map_labels, plain["map"])
    only = rc.predict_points(c["samples"], c["X"], c["Y"], relabelling=rel, **kw)
    assert only.labels is None and only.map_labels is None and np.array_equal(only.pivot_labels, [1005, 1050, 1120])
    assert np.array_equal(only.probabilities(), rc.Prediction(plain["labels"], plain["map"]).allocation(rel, c["samples"]))
    assert np.array_equal(only.allocation_counts().sum(axis=1), np.full(c["q"], c["m"]))
    best = np.argmax(only.counts, axis=1)
    assert np.array_equal(only.hard_allocation(), np.r_[0, rel.pivot_labels][best])
    both = rc.predict_points(c["samples"], c["X"], c["Y"], relabelling=rel, keep_labels=True, scores=True, **kw)
    assert np.array_equal(both.labels, plain["labels"]) and np.array_equal(both.counts, only.counts)
    assert np.array_equal(both.map_counts, only.map_counts)
    assert np.array_equal(both.scores, plain["scores"], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------
def _raw(n=3, dim=2, q=2, m=1, X=None, Y=None, S=None, maps=None, W=2, pivot=None, Kp=2, counts=False, labels=True, device=0, null=()):
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0]]) if X is None else np.ascontiguousarray(X, dtype=np.float64)
    Y = np.array([[0.5, 0.5], [3.0, 1.0]]) if Y is None else np.ascontiguousarray(Y, dtype=np.float64)
    S = np.array([[1, 1, 2]], np.int64) if S is None else np.ascontiguousarray(S, dtype=np.int64)
    r, p = np.array([1.0]), np.array([0.5])
    P = R.PR.PARAMS
    prm = _lib.RcParams(P["delta1"], P["delta2"], P["alpha"], P["beta"], P["zeta"], P["gamma"], 1.0, 1.0, 1.0, 1.0, 0, 1)
    lab = np.zeros((max(m, 1), max(q, 1)), np.int64)
    cnt = np.zeros((max(q, 1), max(Kp, 0) + 1), np.uint32)
    mp = None if maps is None else np.ascontiguousarray(maps, dtype=np.int64)
    pv = None if pivot is None else np.ascontiguousarray(pivot, dtype=np.int64)
    ptr = dict(X=X.ctypes.data, Y=Y.ctypes.data, S=S.ctypes.data, r=r.ctypes.data, p=p.ctypes.data, prm=C.byref(prm),
               labels=lab.ctypes.data if labels else None, maps=None if mp is None else mp.ctypes.data,
               pivot=None if pv is None else pv.ctypes.data, counts=cnt.ctypes.data if counts else None)
    for k in null:
        ptr[k] = None
    L = rc.lib()
    code = L.rc_predict_points(device, n, dim, ptr["X"], q, ptr["Y"], m, ptr["S"], ptr["r"], ptr["p"], ptr["prm"], 0, 0, 0, ptr["labels"], None,
                               ptr["maps"], W, ptr["pivot"], Kp, ptr["counts"], None, 0, None, None, None, None, None, None, None)
    return _lib.ERRORS.get(code, code), L.rc_last_error(None).decode(), cnt


def test_the_plain_calls_of_the_error_helper_succeed():
    assert _raw()[0] == 0
    code, _, cnt = _raw(counts=True, labels=False, maps=[[2, 0]], pivot=[1, 2])
    assert code == 0 and np.all(cnt.sum(axis=1) == 1)


def test_a_new_point_on_a_training_point_is_named():
    code, msg, _ = _raw(Y=[[0.5, 0.5], [0.0, 2.0]])
    assert code == "RC_ERR_DOMAIN" and msg.startswith("rc_predict_points") and "new point 2 " in msg and "training point 3" in msg, (code, msg)
    c = R.predict_case()
    Y = c["Y"].copy()
    Y[41], Y[60] = c["X"][150], c["X"][3]                           # the first in row-major order is (42, 151)
    with pytest.raises(rc.RedClustDomainError, match=r"new point 42 coincides with training point 151"):
        _lib.predict_points(c["X"], Y, c["samples"], c["r"], c["p"], c["P"])


@pytest.mark.parametrize("e", [600, -600])
def test_a_scale_that_overflows_or_underflows_the_square_is_a_domain_error(e):
    X, Y, _ = R.dist_case(65, 17, 65)
    s = np.ldexp(1.0, e)
    with pytest.raises(rc.RedClustDomainError, match="rc_predict_points"):
        _lib.predict_points(X * s, Y * s, np.ones((1, 65), np.int64), ONE["r"], ONE["p"], ONE["params"])
    assert _dist_log(X, Y)[0].shape == (65, 65)                     # the device is as it was


@pytest.mark.parametrize("kw", [dict(Y=[[0.5, np.nan], [3.0, 1.0]]), dict(X=[[0.0, 0.0], [np.inf, 0.0], [0.0, 2.0]])])
def test_a_coordinate_that_is_not_finite_is_a_domain_error(kw):
    code, msg, _ = _raw(**kw)
    assert code == "RC_ERR_DOMAIN" and msg.startswith("rc_predict_points"), (code, msg)


@pytest.mark.parametrize("kw", [dict(dim=0), dict(dim=(1 << 20) + 1), dict(null=("X",)), dict(null=("Y",)), dict(null=("S",)), dict(null=("prm",)),
                                dict(labels=False), dict(n=0), dict(q=0), dict(m=0), dict(S=[[1, 4, 2]]), dict(device=99),
                                dict(counts=True, pivot=[1, 2]), dict(counts=True, maps=[[2, 0]]),
                                dict(counts=True, maps=[[2, 0]], pivot=[1, 2], W=1), dict(counts=True, maps=[[2, 0]], pivot=[2, 1]),
                                dict(counts=True, maps=[[2, 0]], pivot=[1, 4]), dict(counts=True, maps=[[3, 0]], pivot=[1, 2]),
                                dict(counts=True, maps=[[2, -1]], pivot=[1, 2]), dict(counts=True, maps=[[2, 0]], pivot=[1, 2], Kp=0)])
def test_argument_errors(kw):
    code, msg, _ = _raw(**kw)
    assert code == "RC_ERR_ARG" and msg.startswith("rc_predict_points"), (code, msg)


@pytest.mark.parametrize("kw", [dict(n=32768), dict(n=32767, m=65539)])
def test_capacity_errors_come_first_and_need_no_large_allocation(kw):
    z = np.zeros((3, 2))
    code, msg, _ = _raw(X=z, Y=z[:2], S=np.zeros((1, 3), np.int64), **kw)       # all-zero three-point arrays: nothing of them is read
    assert code == "RC_ERR_CAPACITY" and msg.startswith("rc_predict_points"), (code, msg)
