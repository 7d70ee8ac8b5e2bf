"""rc_relabel on the device against the NumPy restatement (relabel_ref.py), bit for bit — every output is an integer — in the
default mode, with the table forced into the global slab, and with a workspace of 1 KiB (chunks of one sample).  Then the
Python layer built on it: relabel and Prediction.allocation."""
import ctypes as C_
import functools

import numpy as np
import pytest

import predict_ref as P
import psm_search_ref as R
import relabel_ref as RL
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "global": {"RC_RELABEL_TABLE_GLOBAL": "1"}, "chunked": {"RC_RELABEL_WORKSPACE_KIB": "1"}}


def _spread(z, n, seed):
    """z under other names, spread up to n (n itself is used)"""
    names = np.unique(z)
    new = np.sort(np.random.default_rng(seed).choice(np.arange(1, n), len(names) - 1, replace=False)) if len(names) > 1 else np.zeros(0, np.int64)
    new = np.concatenate([new, [n]]).astype(np.int64)
    return new[np.random.default_rng(seed + 1).permutation(len(names))][np.searchsorted(names, z)]


def _small(n, m, seed):
    rng = np.random.default_rng(seed)
    S = np.stack([rng.integers(1, min(n, 2 + s % 9) + 1, n) for s in range(m)]).astype(np.int64)
    S[m // 2] = _spread(S[m // 2], n, seed)
    return S, rng.integers(1, min(n, 5) + 1, n).astype(np.int64)


def _planted(pivot):
    n, m = 777, 37
    S = R.planted_counts(n, m, 20, 0.2, seed=1777)[0]
    if pivot == "one":
        c = np.ones(n, np.int64)
    elif pivot.startswith("cut"):                                      # fewer (5), as many (20) and more (40) clusters than the samples
        c = _lib.hclust_cut(_lib.hclust(None, m, 0, samples=S)["merges"], n, int(pivot[3:]))
    elif pivot == "sample":
        c = S[11].copy()
    else:
        c = _spread(S[3], n, 7)
    return S, c


def _ties():
    j = np.arange(16384)
    return np.stack([j // 128 + 1, (16383 - j) // 128 + 1]).astype(np.int64), (j % 128 + 1).astype(np.int64)


def _wide(n, K, seed):
    """a labelling of exactly K clusters under random names"""
    rng = np.random.default_rng(seed)
    z = np.concatenate([np.arange(K), rng.integers(0, K, n - K)])
    return (rng.permutation(n)[:K] + 1)[rng.permutation(z)].astype(np.int64)


CASES = {
    "n1": lambda: (np.ones((3, 1), np.int64), np.ones(1, np.int64)),
    "n63": lambda: _small(63, 5, 63), "n64": lambda: _small(64, 5, 64), "n65": lambda: _small(65, 5, 65),
    "m130": lambda: _small(65, 130, 130),
    "planted-one": lambda: _planted("one"), "planted-cut5": lambda: _planted("cut5"), "planted-cut20": lambda: _planted("cut20"),
    "planted-cut40": lambda: _planted("cut40"), "planted-sample": lambda: _planted("sample"), "planted-spread": lambda: _planted("spread"),
    "ties": _ties,
    # all singletons against all-one, and the reverse
    "singletons-vs-one": lambda: (np.stack([np.random.default_rng(1).permutation(300) + 1, np.arange(1, 301)]).astype(np.int64), np.ones(300, np.int64)),
    "one-vs-singletons": lambda: (np.stack([np.full(300, 7), np.full(300, 300)]).astype(np.int64), np.random.default_rng(2).permutation(300) + 1),
    # K_p = 1024: against 16 clusters the table (16 × 1024 cells) is in LDS by default, against singletons (1024 × 1024) it cannot be
    "kp1024-vs-16": lambda: (np.stack([_wide(1024, 16, 3), _wide(1024, 16, 4)]), np.arange(1, 1025)),
    "kp1024-vs-singletons": lambda: (np.stack([np.random.default_rng(5).permutation(1024) + 1, np.arange(1, 1025)]).astype(np.int64),
                                     (np.random.default_rng(6).permutation(1024) + 1).astype(np.int64)),
    # the LDS budget: vectors and table take 24·252 + 250·250·2 = 131048 of 131072 bytes at K_p = K_s = 250 (the largest launch with
    # the table in LDS), 24·252 + 250·252·2 = 132048 at K_s = 251 (the slab)
    "lds-edge-250": lambda: (np.stack([_wide(1500, 250, 8)]), _wide(1500, 250, 9)),
    "lds-edge-251": lambda: (np.stack([_wide(1500, 251, 10), _wide(1500, 250, 8)]), _wide(1500, 250, 9)),
    # one cell of 32767, the 16-bit edge
    "n32767": lambda: (np.stack([np.full(32767, 5), np.full(32767, 32767)]).astype(np.int64), np.full(32767, 9, np.int64)),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """(samples, pivot, reference outputs) of a case; computed once and shared (never modified)"""
    S, c = CASES[name]()
    S, c = np.ascontiguousarray(S, np.int64), np.ascontiguousarray(c, np.int64)
    ref = RL.relabel_ref(S, c)
    for a in (S, c) + tuple(ref.values()):
        a.setflags(write=False)
    return S, c, ref


def assert_equals_reference(got, ref, S, c, rows=slice(None)):
    m, n = S.shape
    for key in ("labels", "overlap"):
        assert got[key].dtype == np.int64 and np.array_equal(got[key], ref[key][rows]), key
    W = got["maps"].shape[1]                                         # the largest K_s of the call's samples
    assert got["maps"].dtype == np.int64 and np.array_equal(got["maps"], ref["maps"][rows][:, :W]) and np.all(ref["maps"][rows][:, W:] == -1)
    assert np.array_equal(got["pivot_labels"], ref["pivot_labels"])
    if rows == slice(None):
        assert got["counts"].dtype == np.uint32 and np.array_equal(got["counts"], ref["counts"]), "counts"
    # invariants
    assert np.array_equal(got["counts"].sum(1), np.full(n, len(got["overlap"])))
    assert np.all(got["overlap"] <= n) and np.all(got["overlap"] >= 1)
    for s, z in enumerate(S[rows]):
        names = np.unique(z)
        assert np.array_equal(got["labels"][s], got["maps"][s][np.searchsorted(names, z)])
        assert np.all(got["maps"][s, len(names):] == -1)
        assert got["overlap"][s] == np.sum(got["labels"][s] == c)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_every_output_equals_the_reference_bit_for_bit(name, mode, monkeypatch):
    S, c, ref = problem(name)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    got = _lib.relabel(S, c)
    print(name, mode, "kernel_ms", got["kernel_ms"])
    assert_equals_reference(got, ref, S, c)


def test_the_cases_cover_what_they_claim():
    K = lambda name: (len(np.unique(problem(name)[1])), [len(np.unique(z)) for z in problem(name)[0]])
    assert K("planted-cut5")[0] < min(K("planted-cut5")[1]) and K("planted-cut40")[0] > max(K("planted-cut40")[1])
    assert K("planted-cut20")[0] in K("planted-cut20")[1] and K("planted-sample")[0] in K("planted-sample")[1]
    assert problem("planted-spread")[1].max() == 777
    assert K("ties") == (128, [128, 128]) and K("kp1024-vs-16") == (1024, [16, 16]) and K("kp1024-vs-singletons") == (1024, [1024, 1024])
    assert K("lds-edge-250") == (250, [250]) and K("lds-edge-251") == (250, [251, 250])
    assert problem("n32767")[2]["overlap"].tolist() == [32767, 32767]
    assert problem("ties")[2]["overlap"].tolist() == [128, 128]      # a table of ones: whatever is matched, 128 points agree


@pytest.mark.parametrize("mode", MODES)
def test_one_sample_and_a_sample_on_its_own(mode, monkeypatch):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    for name in ("n65", "planted-cut5", "lds-edge-251"):
        S, c, ref = problem(name)
        for s in sorted({0, len(S) // 2, len(S) - 1}):               # m = 1: the same row as within the batch
            one = _lib.relabel(S[s:s + 1], c)
            assert_equals_reference(one, ref, S, c, slice(s, s + 1))
            K = len(np.unique(S[s]))
            assert np.array_equal(one["maps"][0, :K], ref["maps"][s, :K]) and one["maps"].shape[1] == K


def test_labels_and_maps_may_be_left_out():
    S, c, ref = problem("planted-cut40")
    got = _lib.relabel(S, c, want_labels=False, want_maps=False)
    assert got["labels"] is None and got["maps"] is None
    assert np.array_equal(got["overlap"], ref["overlap"]) and np.array_equal(got["counts"], ref["counts"])


def raw_call(S, c, m=None, n=None, Kp=None, width=None, device=0, null=()):
    """rc_relabel through ctypes with any argument overridden or NULL; returns the code"""
    lib = _lib.lib()
    S, c = np.ascontiguousarray(S, np.int64), np.ascontiguousarray(c, np.int64)
    m = S.shape[0] if m is None else m
    n = S.shape[1] if n is None else n
    Kp = len(np.unique(c)) if Kp is None else Kp
    W = max(len(np.unique(z)) for z in S) if width is None else width
    bufs = dict(samples=S, pivot=c, labels=np.zeros(S.shape, np.int64), maps=np.zeros((S.shape[0], max(W, 1)), np.int64),
                overlap=np.zeros(S.shape[0], np.int64), counts=np.zeros((S.shape[1], Kp + 1), np.uint32))
    ptr = {k: None if k in null else v.ctypes.data for k, v in bufs.items()}
    ms = C_.c_double(-1.0)
    return lib.rc_relabel(device, ptr["samples"], m, n, ptr["pivot"], Kp, ptr["labels"], ptr["maps"], W, ptr["overlap"], ptr["counts"],
                          None if "kernel_ms" in null else C_.byref(ms))


def last_error():
    return _lib.lib().rc_last_error(None).decode()


def test_argument_and_capacity_errors():
    S, c = np.array([[1, 1, 2, 3], [2, 2, 2, 4]], np.int64), np.array([1, 2, 2, 4], np.int64)
    assert raw_call(S, c) == 0
    assert raw_call(S, c, null=("labels", "maps", "kernel_ms")) == 0
    for req in ("samples", "pivot", "overlap", "counts"):
        assert raw_call(S, c, null=(req,)) == -1 and "NULL" in last_error(), req
    assert raw_call(S, c, m=0) == -1 and raw_call(S, c, n=0) == -1
    for bad in (0, 5):
        T = S.copy(); T[1, 2] = bad
        assert raw_call(T, c) == -1 and "sample 2 at position 3" in last_error(), last_error()
        d = c.copy(); d[3] = bad
        assert raw_call(S, d, Kp=3) == -1 and "pivot 1 at position 4" in last_error(), last_error()
    assert raw_call(S, c, Kp=2) == -1 and "3 clusters" in last_error()
    assert raw_call(S, c, width=2) == -1 and "maps" in last_error()
    assert raw_call(S, c, device=99) == -1 and "device" in last_error()
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_ARG"):
        _lib.relabel(np.array([[1, 9, 1]]), np.array([1, 1, 1]))
    # capacity, before any device work (device 99 does not exist: the capacity error comes first)
    big = np.ones((1, 32768), np.int64)
    assert raw_call(big, big[0], device=99) == -6 and "32768" in last_error()
    wide = np.arange(1, 1026, dtype=np.int64)
    assert raw_call(np.ones((1, 1025), np.int64), wide, device=99) == -6 and "pivot has 1025" in last_error()
    assert raw_call(np.stack([np.ones(1025, np.int64), wide]), np.ones(1025, np.int64), device=99) == -6 and "sample 2 has 1025" in last_error()
    with pytest.raises(rc.RedClustHIPError, match="RC_ERR_CAPACITY"):
        _lib.relabel(big, big[0])


def test_relabel_through_the_public_surface():
    S, c, ref = problem("planted-spread")
    rel = rc.relabel(S, c)
    assert isinstance(rel, rc.Relabelling)
    for key in ("labels", "maps", "overlap", "counts", "pivot_labels"):
        assert np.array_equal(getattr(rel, key), ref[key]), key
    m, n = S.shape
    pr = rel.probabilities()
    assert pr.shape == (n, len(ref["pivot_labels"]) + 1) and np.allclose(pr.sum(1), 1.0) and np.array_equal(pr, ref["counts"] / m)
    alloc = rel.allocation()
    assert np.array_equal(alloc, np.concatenate([[0], ref["pivot_labels"]])[np.argmax(ref["counts"], axis=1)])
    # the pivot is a sample: a 0.2 share of its own points is noise, which the modal allocation does not follow (0.81 ± 0.014 expected)
    assert 0.7 < np.mean(alloc == c) < 0.9
    assert np.array_equal(rel.uncertainty(), 1.0 - ref["counts"].max(1) / m)
    # anything with .clusts, and a list of label vectors
    import types
    again = rc.relabel(types.SimpleNamespace(clusts=[z for z in S]), list(c))
    assert np.array_equal(again.counts, rel.counts) and np.array_equal(again.labels, rel.labels)
    # a pivot whose names exceed n comes back under its own names
    far = c * 1000
    rel2 = rc.relabel(S, far)
    assert np.array_equal(rel2.pivot_labels, ref["pivot_labels"] * 1000) and np.array_equal(rel2.labels, ref["labels"] * 1000)
    assert np.array_equal(rel2.maps, np.where(ref["maps"] > 0, ref["maps"] * 1000, ref["maps"])) and np.array_equal(rel2.counts, ref["counts"])


def test_prediction_allocation_end_to_end():
    """The planted hold-out of test_gpu_predict (three tight groups, 30 held-out points and one far point), under four samples
    that name and cut the same clusters differently: every held-out point goes to its group's cluster of the pivot in most
    samples, whatever the samples call it."""
    h = P.holdout_case()
    lab = h["samples"][0]
    renamed = np.array([0, 50, 7, 99])[lab]
    split = lab.copy(); split[np.flatnonzero(lab == 1)[::2]] = 100   # cluster 1 cut in two
    S = np.stack([lab, renamed, split, np.array([0, 3, 1, 2])[lab]]).astype(np.int64)
    pred = rc.predict(S, new_points=h["new_points"], points=h["points"], r=np.array([1.5, 2.0, 1.5, 2.0]), p=np.array([0.3, 0.5, 0.3, 0.5]),
                      params=h["P"])
    rel = rc.relabel(S, lab)
    assert np.array_equal(rel.pivot_labels, [1, 2, 3]) and np.array_equal(rel.overlap[[0, 1, 3]], [120] * 3)
    A = pred.allocation(rel, S)
    print(A)
    assert A.shape == (31, 4) and np.allclose(A.sum(1), 1.0) and np.all(A >= 0)
    truth = h["truth_new"]
    assert np.all(A[np.arange(30), truth] > 0.5)
    with pytest.raises(ValueError, match="4 samples"):
        pred.allocation(rel, S[:3])
