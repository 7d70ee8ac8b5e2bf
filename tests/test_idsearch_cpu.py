"""The exact expected-ID search without a GPU: the criterion (expectedid) against a direct entropy formula, the properties of
the NumPy restatement the device is held to (tests/id_search_ref.py), the ABI declarations and the argument errors of
searchpointestimate(loss="ID") that need no device."""
import os
import re

import numpy as np
import pytest

import psm_search_ref as R
import vi_search_ref as V
import id_search_ref as I
import redclust_amd as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Samples:
    def __init__(self, clusts):
        self.clusts = list(clusts)


def _entropies(a, b):
    """(H(a), H(b), H(a, b)) from the empirical distributions, natural logs"""
    n = len(a)
    ia = np.unique(a, return_inverse=True)[1]
    ib = np.unique(b, return_inverse=True)[1]
    P = np.zeros((ia.max() + 1, ib.max() + 1))
    np.add.at(P, (ia, ib), 1.0 / n)
    H = lambda p: -float(np.sum(p[p > 0] * np.log(p[p > 0])))
    return H(P.sum(axis=1)), H(P.sum(axis=0)), H(P.ravel())


def _id_direct(a, b):
    """infodist(a, b; normalised = false) = max(H(a), H(b)) − I(a; b), I = H(a) + H(b) − H(a, b)"""
    ha, hb, hab = _entropies(a, b)
    return max(ha, hb) - (ha + hb - hab)


def test_expectedid_is_the_mean_information_distance():
    n, m = 65, 7
    S, _ = R.planted_counts(n, m, 5, 0.2, seed=1)
    rng = np.random.default_rng(2)
    for c in (S[0], S[3], rng.integers(1, 9, n), np.ones(n, np.int64), np.arange(1, n + 1)):
        ref = np.mean([_id_direct(c, S[s]) for s in range(m)])
        assert abs(rc.expectedid(c, S) - ref) <= 1e-12
        assert abs(rc.expectedid(c, _Samples(S)) - ref) <= 1e-12
    assert abs(rc.expectedid(S[2], S[2:3])) <= 1e-12               # ID(c, c) = 0
    assert abs(rc.expectedid(S[2], [S[2]])) <= 1e-12
    with pytest.raises(ValueError):
        rc.expectedid(S[0][:-1], S)
    with pytest.raises(ValueError):
        rc.expectedid(S[0], [])


def test_expectedid_of_one_sample_is_the_joint_entropy_minus_the_smaller():
    n = 40
    rng = np.random.default_rng(3)
    for K, L in ((2, 7), (7, 2), (5, 5), (1, 4)):
        c, s = rng.integers(1, K + 1, n), rng.integers(1, L + 1, n)
        hc, hs, hcs = _entropies(c, s)
        assert abs(rc.expectedid(c, [s]) - (hcs - min(hc, hs))) <= 1e-12


def test_sorted_table_evaluates_F():
    """F(x) = x·p(x) + Pre[m] − Pre[p(x)] is Σ_s max(x, B_s), also where x meets a B_s and where every B_s is the same"""
    rng = np.random.default_rng(4)
    for B in ([int(b) for b in rng.integers(0, 2 ** 48, 9)], [5, 5, 5, 5], [7]):
        Bs, Pre = I.sorted_table(B)
        for x in [0, 1, min(B) - 1, min(B), max(B), max(B) + 1, 2 ** 49] + B + [b + 1 for b in B]:
            assert I.F_sorted(x, Bs, Pre) == I.F(x, B)


@pytest.mark.parametrize("init_kind", ["empty", "ones", "mixed"])
@pytest.mark.parametrize("maxK", [0, 2])
def test_reference_runs_converge_to_a_local_optimum(init_kind, maxK):
    n, m = 12, 9
    S, _ = R.planted_counts(n, m, 3, 0.3, seed=4)
    G = V.numpy_G(n)
    rng = np.random.default_rng(5)
    init = {"empty": np.zeros(n, np.int64), "ones": np.ones(n, np.int64),
            "mixed": np.where(np.arange(n) % 2 == 0, 0, rng.integers(1, 3, n))}[init_kind]
    r = I.id_search_ref(S, G, init, rng.permutation(n) + 1, maxK=maxK)
    assert r["converged"] and r["sweeps"] <= 100
    assert r["loss_num"] == I.q_direct(r["labels"], S, G)                              # the tables and the A it kept are right
    assert r["K"] == len(np.unique(r["labels"])) and (maxK == 0 or r["K"] <= maxK)
    assert I.best_single_move_gain(r["labels"], S, G, maxK=maxK) <= 0                  # no improving single move
    # Q_ID is n·m·2^32·E[ID] up to the table's rounding (one unit per point and sample)
    assert abs(r["loss_num"] / (2.0 ** 32 * n * m) - rc.expectedid(r["labels"], S)) <= 2.0 ** -32 + 1e-12


def test_one_sweep_and_the_compaction_of_the_start():
    n, m = 12, 9
    S, _ = R.planted_counts(n, m, 4, 0.3, seed=7)
    G = V.numpy_G(n)
    u = I.id_search_ref(S, G, np.zeros(n, np.int64), np.arange(1, n + 1), maxsweeps=1)
    assert not u["converged"] and u["sweeps"] == 1 and u["moves"] == n
    a = I.id_search_ref(S, G, np.array([7, 7, 0, 3, 3, 3, 0, 12, 12, 7, 3, 0]), np.arange(1, n + 1))
    b = I.id_search_ref(S, G, np.array([1, 1, 0, 2, 2, 2, 0, 3, 3, 1, 2, 0]), np.arange(1, n + 1))
    assert np.array_equal(a["raw"], b["raw"]) and a["loss_num"] == b["loss_num"]


def _partitions(n):
    """all set partitions of n points as restricted-growth label vectors (203 for n = 6)"""
    def rec(prefix, k):
        if len(prefix) == n:
            yield prefix
            return
        for l in range(1, k + 2):
            yield from rec(prefix + [l], max(k, l))
    return [np.array(p, np.int64) for p in rec([], 0)]


def test_a_run_started_at_the_optimum_does_not_move():
    n, m = 6, 5
    S, _ = R.planted_counts(n, m, 2, 0.25, seed=6)
    G = V.numpy_G(n)
    parts = _partitions(n)
    assert len(parts) == 203
    opt = parts[int(np.argmin([I.q_direct(p, S, G) for p in parts]))]
    # the integer criterion and the f64 one agree on the optimum's value (to the table's rounding)
    assert abs(I.q_direct(opt, S, G) / (2.0 ** 32 * n * m) - min(rc.expectedid(p, S) for p in parts)) <= 2.0 ** -32 + 1e-12
    r = I.id_search_ref(S, G, opt, np.arange(1, n + 1), maxK=n)
    assert r["converged"] and r["sweeps"] == 1 and r["moves"] == 0 and np.array_equal(r["labels"], R.sortlabels(opt))


def _nargs(proto):
    return len([a for a in proto.split(",") if a.strip()])


def test_header_and_signatures_agree_on_rc_id_search():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "redclust_hip.h")).read(), flags=re.S)
    protos = {}
    for name in ("rc_vi_search", "rc_id_search"):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        protos[name] = re.sub(r"\s+", " ", m.group(1)).strip()
        assert name in rc.SIGNATURES and _nargs(m.group(1)) == len(rc.SIGNATURES[name][1]), name
    assert protos["rc_id_search"] == protos["rc_vi_search"]                            # exactly rc_vi_search's parameter list
    assert rc.SIGNATURES["rc_id_search"] == rc.SIGNATURES["rc_vi_search"]
    assert not re.search(r"#define RC_PSM_\w+ 2\b", hdr)                               # no loss code was added
    assert callable(rc._lib.id_search) and "expectedid" in dir(rc)


def test_julia_wrapper_calls_the_id_search():
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    assert "ccall((:rc_id_search, LIB)" in jl
    import test_oracle_cpu
    test_oracle_cpu.test_julia_glue_ccalls_match_the_header()


def test_argument_errors_that_need_no_device():
    S, C = R.planted_counts(8, 3, 2, 0.2, seed=1)
    for exact in (False, True):
        with pytest.raises(ValueError, match="count matrix"):
            rc.searchpointestimate(C, "ID", numsamples=3, exact=exact)
        with pytest.raises(ValueError, match="Context"):
            rc.searchpointestimate(None, "ID", numsamples=3, ctx=object(), exact=exact)
        with pytest.raises(ValueError):
            rc.searchpointestimate(None, "ID", exact=exact)
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.searchpointestimate(_Samples(S), "omARI")
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.searchpointestimate(C, "omARI", numsamples=3)
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.expectedloss(S[0], C, 3, "ID")                                              # expectedloss stays as it is
