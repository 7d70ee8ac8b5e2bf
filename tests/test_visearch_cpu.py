"""The exact expected-VI search without a GPU: the criterion (expectedvi) against a direct entropy formula, the properties
of the NumPy restatement the device is held to (tests/vi_search_ref.py), the fixed-point table, the ABI declarations and
the argument errors of searchpointestimate(exact=True) that need no device."""
import os
import re

import numpy as np
import pytest

import psm_search_ref as R
import vi_search_ref as V
import redclust_amd as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Samples:
    def __init__(self, clusts):
        self.clusts = list(clusts)


def _vi_direct(a, b):
    """VI(a, b) = H(a) + H(b) − 2·I(a; b) from the joint distribution, natural logs"""
    n = len(a)
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    P = np.zeros((len(ua), len(ub)))
    np.add.at(P, (ia, ib), 1.0 / n)
    pa, pb = P.sum(axis=1), P.sum(axis=0)
    H = lambda p: -float(np.sum(p[p > 0] * np.log(p[p > 0])))
    nz = P > 0
    I = float(np.sum(P[nz] * np.log(P[nz] / np.outer(pa, pb)[nz])))
    return H(pa) + H(pb) - 2.0 * I


def test_expectedvi_is_the_mean_variation_of_information():
    n, m = 65, 7
    S, _ = R.planted_counts(n, m, 5, 0.2, seed=1)
    rng = np.random.default_rng(2)
    for c in (S[0], S[3], rng.integers(1, 9, n), np.ones(n, np.int64), np.arange(1, n + 1)):
        ref = np.mean([_vi_direct(c, S[s]) for s in range(m)])
        assert abs(rc.expectedvi(c, S) - ref) <= 1e-12
        assert abs(rc.expectedvi(c, _Samples(S)) - ref) <= 1e-12
    assert abs(rc.expectedvi(S[2], S[2:3])) <= 1e-12               # VI(c, c) = 0
    with pytest.raises(ValueError):
        rc.expectedvi(S[0][:-1], S)


def test_numpy_table_is_positive_and_increasing():
    G = V.numpy_G(8192)
    assert "rc_vi_gtable" in rc.SIGNATURES                         # the library's table is held to this one on the GPU
    assert G[0] == 0 and len(G) == 8192
    assert (G[1:] > 0).all() and (np.diff(G) > 0).all()
    # G is φ(x+1) − φ(x) in units of 2^-32: the prefix sums are φ to within half a unit per entry
    Phi = V.phi_table(G)
    for x in (1, 2, 3, 100, 8192):
        assert abs(Phi[x] - x * np.log(x) * 2.0 ** 32) <= 0.5 * x + 1e-3 * x


@pytest.mark.parametrize("init_kind", ["empty", "ones", "mixed"])
@pytest.mark.parametrize("maxK", [0, 2])
def test_reference_runs_converge_to_a_local_optimum(init_kind, maxK):
    n, m = 12, 9
    S, _ = R.planted_counts(n, m, 3, 0.3, seed=4)
    G = V.numpy_G(n)
    rng = np.random.default_rng(5)
    init = {"empty": np.zeros(n, np.int64), "ones": np.ones(n, np.int64),
            "mixed": np.where(np.arange(n) % 2 == 0, 0, rng.integers(1, 3, n))}[init_kind]
    r = V.vi_search_ref(S, G, init, rng.permutation(n) + 1, maxK=maxK)
    assert r["converged"] and r["sweeps"] <= 100
    assert r["loss_num"] == V.q_direct(r["labels"], S, G)                              # the tables it kept are right
    assert r["K"] == len(np.unique(r["labels"])) and (maxK == 0 or r["K"] <= maxK)
    assert V.best_single_move_gain(r["labels"], S, G, maxK=maxK) <= 0                  # no improving single move
    # Q + constant is n·m·2^32·E[VI] up to the table's rounding (2 units per point and sample)
    ev = (r["loss_num"] + V.constant(S, G)) / (2.0 ** 32 * n * m)
    assert abs(ev - rc.expectedvi(r["labels"], S)) <= 2.0 * 2.0 ** -32 + 1e-12


def test_one_sweep_and_the_compaction_of_the_start():
    n, m = 12, 9
    S, _ = R.planted_counts(n, m, 4, 0.3, seed=7)
    G = V.numpy_G(n)
    u = V.vi_search_ref(S, G, np.zeros(n, np.int64), np.arange(1, n + 1), maxsweeps=1)
    assert not u["converged"] and u["sweeps"] == 1 and u["moves"] == n
    a = V.vi_search_ref(S, G, np.array([7, 7, 0, 3, 3, 3, 0, 12, 12, 7, 3, 0]), np.arange(1, n + 1))
    b = V.vi_search_ref(S, G, np.array([1, 1, 0, 2, 2, 2, 0, 3, 3, 1, 2, 0]), np.arange(1, n + 1))
    assert np.array_equal(a["raw"], b["raw"]) and a["loss_num"] == b["loss_num"]
    # Q of the compacted run is the expected VI of its labelling, as the package evaluates it
    ev = (a["loss_num"] + V.constant(S, G)) / (2.0 ** 32 * n * m)
    assert abs(ev - rc.expectedvi(a["labels"], S)) <= 2.0 * 2.0 ** -32 + 1e-12


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
    parts = _partitions(n)
    assert len(parts) == 203
    opt = parts[int(np.argmin([rc.expectedvi(p, S) for p in parts]))]
    r = V.vi_search_ref(S, V.numpy_G(n), opt, np.arange(1, n + 1), maxK=n)
    assert r["converged"] and r["sweeps"] == 1 and r["moves"] == 0 and np.array_equal(r["labels"], R.sortlabels(opt))


def _nargs(proto):
    return len([a for a in proto.split(",") if a.strip()])


def test_header_and_signatures_agree_on_the_new_entries():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "redclust_hip.h")).read(), flags=re.S)
    for name in ("rc_vi_gtable", "rc_vi_search"):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert name in rc.SIGNATURES and _nargs(m.group(1)) == len(rc.SIGNATURES[name][1]), name
    # rc_psm_search keeps its two loss codes
    assert re.search(r"#define RC_PSM_BINDER 0\b", hdr) and re.search(r"#define RC_PSM_VILB 1\b", hdr)
    assert not re.search(r"#define RC_PSM_\w+ 2\b", hdr)


def test_julia_wrapper_calls_the_exact_search():
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    assert "ccall((:rc_vi_search, LIB)" in jl
    assert re.search(r"function searchpointestimate\(b::HIPBackend, result;[^)]*exact::Bool\s*=\s*false", jl, flags=re.S)
    import test_oracle_cpu
    test_oracle_cpu.test_julia_glue_ccalls_match_the_header()


def test_argument_errors_of_exact_that_need_no_device():
    S, C = R.planted_counts(8, 3, 2, 0.2, seed=1)
    with pytest.raises(ValueError, match="count matrix"):
        rc.searchpointestimate(C, "VI", numsamples=3, exact=True)
    with pytest.raises(ValueError, match="Context"):
        rc.searchpointestimate(None, "VI", numsamples=3, ctx=object(), exact=True)
    with pytest.raises(ValueError, match='loss="VI"'):
        rc.searchpointestimate(_Samples(S), "binder", exact=True)
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.searchpointestimate(_Samples(S), "omARI", exact=True)
    with pytest.raises(ValueError):
        rc.searchpointestimate(None, "VI", exact=True)
