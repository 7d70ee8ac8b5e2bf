"""The point-estimate search without a GPU: the criterion (expectedloss) against the reference's pairwise losses, the
properties of the NumPy restatement the device is held to (tests/psm_search_ref.py), the ABI declarations and the
argument errors of searchpointestimate that need no device."""
import os
import re

import numpy as np
import pytest

import np_transcription as T
import psm_search_ref as R
import redclust_amd as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binder_expectedloss_is_the_mean_pairwise_binder_loss():
    n, m = 65, 7
    S, C = R.planted_counts(n, m, 5, 0.2, seed=1)
    pairs = n * (n - 1) // 2
    rng = np.random.default_rng(2)
    for c in (S[0], S[3], rng.integers(1, 9, n), np.ones(n, np.int64), np.arange(1, n + 1)):
        num = R.binder_num(c, C, m)
        ref = sum(int(round(T.binderloss(c, S[s], normalised=False))) for s in range(m))
        assert num == ref
        got = rc.expectedloss(c, C, m, "binder")
        assert got == num / (m * pairs)
        mean = np.mean([T.binderloss(c, S[s]) for s in range(m)])
        assert abs(got - mean) <= 1e-12 * abs(mean)


def test_vi_expectedloss_against_the_direct_evaluation():
    n, m = 65, 7
    S, C = R.planted_counts(n, m, 5, 0.2, seed=1)
    rng = np.random.default_rng(3)
    for c in (S[0], rng.integers(1, 9, n), np.ones(n, np.int64), np.arange(1, n + 1)):
        f = 0.0
        for i in range(n):                                          # §1 of the design, term by term
            mem = [j for j in range(n) if c[j] == c[i]]
            f += np.log(len(mem)) - 2.0 * np.log(sum(int(C[i, j]) for j in mem))
        assert abs(rc.expectedloss(c, C, m, "VI") - (f / n + 2.0 * np.log(m))) <= 1e-12
    # all singletons: T_i = m, every term cancels
    assert abs(rc.expectedloss(np.arange(1, n + 1), C, m, "VI")) <= 1e-12


def test_expectedloss_accepts_only_the_two_losses():
    C = np.full((2, 2), 3, np.uint32)
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.expectedloss([1, 1], C, 3, "omARI")
    assert rc.expectedloss([1], np.full((1, 1), 3, np.uint32), 3, "binder") == 0.0


@pytest.mark.parametrize("init_kind", ["empty", "ones", "mixed"])
def test_reference_binder_runs_converge_to_a_local_optimum(init_kind):
    n, m = 12, 9
    _, C = R.planted_counts(n, m, 3, 0.3, seed=4)
    rng = np.random.default_rng(5)
    init = {"empty": np.zeros(n, np.int64), "ones": np.ones(n, np.int64),
            "mixed": np.where(np.arange(n) % 2 == 0, 0, rng.integers(1, 4, n))}[init_kind]
    r = R.psm_search_ref(C, m, R.BINDER, init, rng.permutation(n) + 1)
    assert r["converged"] and r["sweeps"] <= 100
    assert R.best_single_move_gain(r["labels"], C, m, R.BINDER) <= 0
    assert r["loss_num"] == R.binder_num(r["labels"], C, m) and r["K"] == len(np.unique(r["labels"]))
    v = R.psm_search_ref(C, m, R.VILB, init, rng.permutation(n) + 1)
    assert v["converged"] and R.best_single_move_gain(v["labels"], C, m, R.VILB) <= 1e-12
    assert abs(R.vi_best_move_gain(v["labels"], C, m) - max(R.best_single_move_gain(v["labels"], C, m, R.VILB), 0.0)) <= 1e-12


def _partitions(n):
    """all set partitions of n points as restricted-growth label vectors (203 for n = 6)"""
    def rec(prefix, k):
        if len(prefix) == n:
            yield prefix
            return
        for l in range(1, k + 2):
            yield from rec(prefix + [l], max(k, l))
    return [np.array(p, np.int64) for p in rec([], 0)]


@pytest.mark.parametrize("loss", [R.BINDER, R.VILB])
def test_a_run_started_at_the_optimum_does_not_move(loss):
    n, m = 6, 5
    _, C = R.planted_counts(n, m, 2, 0.25, seed=6)
    parts = _partitions(n)
    assert len(parts) == 203
    vals = [R.binder_num(p, C, m) if loss == R.BINDER else R.vi_f(p, C) for p in parts]
    opt = parts[int(np.argmin(vals))]
    r = R.psm_search_ref(C, m, loss, opt, np.arange(1, n + 1))
    assert r["converged"] and r["sweeps"] == 1 and r["moves"] == 0 and np.array_equal(r["labels"], R.sortlabels(opt))


def test_maxk_caps_the_reference_run():
    n, m = 12, 9
    _, C = R.planted_counts(n, m, 4, 0.3, seed=7)
    r = R.psm_search_ref(C, m, R.BINDER, np.zeros(n, np.int64), np.arange(1, n + 1), maxK=2)
    assert r["K"] <= 2 and r["converged"]
    u = R.psm_search_ref(C, m, R.BINDER, np.zeros(n, np.int64), np.arange(1, n + 1), maxsweeps=1)
    assert not u["converged"] and u["sweeps"] == 1 and u["moves"] == n


def _nargs(proto):
    return len([a for a in proto.split(",") if a.strip()])


def test_header_and_signatures_agree_on_the_new_entries():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "redclust_hip.h")).read(), flags=re.S)
    for name in ("rc_psm_search", "rc_psm_search_ctx"):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert name in rc.SIGNATURES and _nargs(m.group(1)) == len(rc.SIGNATURES[name][1]), name
    assert re.search(r"#define RC_PSM_BINDER 0\b", hdr) and re.search(r"#define RC_PSM_VILB 1\b", hdr)
    from redclust_amd import _lib
    import ctypes
    assert ctypes.sizeof(_lib.RcPsmRun) == 40 and [f[0] for f in _lib.RcPsmRun._fields_] == ["loss", "loss_num", "sweeps", "converged", "moves", "K"]


def test_julia_wrapper_calls_the_search():
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    assert re.search(r"function searchpointestimate\(b::HIPBackend, result;", jl)
    assert "ccall((:rc_psm_search, LIB)" in jl
    import test_oracle_cpu
    test_oracle_cpu.test_julia_glue_ccalls_match_the_header()


def test_argument_errors_that_need_no_device():
    C = np.full((3, 3), 2, np.uint32)
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.searchpointestimate(C, "omARI", numsamples=2)
    with pytest.raises(ValueError, match="numsamples"):
        rc.searchpointestimate(C, "binder")
    with pytest.raises(ValueError, match="square"):
        rc.searchpointestimate(np.zeros((2, 3), np.uint32), "binder", numsamples=2)
    with pytest.raises(ValueError, match="n entries"):
        rc.searchpointestimate(C, "binder", numsamples=2, init=[[1, 1]])
    with pytest.raises(ValueError):
        rc.searchpointestimate(None, "VI")
