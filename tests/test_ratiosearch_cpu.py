"""The ratio-loss search without a GPU: the NumPy restatement the device is held to (tests/ratio_search_ref.py) against a direct
evaluation, the integer criterion against exact rationals (omARI) and against the f64 evaluators (NVI, NID), and the ABI
declarations of rc_ratio_search."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import psm_search_ref as R
import ratio_search_ref as Q
import vi_search_ref as V
import redclust_amd as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 14, 9


def _samples():
    S, _ = R.planted_counts(N, M, 3, 0.3, seed=4)
    S[1], S[2] = np.arange(1, N + 1), 1                              # all singletons; one cluster: den = 0 where c equals them
    return S


@pytest.mark.parametrize("loss", Q.LOSSES)
@pytest.mark.parametrize("init_kind", ["empty", "ones", "singletons", "mixed"])
def test_reference_keeps_the_criterion_it_returns(init_kind, loss):
    S, G = _samples(), V.numpy_G(N)
    rng = np.random.default_rng(5)
    init = {"empty": np.zeros(N, np.int64), "ones": np.ones(N, np.int64), "singletons": np.arange(1, N + 1),
            "mixed": np.where(np.arange(N) % 2 == 0, 0, rng.integers(1, 3, N))}[init_kind]
    r = Q.ratio_search_ref(S, G, loss, init, rng.permutation(N) + 1)
    assert r["converged"] and r["loss_num"] == Q.q_direct(r["labels"], S, G, loss)
    assert V.best_single_move_gain(r["labels"], S, G, q=lambda c, s, g: Q.q_direct(c, s, g, loss)) <= 0
    # the trivial partitions against themselves (samples 2 and 1): num = 0; den = 0 too, except the entropic den of singletons, Φ(n)
    for c, own in ((np.ones(N, np.int64), 2), (np.arange(1, N + 1), 1)):
        num, den = Q.num_den(*Q.sample_states(c, S, G, loss), loss)
        assert num[own] == 0 and np.flatnonzero(den == 0).tolist() == ([own] if own == 2 or loss == "omARI" else [])


def _one_minus_ari(c, s):
    """exact: C(P + Q − 2X) / (C(P + Q) − 2PQ) over the pairs, 0 where the denominator is"""
    n = len(c)
    iu = np.triu_indices(n, 1)
    a, b = (c[:, None] == c[None, :])[iu], (s[:, None] == s[None, :])[iu]
    P, Qs, X, C = int(a.sum()), int(b.sum()), int((a & b).sum()), n * (n - 1) // 2
    den = C * (P + Qs) - 2 * P * Qs
    return Fraction(C * (P + Qs - 2 * X), den) if den else Fraction(0)


def test_omari_criterion_is_the_exact_mean_to_two_to_the_minus_40():
    """a term is rint(fl(ratio)·2^40): within 2^-41 of ratio·(1 + 2^-53), ratio <= 2 — 2^-40 covers both"""
    S, G = _samples(), V.numpy_G(N)
    rng = np.random.default_rng(6)
    for c in (S[0], S[1], S[2], rng.integers(1, 5, N)):
        exact = sum(_one_minus_ari(c, s) for s in S) / M
        assert abs(Fraction(Q.q_direct(c, S, G, "omARI"), 2 ** 40 * M) - exact) <= Fraction(1, 2 ** 40)
        assert abs(rc.expectedomari(c, S) - float(exact)) <= 1e-14


@pytest.mark.parametrize("loss", ["NVI", "NID"])
def test_entropic_criteria_are_the_f64_evaluators_to_the_tables_rounding(loss):
    """DESIGN.md §8 "Ratio-loss search": Φq(x) is within x/2 units of 2^-32, so A, B_s, T_s and C are each within n/2 units; num is
    then within e_num = 2n (NVI: A + B − 2T) or n (NID) units and den within e_den = n, and for a true ratio <= 1 the quotient moves
    by at most (e_num + e_den) / den_q.  Plus 2^-41 for the term's rounding and 1e-12 for the f64 sums of the evaluator."""
    S, G = _samples(), V.numpy_G(N)
    evaluate = {"NVI": rc.expectednvi, "NID": rc.expectednid}[loss]
    rng = np.random.default_rng(7)
    for c in (S[0], S[1], S[2], rng.integers(1, 5, N)):
        _, den = Q.num_den(*Q.sample_states(c, S, G, loss), loss)
        bound = float(np.mean(np.where(den > 0, ((2 if loss == "NVI" else 1) * N + N) / np.maximum(den, 1), 0.0))) + 2.0 ** -41 + 1e-12
        err = abs(Q.q_direct(c, S, G, loss) / (2.0 ** 40 * M) - evaluate(c, S))
        print(loss, "err", err, "bound", bound)
        assert err <= bound


def test_header_signatures_and_julia_agree_on_rc_ratio_search():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "redclust_hip.h")).read(), flags=re.S)
    protos = {name: re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1) for name in ("rc_vi_search", "rc_ratio_search")}
    nargs = {k: len([a for a in v.split(",") if a.strip()]) for k, v in protos.items()}
    assert nargs["rc_ratio_search"] == nargs["rc_vi_search"] + 1 == len(rc.SIGNATURES["rc_ratio_search"][1])
    assert re.sub(r"\s+", " ", protos["rc_ratio_search"]).replace("int64_t n, int32_t loss,", "int64_t n,") == re.sub(r"\s+", " ", protos["rc_vi_search"])
    for name, code in rc._lib.RATIO_LOSSES.items():
        assert re.search(r"#define RC_RATIO_%s %d\b" % (name.upper(), code), hdr)
    assert "ccall((:rc_ratio_search, LIB)" in open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    import test_oracle_cpu
    test_oracle_cpu.test_julia_glue_ccalls_match_the_header()
    with pytest.raises(ValueError, match="omARI"):
        rc.searchratio(_samples(), "VI")


def test_capacity_and_loss_errors_come_before_the_samples_are_read():
    import ctypes as C_
    L = rc.lib()
    buf = np.ones(8, np.int64)
    order = np.arange(1, 9, dtype=np.int32)
    runs, best = (rc._lib.RcPsmRun * 1)(), C_.c_int32()

    def call(m, n, loss=0):
        code = L.rc_ratio_search(0, buf.ctypes.data, m, n, loss, 1, buf.ctypes.data, order.ctypes.data, 0, 5, buf.ctypes.data, runs, C_.byref(best), None)
        return code, L.rc_last_error(None).decode()

    for (m, n, loss), (code, word) in {(1, 8, 3): (-1, "RC_RATIO_OMARI"), (1, 8193, 0): (-6, "8192"), (2 ** 26 // 64 + 1, 64, 1): (-6, "2^26"),
                                       (2 ** 21 + 1, 8, 2): (-6, "2^21")}.items():
        got, msg = call(m, n, loss)
        assert got == code and msg.startswith("rc_ratio_search") and word in msg, (m, n, loss, got, msg)
