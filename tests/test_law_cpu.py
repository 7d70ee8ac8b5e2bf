"""The oracle and the restatements against the exact law of each step (DESIGN.md "Testing the draws"); no GPU.

Every parity test holds the device against tests/oracle_lib.py, tests/np_transcription.py, tests/kmeans_ref.py or
tests/kmedoids_ref.py on the same Philox stream.  These tests hold those restatements' draws against probabilities computed
without any stream (tests/law_ref.py): a design error the two sides share shows here.  Bounds: the upper 1e-6 quantile of
chi2(df); seeds are fixed, so every test is deterministic."""
import numpy as np
import pytest

import kmeans_ref as KM
import kmedoids_ref as KD
import law_ref as LR
import oracle_lib as O

N_RESTART = 20000
N_TWO = 30000            # the composed law is more spread out: at 20 000 its unpooled cells hold 89 %, short of the 90 % asked
N_CHAIN = 100000
N_SM = 20000
N_SM_POWER = 200000
N_SEED = 20000

STREAMS = LR.streams()


@pytest.mark.parametrize("n", [5, 6])
def test_oracle_scores_give_the_same_law(n):
    """the tree built from Oracle.point_scores_stable against the transcription's, to 1e-12"""
    D, start = LR.small_case(n)
    orc = LR.small_oracle(n)
    orc.set_state(start)
    a = LR.law_cache(n)(start)
    b = LR.sweep_law(D, LR.PARAMS, start, LR.R0, LR.P0, scores=LR.oracle_scores(orc, LR.R0, LR.P0))
    assert set(a) == set(b) and len(a) == {5: 508, 6: 2617}[n]
    worst = max(abs(a[k] - b[k]) for k in a)
    print(f"LAW agreement n={n}: {worst:.3g}")
    assert worst <= 1e-12


@pytest.mark.parametrize("stream", STREAMS, ids=[s[2] for s in STREAMS])
@pytest.mark.parametrize("n", [5, 6])
def test_sweep_restart(n, stream):
    seed, index, name = stream
    start = LR.small_case(n)[1]
    counts = LR.oracle_restart_counts(n, seed, index, N_RESTART)
    LR.assert_consistent(f"cpu sweep restart n={n} {name}", counts, LR.law_cache(n)(start), N_RESTART)


@pytest.mark.parametrize("seed", LR.SEEDS, ids=hex)
def test_sweep_chain(seed):
    """free-running chain, every row of at least 200 visits against that state's exact law — and the same counts against
    three slightly wrong laws, which must be rejected at the same bound"""
    trans = LR.transitions(LR.oracle_chain_path(seed, N_CHAIN))
    stat, df, share = LR.chi2_transitions(trans, LR.law_cache(6))
    LR.report(f"cpu sweep chain n=6 {seed:#x}", stat, df, N=N_CHAIN, share=share, rows=len(LR.law_cache(6).laws))
    assert share >= 0.9
    assert stat <= LR.bound(df)
    for which in LR.PERTURBED:
        s2, d2, _ = LR.chi2_transitions(trans, LR.law_cache(6, which))
        LR.report(f"cpu sweep chain n=6 {seed:#x} against {which}", s2, d2)
        assert s2 > LR.bound(d2), which


@pytest.mark.parametrize("seed", LR.SEEDS, ids=hex)
def test_two_consecutive_sweeps(seed):
    """sweeps 2k and 2k + 1 from the start, against the composed law: correlation between sweep t and t + 1 shows here"""
    D, start = LR.small_case(5)
    orc = LR.small_oracle(5)

    def two(seed, k):
        orc.set_state(start)
        orc.sweep_stable(LR.R0, LR.P0, seed, 2 * k)
        orc.sweep_stable(LR.R0, LR.P0, seed, 2 * k + 1)
        return orc.clusts
    LR.assert_consistent(f"cpu two sweeps n=5 {seed:#x}", LR.restart_counts(two, seed, int, N_TWO), LR.small_law2(5), N_TWO)


@pytest.mark.parametrize("seed", LR.SEEDS[:2], ids=hex)
@pytest.mark.parametrize("state", list(LR.SM_STATES))
def test_splitmerge_proposal(state, seed):
    """(accept, split, labels afterwards) of Oracle.mh_proposal against the enumerated law: the state it leaves ("intended"),
    and the flags alone with the caller's labels untouched ("as_written", quirk Q1)"""
    outs = LR.oracle_proposals(state, seed, N_SM)
    law = LR.sm_law(state)
    assert abs(sum(q for k, q in law.items() if k[1]) - {"merge": 0.2, "split": 1.0}[state]) < 1e-12   # pairs within a cluster
    LR.assert_consistent(f"cpu splitmerge {state} intended {seed:#x}", LR.count(outs), law, N_SM)
    before = LR.SM_STATES[state]
    LR.assert_consistent(f"cpu splitmerge {state} as_written {seed:#x}", LR.count((a, s, before) for a, s, _ in outs),
                         LR.sm_law(state, "as_written"), N_SM)


def test_splitmerge_power():
    """the split state's counts against the law at r·1.1 — rejected at N_SM_POWER proposals (DESIGN.md gives the measured p)"""
    outs = LR.oracle_proposals("split", LR.SEEDS[0], N_SM_POWER)
    LR.assert_consistent("cpu splitmerge split intended, power run", LR.count(outs), LR.sm_law("split"), N_SM_POWER)
    LR.assert_rejected("cpu splitmerge split against r*1.1", LR.count(outs), LR.sm_law("split", r=LR.R0 * 1.1), N_SM_POWER)


SEED_CASES = [("plain", 2), ("plain", 3), ("coincident", 3), ("close", 3)]


@pytest.mark.parametrize("case,k", SEED_CASES)
def test_kmeanspp_seeds(case, k):
    X = LR.seeding_points(case)
    law = LR.kmeanspp_law(X, k)
    if case != "plain":
        assert all(not (2 in key and 5 in key) for key in law)          # the zero weight: never both of the pair
    counts = LR.seeding_counts(lambda s: KM.kmpp_seeds(X, k, s), N_SEED)
    LR.assert_consistent(f"cpu kmeans++ {case} k={k}", counts, law, 2 * N_SEED)
    if (case, k) == ("plain", 3):
        LR.assert_rejected(f"cpu kmeans++ {case} k={k} against weight 0 x 1.1", counts, LR.kmeanspp_law(X, k, tilt=(0, 1.1)),
                           2 * N_SEED)


@pytest.mark.parametrize("case,k", SEED_CASES)
def test_kmedoidspp_seeds(case, k):
    Dq = O.Oracle(LR.distances(LR.seeding_points(case)), LR.PARAMS).Dq
    law = LR.kmedoidspp_law(Dq, k)
    counts = LR.seeding_counts(lambda s: KD.kmpp_seeds(Dq, k, s), N_SEED)
    LR.assert_consistent(f"cpu kmedoids++ {case} k={k}", counts, law, 2 * N_SEED)
    if (case, k) == ("plain", 3):
        LR.assert_rejected(f"cpu kmedoids++ {case} k={k} against weight 0 x 1.1", counts, LR.kmedoidspp_law(Dq, k, tilt=(0, 1.1)),
                           2 * N_SEED)


@pytest.mark.parametrize("n,nsweeps", [(135, 300), (1029, 40)])
def test_calibration_of_the_oracle_chain(n, nsweeps):
    """the larger cases of tests/test_gpu_law.py, shorter: the oracle's own chain replayed visit by visit — both martingale
    sums within 4.9 sd, and the cases as undecided as they are meant to be (median p_top below 0.9)"""
    D, P, start = LR.large_case(n)
    path = LR.device_path(LR.oracle_chain(O.Oracle(D, P), start, LR.LARGE_R, LR.LARGE_P), start, LR.LARGE_R, LR.LARGE_P,
                          LR.SEEDS[1], nsweeps)
    res = LR.calibration(path, O.Oracle(D, P))
    print(f"LAW cpu calibration n={n} sweeps={nsweeps}: {res}")
    assert res["median_p_top"] < 0.9
    assert abs(res["z_top"]) <= LR.Z_BOUND and abs(res["z_new"]) <= LR.Z_BOUND
