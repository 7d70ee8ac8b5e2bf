"""The device's draws against the exact law of each step (-m gpu; DESIGN.md "Testing the draws").

The Gibbs sweep, one split–merge proposal and the seeding draws of k-means / k-medoids, each run many times on the device
and counted; the counts are held against probabilities computed from the transcription's scores alone (tests/law_ref.py),
at the upper 1e-6 quantile of chi2(df), and — draw by draw, or count by count — against what the oracle drew from the
same stream.  Every test is a plain loop of short calls on one context."""
import numpy as np
import pytest

import kmeans_ref as KM
import kmedoids_ref as KD
import law_ref as LR
import oracle_lib as O
import redclust_amd as rc

pytestmark = pytest.mark.gpu

N_RESTART = 20000
N_TWO = 30000            # the composed law is more spread out: at 20 000 its unpooled cells hold 89 %, short of the 90 % asked
N_CHAIN = 100000          # about 5 s on the device; the power assertion needs 100 000
N_SM = 10000
N_SEED = 20000
STREAMS = LR.streams()


def small_context(n, orc=None):
    D = LR.small_case(n)[0]
    orc = LR.small_oracle(n) if orc is None else orc
    ctx = rc.Context(D, logD=orc.logD)
    ctx.set_params(**LR.PARAMS)
    return ctx


def device_restart(ctx, start, r, p, blocking=True):
    def sweep_from(seed, s):
        ctx.set_state(start)
        ctx.gibbs_sweep(r, p, seed, s, blocking=blocking)
        if not blocking:
            ctx.synchronize()
        return ctx.get_state()[0]
    return sweep_from


def device_chain(ctx, start, r, p):
    ctx.set_state(start)

    def sweep(seed, s):
        ctx.gibbs_sweep(r, p, seed, s)
        return ctx.get_state()[0]
    return sweep


@pytest.mark.parametrize("stream", STREAMS, ids=[s[2] for s in STREAMS])
@pytest.mark.parametrize("mode", ["full", "incremental"])
@pytest.mark.parametrize("n", [5, 6])
def test_sweep_restart(n, mode, stream):
    """set_state, one sweep, get_state, 20 000 times: the labellings' frequencies follow the exact law of one sweep, and
    equal the oracle's count for count"""
    seed, index, name = stream
    start = LR.small_case(n)[1]
    ctx = small_context(n)
    try:
        ctx.set_mode(mode)
        counts = LR.restart_counts(device_restart(ctx, start, LR.R0, LR.P0), seed, index, N_RESTART)
    finally:
        ctx.close()
    LR.assert_consistent(f"gpu sweep restart n={n} {mode} {name}", counts, LR.law_cache(n)(start), N_RESTART)
    assert counts == LR.oracle_restart_counts(n, seed, index, N_RESTART)


def test_sweep_restart_async():
    """the same through rc_gibbs_sweep_async + rc_synchronize"""
    seed, index, name = STREAMS[3]
    start = LR.small_case(6)[1]
    ctx = small_context(6)
    try:
        counts = LR.restart_counts(device_restart(ctx, start, LR.R0, LR.P0, blocking=False), seed, index, N_RESTART)
    finally:
        ctx.close()
    LR.assert_consistent(f"gpu sweep restart n=6 async {name}", counts, LR.law_cache(6)(start), N_RESTART)
    assert counts == LR.oracle_restart_counts(6, seed, index, N_RESTART)


@pytest.mark.parametrize("seed", LR.SEEDS[:2], ids=hex)
def test_sweep_chain(seed):
    """a free-running chain with get_state after every sweep: every source state of at least 200 visits against its exact
    law; with 100 000 sweeps the same counts must also reject the three slightly wrong laws"""
    start = LR.small_case(6)[1]
    ctx = small_context(6)
    try:
        path = LR.chain_path(device_chain(ctx, start, LR.R0, LR.P0), start, seed, N_CHAIN)
    finally:
        ctx.close()
    trans = LR.transitions(path)
    stat, df, share = LR.chi2_transitions(trans, LR.law_cache(6))
    LR.report(f"gpu sweep chain n=6 {seed:#x}", stat, df, N=N_CHAIN, share=share)
    assert share >= 0.9
    assert stat <= LR.bound(df)
    assert path == LR.oracle_chain_path(seed, N_CHAIN)
    if N_CHAIN < 100000:
        print("power assertion left out: it is stated for 100 000 sweeps, this chain has", N_CHAIN)
        return
    for which in LR.PERTURBED:
        s2, d2, _ = LR.chi2_transitions(trans, LR.law_cache(6, which))
        LR.report(f"gpu sweep chain n=6 {seed:#x} against {which}", s2, d2)
        assert s2 > LR.bound(d2), which


def test_two_consecutive_sweeps():
    """sweeps 2k and 2k + 1 from the start against the composed law"""
    seed = LR.SEEDS[1]
    start = LR.small_case(5)[1]
    ctx = small_context(5)

    def two(seed, k):
        ctx.set_state(start)
        ctx.gibbs_sweep(LR.R0, LR.P0, seed, 2 * k)
        ctx.gibbs_sweep(LR.R0, LR.P0, seed, 2 * k + 1)
        return ctx.get_state()[0]
    try:
        counts = LR.restart_counts(two, seed, int, N_TWO)
    finally:
        ctx.close()
    LR.assert_consistent(f"gpu two sweeps n=5 {seed:#x}", counts, LR.small_law2(5), N_TWO)


def large_context(n):
    D, P, start = LR.large_case(n)
    orc = O.Oracle(D, P)
    ctx = rc.Context(D, logD=orc.logD)
    ctx.set_params(**P)
    return ctx, orc, start


@pytest.mark.parametrize("n,nsweeps", [(135, 2000), (1029, 300)])
def test_calibration_of_a_device_chain(n, nsweeps):
    """n = 135 (one full column block plus seven rows) and n = 1029, where the other kernels and the re-layout run: every
    visit of a free-running device chain replayed on the oracle at the labels the device drew.  How often the most probable
    candidate, and the new cluster, were drawn against the sum of their probabilities: |Z| <= 4.9 for both."""
    ctx, orc, start = large_context(n)
    try:
        path = LR.device_path(device_chain(ctx, start, LR.LARGE_R, LR.LARGE_P), start, LR.LARGE_R, LR.LARGE_P, LR.SEEDS[1], nsweeps)
    finally:
        ctx.close()
    res = LR.calibration(path, orc)
    print(f"LAW gpu calibration n={n} sweeps={nsweeps}: {res}")
    assert res["visits"] == n * nsweeps and res["median_p_top"] < 0.9
    assert abs(res["z_top"]) <= LR.Z_BOUND and abs(res["z_new"]) <= LR.Z_BOUND


def test_sweep_restart_first_three_points_n135():
    """restart protocol at n = 135: the first three points' labels against sweep_law(depth=3)"""
    seed = LR.SEEDS[2]
    ctx, orc, start = large_context(135)
    D, P, _ = LR.large_case(135)
    try:
        counts = LR.restart_counts(device_restart(ctx, start, LR.LARGE_R, LR.LARGE_P), seed, LR.high_index, N_RESTART, take=3)
    finally:
        ctx.close()
    law = LR.sweep_law(D, P, start, LR.LARGE_R, LR.LARGE_P, depth=3)
    LR.assert_consistent(f"gpu sweep restart n=135 depth=3 {seed:#x}-high", counts, law, N_RESTART)


@pytest.mark.parametrize("state", list(LR.SM_STATES))
def test_splitmerge_proposal(state):
    """rc_splitmerge has one mode — an accepted proposal becomes the state ("intended"; the as-written loop is the caller's
    checkpoint / restore): (accept, split, labels afterwards) against the enumerated law and against the oracle's, draw by draw"""
    seed = LR.SEEDS[1]
    D = LR.small_case(LR.SM_N)[0]
    orc = LR.small_oracle(LR.SM_N)
    start = np.array(LR.SM_STATES[state], np.int64)
    ctx = small_context(LR.SM_N, orc)
    outs = []
    try:
        ctx.attach_host_matrices(D, orc.logD)
        for it in range(N_SM):
            ctx.set_state(start)
            a, s = ctx.splitmerge(LR.R0, LR.P0, 1, seed, it, 0)
            outs.append((a, s, LR.as_key(ctx.get_state()[0])))
    finally:
        ctx.close()
    LR.assert_consistent(f"gpu splitmerge {state} {seed:#x}", LR.count(outs), LR.sm_law(state), N_SM)
    assert outs == LR.oracle_proposals(state, seed, N_SM)


SEED_CASES = [("plain", 2), ("plain", 3), ("close", 3)]


@pytest.mark.parametrize("case,k", SEED_CASES)
def test_kmeanspp_seeds(case, k):
    """kmeans(k, maxiter=0): the centres are the seeds, read back by matching them to the rows of X"""
    X = LR.seeding_points(case)
    row = {tuple(x): i for i, x in enumerate(X.tolist())}
    assert len(row) == len(X)
    ctx = rc.Context.from_points(X)
    try:
        counts = LR.seeding_counts(lambda s: [row[tuple(c)] for c in ctx.kmeans(k, maxiter=0, seed=s).centers.tolist()], N_SEED)
    finally:
        ctx.close()
    LR.assert_consistent(f"gpu kmeans++ {case} k={k}", counts, LR.kmeanspp_law(X, k), 2 * N_SEED)
    assert counts == LR.seeding_counts(lambda s: KM.kmpp_seeds(X, k, s), N_SEED)


@pytest.mark.parametrize("case,k", SEED_CASES)
def test_kmedoidspp_seeds(case, k):
    """kmedoids(k, maxiter=0): the medoids are the seeds, in the order they were drawn"""
    ctx = rc.Context(LR.distances(LR.seeding_points(case)))
    try:
        Dq, _ = KD.device_matrix(ctx)
        counts = LR.seeding_counts(lambda s: ctx.kmedoids(k, maxiter=0, seed=s).medoids - 1, N_SEED)
    finally:
        ctx.close()
    LR.assert_consistent(f"gpu kmedoids++ {case} k={k}", counts, LR.kmedoidspp_law(Dq, k), 2 * N_SEED)
    assert counts == LR.seeding_counts(lambda s: KD.kmpp_seeds(Dq, k, s), N_SEED)
