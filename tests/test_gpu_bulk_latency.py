"""The row stream of k_bulk_syml2 with L2 warm-up touches (-m gpu; RC_S2_STEPS bit 128).

Behind every request of a row pair the folded kernel touches the row pair four rows further down the same unit (in launches
beside the stationary resolver: View.s2_touch): one dword per 128-byte line, into a register nothing reads.  A touch must never leave the unit being requested, and nothing it does
may change a sum; k_bulk_syml2w and the stored form carry no touches and must be what they were.

Cases (rows of tests/bulk_rows.py, the symmetric kernel forced; bulk_rows.check_table: every S entry of both matrices bit for
bit against plain integer sums, the sum over the labels against rc_debug_rowtotals):
  a  n = 384, three unequal clusters: one short unit per wave; the units' tails touch nothing;
  b  n = 392 (a last column block of eight columns: padding) and n = 389 (its rows are no multiple of 8: k_bulk_syml_list
     runs behind the fast launch);
  c  units of 8 rows (rc_set_option "syml2_unit_rows": the plan's own choice gives every wave one unit below n ~ 14 000):
     n = 1536 with RC_SYMW_PER_CU=1 and RC_SW_COARSE=8 around the context's creation as well — switches of a diagnostic
     build (-DRC_DIAG, RC_LIB_PATH), where that is 1 248 one-group units on 1 024 waves; the product build ignores them and
     keeps its 3 072 waves — and n = 2560, 3 360 one-group units, more than the product's waves.  Where the plan
     (rc_bulk_plan_info) has more units than waves the case asserts that some wave holds two: requests cross a unit
     boundary there, and in an 8-row unit only the first two requests have rows left to touch;
  d  case a with fold_log_table 0: k_bulk_syml2w;
  e  two consecutive sweeps with label changes in the first: the reductions read both generations of the slot snapshot."""
import contextlib
import os

import numpy as np
import pytest

import bulk_rows as B
import redclust_amd as rc
import test_gpu_bulk_matrix as M

pytestmark = pytest.mark.gpu

ROW = {r.id: r for r in B.ROWS}


@contextlib.contextmanager
def geometry(**kv):
    """launch-geometry switches, read once per context in rc_create: set around make_context only"""
    saved = {k: os.environ.get(k) for k in kv}
    try:
        os.environ.update({k: str(v) for k, v in kv.items()})
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def three_unequal(n):
    """contiguous runs of about n/8, n/2 and the rest, both boundaries odd (a split lane each)"""
    idx = np.arange(n)
    return (1 + (idx >= n // 8 + 1) + (idx >= n // 8 + n // 2 + 2)).astype(np.int64)


def run(row, n, labs, env=None, unit_rows=0, two_units=False):
    D = M.matrix(row.data, n)
    with geometry(**(env or {})):
        ctx, L_host = B.make_context(row, D)
    try:
        if unit_rows:
            ctx.set_option("syml2_unit_rows", unit_rows)
            plan = ctx.syml2_plan_info()
            assert plan["unit_rows"] == unit_rows, plan
            assert plan["max_units_per_wave"] >= 2 or not (two_units or plan["fast_units"] > plan["waves"]), plan
        ctx.set_state(np.ones(n, np.int64))
        Dq, Lq, _, _ = B.reference_matrices(row, ctx, D, L_host)
        assert ctx.log_table_folded() == (row.fold == 1)
        for name, lab in labs.items():
            ctx.set_state(lab)
            B.check_table(ctx, Dq, Lq, lab, (row.id, n, name), ks=np.unique(lab))
            assert ctx.bulk_kernel_name() == row.name, (name, ctx.bulk_kernel_name())
    finally:
        ctx.close()


def test_a_short_units():
    run(ROW["01"], 384, {"three_unequal": three_unequal(384), "one": np.ones(384, np.int64)})


@pytest.mark.parametrize("n", [392, 389])
def test_b_ragged_last_block(n):
    run(ROW["01"], n, {"three_unequal": three_unequal(n)})


@pytest.mark.parametrize("n", [1536, 2560])
def test_c_two_units_per_wave(n):
    idx = np.arange(n)
    labs = {"three_unequal": three_unequal(n),
            # the rows' cluster changes inside 8-row groups and at group and half boundaries
            "runs_of_37": (1 + idx // 37).astype(np.int64)}
    # (n = 2560: 64 * 20 * 21 / 8 = 3 360 units; a device with more than 840 CUs would need a larger n)
    run(ROW["01"], n, labs, env=dict(RC_SYMW_PER_CU=1, RC_SW_COARSE=8), unit_rows=8, two_units=n == 2560)


def test_d_unfolded_table():
    run(ROW["02-nofold"], 384, {"three_unequal": three_unequal(384)})


def test_e_both_snapshot_generations():
    n, K = 384, 3
    data = rc.generatemixture(n, K, seed=17, sigma=0.35)
    D0, truth = data["distancematrix"], data["clusts"]
    D = np.where(np.eye(n, dtype=bool), 0.0, 0.5 + 3.4 * D0 / D0.max())           # three binades: the folded table
    rng = np.random.default_rng(5)
    init = truth.copy()
    moved = rng.choice(n, n // 12, replace=False)
    init[moved] = rng.integers(1, K + 3, len(moved))
    row = ROW["01"]
    ctx, L_host = B.make_context(row, D)
    try:
        ctx.set_params(**rc.likelihood_hyperparams(D, truth))
        ctx.set_state(init)
        Dq, Lq, _, _ = B.reference_matrices(row, ctx, D, L_host)
        B.check_table(ctx, Dq, Lq, init, "initial state", ks=np.unique(init))
        for t in range(2):
            ctx.gibbs_sweep(1.0, 0.5, 77, t, blocking=False)
        ctx.synchronize()
        lab = ctx.get_state()[0]
        assert (lab != init).any()                                               # the first sweep moved points
        B.check_table(ctx, Dq, Lq, lab, "after two pipelined sweeps", ks=np.unique(lab))
        for t in range(2, 4):                                                    # and blocking: a table per sweep
            ctx.gibbs_sweep(1.0, 0.5, 77, t)
            lab = ctx.get_state()[0]
            B.check_table(ctx, Dq, Lq, lab, ("after sweep", t), ks=np.unique(lab))
            assert ctx.bulk_kernel_name() == row.name
    finally:
        ctx.close()
