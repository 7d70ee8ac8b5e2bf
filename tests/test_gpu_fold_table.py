"""k_bulk_syml2's log table with the exponent folded in (rc_qlog_prep_f) and its fallback k_bulk_syml2w (-m gpu).

A derived context whose off-diagonal entries span at most four binades runs k_bulk_syml2 on the folded table; any wider range runs
k_bulk_syml2w, which derives the exponent per entry.  Both must give the integers rc_qlog defines.  Four matrices at the headline
size (N = 8192, K = 50, bench.py's data set, D in [0.59, 2.44]: three binades):
  * `inside`  the data set itself                                  -> folded
  * `four`    one pair of entries moved into [0.25, 0.5)           -> exactly four binades, folded
  * `five`    one more pair moved into [0.125, 0.25)               -> five binades, fallback
  * `outside` a few entries scaled by 2^-6                          -> nine binades, fallback
each compared with the CPU oracle as tests/test_gpu_headline.py::test_headline_config_against_oracle does (labels, sizes, K, change
counts exactly; fixed-point row sums of both matrices bit for bit; loglik 1e-9 / 1e-6 relative), and the row sums of a context forced
onto the fallback (rc_set_option "fold_log_table" 0) compared with the folded kernel's for the same in-range matrices.
"""
import numpy as np
import pytest

import oracle_lib as O
import redclust_amd as rc
from helpers import assert_derived_log_close, rp_schedule

pytestmark = pytest.mark.gpu

N, K = 8192, 50
NAME = "k_bulk_syml2<true, true>"                          # rc_bulk_kernel_name: both forms; rc_log_table_folded tells them apart
CASES = {"inside": True, "four": True, "five": False, "outside": False}    # folded?


@pytest.fixture(scope="module")
def data():
    d = rc.generatemixture(N, K, seed=1)
    D, truth = d["distancematrix"], d["clusts"]
    return dict(D=D, truth=truth, P=rc.likelihood_hyperparams(D, truth))


def _matrix(D, case):
    D = D.copy()

    def put(i, j, v):
        D[i, j] = v; D[j, i] = v
    off = D[~np.eye(N, dtype=bool)]
    assert 0.5 <= off.min() and off.max() < 4.0          # three binades: [0.5, 1), [1, 2), [2, 4)
    if case in ("four", "five"):
        put(3, 4100, 0.3)                                # two pairs of points, in different clusters and in the same one
        put(5000, 5001, 0.3)
    if case == "five":
        put(17, 6000, 0.15)
    if case == "outside":
        rng = np.random.default_rng(5)
        for i, j in zip(rng.integers(0, N, 40), rng.integers(0, N, 40)):
            if i != j:
                put(i, j, D[i, j] * 2.0 ** -6)
    return D


@pytest.fixture(scope="module", params=list(CASES))
def setup(request, data):
    case = request.param
    D = _matrix(data["D"], case)
    ctx = rc.Context(D)                                   # as bench.py: D only, automatic kernel
    ctx.set_params(**data["P"])
    ctx.set_state(data["truth"])
    L = ctx.get_matrix(1)
    eD, eL = ctx.debug_rowsums(1)[2:4]
    assert_derived_log_close(L, D, eD, eL)                # the device's logD is log(D) (the bound DESIGN.md §3 derives)
    hostL = np.log(np.where(np.eye(N, dtype=bool), 1.0, D))
    orc = O.Oracle(D, data["P"], logD=L, eL=eL, eD=eD)
    yield dict(case=case, D=D, ctx=ctx, orc=orc, hostL=hostL, truth=data["truth"], P=data["P"])
    ctx.close()


def _init(kind, truth):
    n = len(truth)
    if kind == "stationary":
        return truth.copy()
    if kind == "perturbed":                                # 2 % of the labels re-drawn
        init = truth.copy()
        idx = np.random.default_rng(11).choice(n, n // 50, replace=False)
        init[idx] = np.random.default_rng(12).integers(1, K + 1, size=len(idx))
        return init
    return np.random.default_rng(13).integers(1, K + 1, size=n).astype(np.int64)   # uniform on 1..K


@pytest.mark.parametrize("kind", ["stationary", "perturbed", "uniform"])
def test_folded_and_fallback_against_oracle(setup, kind):
    s = setup
    ctx, orc, kernel = s["ctx"], s["orc"], NAME
    assert ctx.log_table_folded() == CASES[s["case"]], s["case"]
    init = _init(kind, s["truth"])
    ctx.set_state(init)
    orc.set_state(init)
    nsweeps = 4
    names, moved = [], 0
    for t in range(nsweeps):
        r, p = rp_schedule(t)
        ctx.gibbs_sweep(r, p, 8192, t)
        names.append(ctx.bulk_kernel_name())
        orc.sweep_stable(r, p, 8192, t)
        lab, sizes, Kc = ctx.get_state()
        assert np.array_equal(lab, orc.clusts), (s["case"], kind, t, int(np.sum(lab != orc.clusts)))
        assert np.array_equal(sizes, orc.sizes) and Kc == orc.K, (s["case"], kind, t)
        st = ctx.sweep_stats()
        assert st["n_changes"] == orc.last_changes and st["K"] == orc.K, (s["case"], kind, t, st, orc.last_changes)
        moved += st["n_changes"]
    assert names[0] == kernel, (s["case"], names)         # the sweep right after rc_set_state sees a cluster-contiguous layout
    if kind == "stationary":
        assert all(x == kernel for x in names), (s["case"], names)
    else:
        assert moved > (50 if kind == "perturbed" else N // 2)
    for k in np.unique(orc.clusts)[[0, 7, -1]]:           # the row-sum table after four sweeps, both matrices, bit for bit
        sd, sl, eD, eL = ctx.debug_rowsums(int(k))
        m = orc.clusts == k
        assert (eD, eL) == (orc.eD, orc.eL)
        assert np.array_equal(sd, orc.Dq[:, m].sum(axis=1)) and np.array_equal(sl, orc.Lq[:, m].sum(axis=1)), (s["case"], kind, k)
    ll = ctx.loglik()
    ref = orc.loglik_stable()
    assert abs(ll - ref) <= 1e-9 * abs(ref), (ll, ref)
    lit = orc.loglik_literal()
    assert abs(ll - lit) <= 1e-6 * abs(lit), (ll, lit)
    lit_host = O.lib().orc_loglik_literal(N, s["D"].reshape(-1), s["hostL"].reshape(-1), orc.clusts, orc.sizes, orc.P)
    assert abs(ll - lit_host) <= 1e-6 * abs(lit_host), (ll, lit_host)
    lp = ctx.logprior(*rp_schedule(nsweeps - 1))
    assert abs(lp - orc.logprior(*rp_schedule(nsweeps - 1))) <= 1e-12 * abs(lp)
    final = orc.clusts.copy()                             # the same sweeps enqueued without host synchronisation end in the same state
    ctx.set_state(init)
    for t in range(nsweeps):
        r, p = rp_schedule(t)
        ctx.gibbs_sweep(r, p, 8192, t, blocking=False)
    ctx.synchronize()
    lab, sizes, Kc = ctx.get_state()
    assert np.array_equal(lab, final) and Kc == orc.K and ctx.loglik() == ll


@pytest.mark.parametrize("case", ["inside", "four"])
def test_forced_fallback_gives_the_same_row_sums(data, case):
    """The same in-range matrix through k_bulk_syml2 (folded table, bias taken off per flush) and through k_bulk_syml2w: every row
    sum of every cluster, both matrices, after a stationary start and after sweeps from a perturbed one (units with stray lanes,
    donor lanes and mid-unit flushes)."""
    D = _matrix(data["D"], case)
    ctxs = []
    for fold in (1, 0):
        ctx = rc.Context(D)
        ctx.set_option("fold_log_table", fold)
        ctx.set_params(**data["P"])
        ctxs.append(ctx)
    try:
        for kind in ("stationary", "perturbed", "uniform"):
            init = _init(kind, data["truth"])
            out = []
            for ctx, folded in zip(ctxs, (True, False)):
                assert ctx.log_table_folded() == folded
                ctx.set_state(init)
                for t in range(3):
                    r, p = rp_schedule(t)
                    ctx.gibbs_sweep(r, p, 8192, t)
                    if t == 0:
                        assert ctx.bulk_kernel_name() == NAME, (case, kind, ctx.bulk_kernel_name())
                lab = ctx.get_state()[0]
                sums = [ctx.debug_rowsums(int(k))[:2] for k in np.unique(lab)]
                out.append((lab, sums))
            assert np.array_equal(out[0][0], out[1][0]), (case, kind)
            assert len(out[0][1]) == len(out[1][1])
            for (sd0, sl0), (sd1, sl1) in zip(out[0][1], out[1][1]):
                assert np.array_equal(sd0, sd1) and np.array_equal(sl0, sl1), (case, kind)
    finally:
        for ctx in ctxs:
            ctx.close()
