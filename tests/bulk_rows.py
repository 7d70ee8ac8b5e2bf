"""The rows of BULK_KERNELS (csrc/redclust_hip.hip: what bulk_choice can return) that a product build reaches, as a table, and the
pieces tests/test_gpu_bulk_matrix.py and tests/test_gpu_diagonal.py share: creating a context that must end up in a given
kernel, the fixed-point reference matrices and their per-cluster row sums.

The choice depends on (i) the storage (64-bit with logD derived on the fly, 64-bit with logD stored, 32-bit), (ii) the
environment switch RC_SYM_VARIANT, read once per context, and (iii) the symmetric / full-read choice (rc_set_bulk_kernel or
RC_BULK_KERNEL).  k_bulk_syml_list<true|false> has no name of its own: it runs behind k_bulk_syml2 whenever the last 128-column
block has a row count that is not a multiple of 8."""
import contextlib
import os
from collections import namedtuple

import numpy as np

import oracle_lib as O
import redclust_amd as rc
from helpers import assert_derived_log_close, rp_schedule

LL_RTOL = 1e-9

Row = namedtuple("Row", "id storage variant kernel name data fold")
#    id          storage    RC_SYM_VARIANT  kernel  rc_bulk_kernel_name            data      fold_log_table
ROWS = [
    Row("01",        "derived", None, "sym",  "k_bulk_syml2<true, true>",   "narrow", 1),   # folded log table
    Row("02-wide",   "derived", None, "sym",  "k_bulk_syml2<true, true>",   "wide",   1),   # k_bulk_syml2w: > 4 binades
    Row("02-nofold", "derived", None, "sym",  "k_bulk_syml2<true, true>",   "narrow", 0),   # k_bulk_syml2w: by option
    Row("03",        "derived", "2",  "sym",  "k_bulk_syml<true>",          "wide",   1),
    Row("04",        "derived", "1",  "sym",  "k_bulk_symw<true>",          "wide",   1),
    Row("05",        "derived", "0",  "sym",  "k_bulk_sym<true>",           "wide",   1),
    Row("06",        "derived", None, "perm", "k_bulk<long long, true>",    "wide",   1),
    Row("07",        "stored",  None, "sym",  "k_bulk_sym<false>",          "narrow", 1),
    Row("08",        "stored",  "1",  "sym",  "k_bulk_symw<false>",         "narrow", 1),
    Row("09",        "stored",  "2",  "sym",  "k_bulk_syml<false>",         "narrow", 1),
    Row("10",        "stored",  "3",  "sym",  "k_bulk_syml2<false, false>", "narrow", 1),
    Row("11",        "stored",  None, "perm", "k_bulk<long long, false>",   "narrow", 1),
    Row("12",        "32",      None, "sym",  "k_bulk_sym32",               "narrow", 1),
    Row("13",        "32",      "2",  "sym",  "k_bulk_syml32",              "narrow", 1),
    Row("14",        "32",      None, "perm", "k_bulk<int, false>",         "narrow", 1),
]
ROW_IDS = [f"{r.id}-{r.name}" for r in ROWS]
DEFAULT_ROWS = [r for r in ROWS if r.id in ("01", "07", "12")]           # what a caller gets without any switch
SWITCHES = ("RC_SYM_VARIANT", "RC_NO_RELAYOUT", "RC_STORED_LOG", "RC_BULK_KERNEL")


@contextlib.contextmanager
def environment(**kv):
    """The library reads its switches once, in rc_create: they are set around rc.Context(...) only (None: not set)."""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            v = kv.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def host_log(D):
    """types.jl:155 — log.(D - Diagonal(D) + I)"""
    return np.log(np.where(np.eye(D.shape[0], dtype=bool), 1.0, D))


def make_context(row, D, relayout=True, kernel_by_env=False, kcap=0, env=None):
    """A context of the row's storage with the row's switches; (ctx, the host logD handed in or None)."""
    L = None if row.storage == "derived" else host_log(D)
    kv = dict(RC_SYM_VARIANT=row.variant, RC_NO_RELAYOUT=None if relayout else "1")
    if kernel_by_env:
        kv["RC_BULK_KERNEL"] = row.kernel
    kv.update(env or {})
    with environment(**kv):
        ctx = rc.Context(D, logD=L, kcap=kcap, storage_bits=32 if row.storage == "32" else 64)
    if not kernel_by_env:
        ctx.set_bulk_kernel(row.kernel)
    if row.fold != 1:
        ctx.set_option("fold_log_table", row.fold)
    return ctx, L


def quantise(X, e):
    """rint(X·2^e) as int64: a double scaled by a power of two is exact, so this owes nothing to the device"""
    return np.rint(np.ldexp(X, e)).astype(np.int64)


def binades(Dq):
    """number of consecutive binades the off-diagonal fixed-point entries span (0 without any)"""
    n = Dq.shape[0]
    off = Dq[~np.eye(n, dtype=bool)]
    if off.size == 0:
        return 0
    assert off.min() > 0
    return int(np.floor(np.log2(float(off.max())))) - int(np.floor(np.log2(float(off.min())))) + 1


def expected_folded(row, Dq):
    """a derived context reads the folded log table when its entries span at most four binades (and the option
    is on); stored contexts never do."""
    return row.storage == "derived" and row.fold == 1 and binades(Dq) <= 4


def reference_matrices(row, ctx, D, L_host):
    """(Dq, Lq, eD, eL) — the integers the kernels must sum.  D: rint(D·2^eD) with the exponent the library reports.  logD of a
    stored context: the same of the host's logD that was handed in.  logD of a derived context: the integers rc_qlog defines, read
    through rc_get_matrix(1) (k_derived_matrix, a per-entry kernel that shares nothing with the reductions) and held against
    libm's log entry by entry.  The caller must have set a state (rc_debug_rowsums reports the exponents)."""
    eD, eL = ctx.debug_rowsums(1)[2:4]
    Dq = quantise(D, eD)
    if row.storage == "derived":
        assert (Dq[~np.eye(len(D), dtype=bool)] >= 2 ** 32).all(), "the matrix would not stay derived (create_impl)"
        L = ctx.get_matrix(1)
        assert_derived_log_close(L, D, eD, eL)
        Lq = quantise(L, eL)
        assert np.array_equal(np.ldexp(Lq.astype(np.float64), -eL), L)       # L was a multiple of the quantum
    else:
        Lq = quantise(L_host, eL)
    return Dq, Lq, eD, eL


def cluster_rowsums(Xq, labels, ks):
    """Xq[:, labels == k].sum(axis=1) for every k of ks, as rows of the result.  Xq is symmetric off the diagonal (asserted by
    the caller), so the columns of a cluster are summed as rows — contiguous — plus the diagonal term of its own points."""
    out = np.empty((len(ks), Xq.shape[0]), np.int64)
    for q, k in enumerate(ks):
        out[q] = Xq[labels == k].sum(axis=0)
    return out


def pick_clusters(labels, limit=64):
    """every label if there are at most `limit`; else `limit` of them with the first and the last label and the smallest and the
    largest cluster among them"""
    ks, cnt = np.unique(labels, return_counts=True)
    if len(ks) <= limit:
        return ks
    must = {int(ks[0]), int(ks[-1]), int(ks[np.argmin(cnt)]), int(ks[np.argmax(cnt)])}
    rest = [int(k) for k in np.random.default_rng(len(labels)).permutation(ks) if int(k) not in must]
    return np.array(sorted(must | set(rest[:limit - len(must)])), np.int64)


def check_table(ctx, Dq, Lq, labels, what, ks=None, ref=None):
    """rc_debug_rowsums of the clusters ks (default: pick_clusters) against the reference sums, both matrices bit for bit, and
    Σ_labels rc_debug_rowsums == rc_debug_rowtotals == the reference's row totals.  ref: precomputed (ks, sums of Dq, sums of Lq,
    totals of Dq, totals of Lq).  Returns ref."""
    if ref is None:
        ks = pick_clusters(labels) if ks is None else np.asarray(ks)
        ref = (ks, cluster_rowsums(Dq, labels, ks), cluster_rowsums(Lq, labels, ks), Dq.sum(axis=1), Lq.sum(axis=1))
    ks, rd, rl, td, tl = ref
    where = {int(k): q for q, k in enumerate(ks)}
    sum_d = np.zeros(len(labels), np.int64); sum_l = np.zeros(len(labels), np.int64)
    for k in np.unique(labels):
        sd, sl = ctx.debug_rowsums(int(k))[:2]
        sum_d += sd; sum_l += sl
        q = where.get(int(k))
        if q is not None:
            assert np.array_equal(sd, rd[q]), (what, "D", int(k), np.flatnonzero(sd != rd[q])[:8], (sd - rd[q])[sd != rd[q]][:8])
            assert np.array_equal(sl, rl[q]), (what, "logD", int(k), np.flatnonzero(sl != rl[q])[:8], (sl - rl[q])[sl != rl[q]][:8])
    gd, gl = ctx.debug_rowtotals()
    assert np.array_equal(gd, td) and np.array_equal(gl, tl), (what, "rc_debug_rowtotals")
    assert np.array_equal(sum_d, td) and np.array_equal(sum_l, tl), (what, "sum over the labels", np.flatnonzero(sum_d != td)[:8],
                                                                      np.flatnonzero(sum_l != tl)[:8])
    return ref


def sweep_data():
    n, K = 1029, 6
    data = rc.generatemixture(n, K, seed=17, sigma=0.35)
    D0, truth = data["distancematrix"], data["clusts"]
    narrow = np.where(np.eye(n, dtype=bool), 0.0, 0.5 + 3.4 * D0 / D0.max())       # [0.5, 3.9]: three binades
    wide = narrow.copy()
    rng = np.random.default_rng(5)
    for i, j in zip(rng.integers(0, n, 60), rng.integers(0, n, 60)):
        if i != j:
            wide[i, j] = wide[j, i] = narrow[i, j] * 2.0 ** -6
    init = truth.copy()
    idx = rng.choice(n, n // 12, replace=False)
    init[idx] = rng.integers(1, K + 3, len(idx))
    return dict(narrow=narrow, wide=wide), truth, init


def run_sweeps(row, D, P, init, nsweeps=6, seed=77):
    """Shared with tests/test_gpu_diagonal.py: blocking sweeps against the oracle, then the same non-blocking, then incremental
    (blocking and non-blocking).  Returns (loglik of the final state, the oracle)."""
    ctx, L_host = make_context(row, D)
    try:
        ctx.set_params(**P)
        ctx.set_state(init)
        Dq, Lq, eD, eL = reference_matrices(row, ctx, D, L_host)
        orc = O.Oracle(D, P, logD=np.ldexp(Lq.astype(np.float64), -eL), eD=eD, eL=eL, bits=32 if row.storage == "32" else 64)
        assert np.array_equal(orc.Dq, Dq) and np.array_equal(orc.Lq, Lq)
        orc.set_state(init)
        check_table(ctx, Dq, Lq, init, (row.id, "initial state"))
        moved = 0
        for t in range(nsweeps):
            r, p = rp_schedule(t)
            ctx.gibbs_sweep(r, p, seed, t)
            orc.sweep_stable(r, p, seed, t)
            assert ctx.bulk_kernel_name() == row.name, (row.id, t, ctx.bulk_kernel_name())
            lab, sizes, K = ctx.get_state()
            assert np.array_equal(lab, orc.clusts), (row.id, t, int(np.sum(lab != orc.clusts)))
            assert np.array_equal(sizes, orc.sizes) and K == orc.K, (row.id, t)
            st = ctx.sweep_stats()
            assert st["n_changes"] == orc.last_changes and st["K"] == orc.K, (row.id, t, st, orc.last_changes)
            moved += st["n_changes"]
        assert moved > 20, moved
        ll, ref = ctx.loglik(), orc.loglik_stable()
        assert np.isfinite(ref) and abs(ll - ref) <= LL_RTOL * abs(ref), (row.id, ll, ref)
        check_table(ctx, Dq, Lq, orc.clusts, (row.id, "after the sweeps"))
        for mode, blocking in (("full", False), ("incremental", True), ("incremental", False)):
            what = (row.id, mode, "blocking" if blocking else "non-blocking")
            ctx.set_mode("full")
            ctx.set_state(init)
            ctx.set_mode(mode)
            for t in range(nsweeps):
                r, p = rp_schedule(t)
                ctx.gibbs_sweep(r, p, seed, t, blocking=blocking)
            ctx.synchronize()
            lab, sizes, K = ctx.get_state()
            assert np.array_equal(lab, orc.clusts) and np.array_equal(sizes, orc.sizes) and K == orc.K, what
            assert ctx.loglik() == ll, what
            check_table(ctx, Dq, Lq, orc.clusts, what)
            assert ctx.bulk_kernel_name() == row.name, what
        return ll, orc
    finally:
        ctx.close()
