"""Direction 2 of k_bulk_syml2 / k_bulk_syml2w in column blocks that span two clusters (-m gpu).

syml2_fast splits the transposed sums of such a unit by class without per-lane branches when the lanes of one cluster all lie above
the whole lanes of the other (one lane octet is then split at a uniform position; RC_S2_STEPS bit 16), hands a donor lane's second
column to its neighbour as a single-lane operation (bit 32) and keeps the per-row totals as 32-bit halves (bit 64); any other
arrangement of the two clusters' lanes, and units with more than one donor, keep the per-lane code.  Every S entry must keep its
bits either way.

Shapes: n = 384 — three 128-column blocks, so the blocks 128..255 and 256..383 hold fast units (rows 0..127 / 0..255, multiples of
8) — and the ragged n = 389.  Rows 01, 02-nofold, 02-wide and 10 of tests/bulk_rows.py, each on its own matrix kind (02-wide needs
the wide matrix to reach k_bulk_syml2w; the others run on `narrow`), the symmetric kernel forced, with the cluster-contiguous
re-layout on and off (RC_NO_RELAYOUT=1: the columns lie exactly as labelled).  Labellings:
  * two contiguous runs with the boundary at b = base + 2 (8 tq + j) + par, base = 128 and 256, tq in {0, 3, 4, 7} (first, last,
    unswizzled and swizzled octets), j = 0..7, par = 0, 1 (1: a lane is split, a donor) — the upper run is the block's majority
    (cluster A) for small tq and its minority (B) for large tq, and the first run is the smaller cluster overall for some
    boundaries and the larger for others;
  * three runs inside one block (the smallest goes through the stray-lane atomics);
  * 1,1,...,2,2,...,1,1,... inside one block: without re-layout cluster B's lanes are no single run at the top or the bottom of the
    wave (per-lane code), and with two odd boundaries the unit has two donors;
  * a change of the rows' cluster inside an 8-row group above a two-cluster block (flush1 between the group's writes and its read).
Checks (bulk_rows.check_table): every S entry of both matrices bit for bit against plain integer sums, the sum over the labels
against rc_debug_rowtotals; rc_bulk_kernel_name is the row's kernel in every case."""
import numpy as np
import pytest

import bulk_rows as B
import test_gpu_bulk_matrix as M

pytestmark = pytest.mark.gpu

ROWS = [r for r in B.ROWS if r.id in ("01", "02-nofold", "02-wide", "10")]
SIZES = (384, 389)


def labelings(n):
    out = {}
    idx = np.arange(n)
    for base in (128, 256):
        for tq in (0, 3, 4, 7):
            for j in range(8):
                for par in (0, 1):
                    b = base + 2 * (8 * tq + j) + par
                    out[f"two_runs_b{b}"] = np.where(idx < b, 1, 2).astype(np.int64)
    for name, cuts in (("three_runs_165_218", (165, 218)), ("three_runs_150_151", (150, 151)), ("three_runs_130_254", (130, 254)),
                       ("three_runs_block3_300_341", (300, 341))):
        out[name] = (1 + (idx >= cuts[0]) + (idx >= cuts[1])).astype(np.int64)
    for name, (lo, hi) in (("sandwich_171_221", (171, 221)), ("sandwich_170_220", (170, 220)), ("sandwich_129_255", (129, 255)),
                           ("sandwich_block3_263_282", (263, 282)), ("sandwich_191_193", (191, 193))):
        out[name] = np.where((idx >= lo) & (idx < hi), 2, 1).astype(np.int64)
    for name, (rcut, b) in (("row_change_43_b171", (43, 171)), ("row_change_5_b200", (5, 200)), ("row_change_126_b129", (126, 129)),
                            ("row_change_203_b300", (203, 300))):
        lab = np.where(idx < b, 1, 2).astype(np.int64)
        lab[:rcut] = 3
        out[name] = lab
    # the rows' cluster changes several times inside the groups above a two-cluster block
    lab = np.where(idx < 215, 1, 2).astype(np.int64)
    lab[:128] = 3 + (idx[:128] // 3) % 2
    out["row_change_every_3_b215"] = lab
    for v in out.values():
        assert v.shape == (n,) and v.min() >= 1 and v.max() <= n
    return out


_references = {}


def _matrices(row, ctx, D, L_host):
    """the fixed-point matrices of this (matrix, storage, exponents): computed once, shared by the rows of a storage"""
    eD, eL = ctx.debug_rowsums(1)[2:4]
    key = (row.data, row.storage, len(D), eD, eL)
    if key not in _references:
        Dq, Lq, _, _ = B.reference_matrices(row, ctx, D, L_host)
        assert np.array_equal(Dq, Dq.T) and np.array_equal(Lq, Lq.T) and not Lq.diagonal().any()
        _references[key] = (Dq, Lq, B.expected_folded(row._replace(fold=1), Dq))
    return _references[key]


@pytest.mark.parametrize("relayout", [True, False], ids=["relayout", "norelayout"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", ROWS, ids=[f"{r.id}-{r.name}" for r in ROWS])
def test_two_cluster_blocks(row, n, relayout):
    D = M.matrix(row.data, n)
    labs = labelings(n)
    ctx, L_host = B.make_context(row, D, relayout=relayout)
    try:
        ctx.set_state(np.ones(n, np.int64))
        Dq, Lq, fold1 = _matrices(row, ctx, D, L_host)
        folded = fold1 and row.fold == 1
        assert folded == (row.id == "01"), (row.id, folded)    # rows 02-*: k_bulk_syml2w under the name of row 01's kernel
        for name, lab in labs.items():
            what = (row.id, n, "relayout" if relayout else "RC_NO_RELAYOUT=1", name)
            ctx.set_state(lab)
            B.check_table(ctx, Dq, Lq, lab, what, ks=np.unique(lab))
            assert ctx.bulk_kernel_name() == row.name, (what, ctx.bulk_kernel_name())
            if row.storage == "derived":
                assert ctx.log_table_folded() == folded, (what, ctx.log_table_folded())
    finally:
        ctx.close()
