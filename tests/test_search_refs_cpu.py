"""The NumPy search references reproduce tests/golden/search_refs.npz exactly: the file was recorded from the three
references as they stood before their loop was shared (tests/golden/make_search_refs.py), so a change to
greedy_search_ref.py that alters a trajectory of an integer criterion fails here, without a GPU."""
import importlib.util
import os

import numpy as np
import pytest

import id_search_ref as I
import psm_search_ref as R
import vi_search_ref as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_search_refs", os.path.join(GOLDEN, "make_search_refs.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "search_refs.npz"))


def test_grid_is_the_recorded_one(golden):
    assert tuple(golden["columns"]) == M.COLUMNS
    want = [[crit, *case] for crit in range(len(M.CRITERIA)) for case in M.cases()]
    assert golden["cases"][:, :6].tolist() == want
    assert len(want) == 3 * 4 * 2 * 2 * 2 * 2


@pytest.mark.parametrize("crit", range(3), ids=M.CRITERIA)
def test_references_reproduce_the_recorded_runs(golden, crit):
    G, raw = golden["G"], golden["raw"]
    assert np.abs(G - V.numpy_G(len(G))).max() <= 1    # one rounding of this host's logarithm; the runs are handed the recorded table
    rows = [r for r in golden["cases"].tolist() if r[0] == crit]
    assert len(rows) == 64
    for row in rows:
        c = dict(zip(M.COLUMNS, row))
        o = M.run((R, V, I), G, crit, c["n"], c["m"], c["maxK"], c["maxsweeps"], c["start"])
        got = (int(o["loss_num"]), o["sweeps"], o["moves"], o["K"], int(o["converged"]))
        assert got == (c["loss_num"], c["sweeps"], c["moves"], c["K"], c["converged"]), c
        assert np.array_equal(o["raw"], raw[c["raw_at"]:c["raw_at"] + c["n"]]), c
        assert np.array_equal(o["labels"], R.sortlabels(o["raw"])), c
