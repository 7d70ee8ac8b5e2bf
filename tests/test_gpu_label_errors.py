"""Every entry point that takes a label matrix names the first label outside 1..n the same way: RC_ERR_ARG with the row and the
position (csrc/hostutil.inc.hip, check_label_rows).  n = 8, m = 3; the label of sample 2 at position 3 is n + 1 or 0."""
import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

N, M = 8, 3
GOOD = np.array([[1, 1, 2, 2, 3, 3, 8, 8], [5, 5, 5, 5, 1, 1, 1, 1], [1, 2, 3, 4, 5, 6, 7, 8]], np.int64)
COUNTS = (GOOD[:, :, None] == GOOD[:, None, :]).sum(axis=0).astype(np.uint32)
INIT, ORDER = np.zeros((1, N), np.int64), np.arange(1, N + 1, dtype=np.int32)[None, :]
PARAMS = dict(delta1=1.0, delta2=1.0, alpha=1.0, beta=1.0, zeta=1.0, gamma=1.0)

ENTRY_POINTS = {
    "loss_matrix": lambda S: _lib.loss_matrix(S, 0),
    "vi_search": lambda S: _lib.vi_search(S, INIT, ORDER),
    "samples_counts": lambda S: _lib.samples_counts(S),
    "predict": lambda S: _lib.predict(np.ones((2, N)), S, np.ones(M), np.full(M, 0.5), PARAMS),
    "psm_expected_loss": lambda S: _lib.psm_expected_loss(S, COUNTS, M, 0),
    "partition_distances-samples": lambda S: _lib.partition_distances(GOOD, S),
    "partition_distances-labellings": lambda S: _lib.partition_distances(S, GOOD),
    "relabel": lambda S: _lib.relabel(S, GOOD[0]),
}


@pytest.mark.parametrize("bad", [N + 1, 0])
@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_the_first_bad_label_is_named_with_its_row_and_position(entry, bad):
    S = GOOD.copy()
    S[1, 2] = bad
    S[2, 0] = bad                                                        # a later offender is not the one reported
    with pytest.raises(rc.RedClustHIPError, match=r"RC_ERR_ARG.*2 at position 3") as e:
        ENTRY_POINTS[entry](S)
    assert e.value.code == -1 and f"label {bad} of" in str(e.value)
