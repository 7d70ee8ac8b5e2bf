"""The four search bindings report a bad run the same way and in the same order of precedence: the host side of the searches
is shared (csrc/greedy.inc.hip), and the texts below are what the library said for these inputs before it was.  n = 5, m = 3,
two runs, the offence in run 2 only.  Within a run the starting labels are read before its order; the argument checks come
before any capacity."""
import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu

N, M = 5, 3
SAMPLES = np.array([[1, 1, 2, 2, 3], [1, 1, 1, 2, 2], [1, 2, 3, 4, 5]], np.int64)
COUNTS = (SAMPLES[:, :, None] == SAMPLES[:, None, :]).sum(axis=0).astype(np.uint32)


def bindings(samples, counts):
    return {
        "psm_search": lambda init, order, **kw: _lib.psm_search(counts, M, 0, init, order, **kw),
        "psm_search_samples": lambda init, order, **kw: _lib.psm_search_samples(samples, 0, init, order, **kw),
        "vi_search": lambda init, order, **kw: _lib.vi_search(samples, init, order, **kw),
        "id_search": lambda init, order, **kw: _lib.id_search(samples, init, order, **kw),
    }


# (a non-permutation order, a label n + 1, maxsweeps = 0) as the library worded them at the parent of the commit that merged
# the host sides: the counts' searches share one driver ("point search"), the exact searches name their entry point
EXPECT = {
    "psm_search": ("RC_ERR_ARG: point search: the order of run 2 is not a permutation of 1..n",
                   "RC_ERR_ARG: point search: label 6 of run 2 outside 0..n",
                   "RC_ERR_ARG: rc_psm_search: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)"),
    "psm_search_samples": ("RC_ERR_ARG: point search: the order of run 2 is not a permutation of 1..n",
                           "RC_ERR_ARG: point search: label 6 of run 2 outside 0..n",
                           "RC_ERR_ARG: rc_psm_search_samples: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)"),
    "vi_search": ("RC_ERR_ARG: rc_vi_search: the order of run 2 is not a permutation of 1..n",
                  "RC_ERR_ARG: rc_vi_search: label 6 of run 2 outside 0..n",
                  "RC_ERR_ARG: rc_vi_search: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)"),
    "id_search": ("RC_ERR_ARG: rc_id_search: the order of run 2 is not a permutation of 1..n",
                  "RC_ERR_ARG: rc_id_search: label 6 of run 2 outside 0..n",
                  "RC_ERR_ARG: rc_id_search: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)"),
}


def runs(bad_order=False, bad_label=False):
    init, order = np.zeros((2, N), np.int64), np.tile(np.arange(1, N + 1, dtype=np.int32), (2, 1))
    if bad_order:
        order[1] = [1, 2, 2, 4, 5]
    if bad_label:
        init[1, 3] = N + 1
    return init, order


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_errors_of_a_run_keep_their_text_and_precedence(name):
    call = bindings(SAMPLES, COUNTS)[name]
    bad_order, bad_label, _ = EXPECT[name]
    for kw, text in ((dict(bad_order=True), bad_order), (dict(bad_label=True), bad_label),
                     (dict(bad_order=True, bad_label=True), bad_label)):
        with pytest.raises(rc.RedClustHIPError) as e:
            call(*runs(**kw))
        assert type(e.value) is rc.RedClustHIPError and e.value.code == -1
        assert str(e.value) == text, kw
    # a valid call afterwards still succeeds
    out = call(*runs())
    want = [1, 1, 2, 2, 3] if name == "id_search" else [1, 1, 2, 3, 4]
    assert out["labels"].tolist() == [want, want] and out["best"] == 0


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_maxsweeps_is_checked_before_the_capacity_in_n(name):
    W = 8193                                                             # one past the searches' capacity; all-zero inputs
    call = bindings(np.zeros((M, W), np.int64), np.zeros((W, W), np.uint32))[name]
    with pytest.raises(rc.RedClustHIPError) as e:
        call(np.zeros((2, W), np.int64), np.zeros((2, W), np.int32), maxsweeps=0)
    assert type(e.value) is rc.RedClustHIPError and e.value.code == -1
    assert str(e.value) == EXPECT[name][2]
    out = bindings(SAMPLES, COUNTS)[name](*runs())
    assert out["converged"].all()
