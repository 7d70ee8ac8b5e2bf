"""rc_relabel_wide on the device against the NumPy restatement (relabel_ref.py), bit for bit — every output is an integer — and,
where rc_relabel accepts the input, against rc_relabel.  The cases stand where k_relabel_wide can go wrong: the columns a thread
owns (1 + t + 1024·k, k < 4) at 1023 … 4096 columns, both orientations above 1024 clusters, a table of zeros and ones in which
the smallest-column rule decides the matching, cells of 32767 and row offsets near 32767, and chunks of one sample."""
import functools

import numpy as np
import pytest

import relabel_ref as RL
import test_gpu_relabel as G
import redclust_amd as rc
from redclust_amd import _lib

pytestmark = pytest.mark.gpu


def _columns(C):
    """C sample clusters against a pivot of 7: the pivot's clusters are the rows"""
    return np.stack([G._wide(C + 300, C, C)]), G._wide(C + 300, 7, C + 1)


def _blocks(K=1100, b=25):
    """test_gpu_relabel's _ties at K clusters a side, every cell 0 or 1: K / b diagonal blocks of b × b ones (n <= 32767 has no
    room for a full table of ones), the second sample with its clusters in reverse order; within a block every step is a tie"""
    blk, r = np.divmod(np.arange(K * b), b * b)
    k, t = np.divmod(r, b)
    return np.stack([blk * b + t + 1, K - blk * b - t]).astype(np.int64), (blk * b + k + 1).astype(np.int64)


CASES = {
    # where both kernels run
    "n1": G.CASES["n1"], "n63": G.CASES["n63"], "n64": G.CASES["n64"], "n65": G.CASES["n65"],
    "kp1024-vs-singletons": G.CASES["kp1024-vs-singletons"],
    "c1023": lambda: _columns(1023), "c1024": lambda: _columns(1024),
    "n32767-one-cell": G.CASES["n32767"],
    # above rc_relabel's limit: the column-ownership edges (at 4096: K_s = 4096 against K_p = 7) ...
    "c1025": lambda: _columns(1025), "c2048": lambda: _columns(2048), "c2049": lambda: _columns(2049), "c4096": lambda: _columns(4096),
    # ... both orientations, square tables ...
    "kp1025-vs-16-and-1025": lambda: (np.stack([G._wide(3000, 16, 11), G._wide(3000, 1025, 12)]), G._wide(3000, 1025, 13)),
    "kp4096-vs-3": lambda: (np.stack([G._wide(4400, 3, 14)]), G._wide(4400, 4096, 15)),
    "singletons4096": lambda: (np.stack([np.random.default_rng(16).permutation(4096) + 1, np.arange(1, 4097)]).astype(np.int64),
                               (np.random.default_rng(17).permutation(4096) + 1).astype(np.int64)),
    # ... ties, and the 16-bit row offsets with 4096 rows' worth of columns
    "ties1100": _blocks,
    "n32767-kp4096-vs-3": lambda: (np.stack([G._wide(32767, 3, 18)]), G._wide(32767, 4096, 19)),
}
CHUNKED = ("kp1025-vs-16-and-1025",)                                # again with a workspace of 1 KiB: chunks of one sample


@functools.lru_cache(maxsize=None)
def problem(name):
    """(samples, pivot, reference outputs, largest cluster count) of a case; computed once and shared (never modified)"""
    S, c = CASES[name]()
    S, c = np.ascontiguousarray(S, np.int64), np.ascontiguousarray(c, np.int64)
    ref = RL.relabel_ref(S, c)
    for a in (S, c) + tuple(ref.values()):
        a.setflags(write=False)
    return S, c, ref, max(len(ref["pivot_labels"]), ref["maps"].shape[1])


@pytest.mark.parametrize("name,kib", [(k, None) for k in CASES] + [(k, "1") for k in CHUNKED])
def test_every_output_equals_the_reference_bit_for_bit(name, kib, monkeypatch):
    S, c, ref, K = problem(name)
    if kib:
        monkeypatch.setenv("RC_RELABEL_WORKSPACE_KIB", kib)
    got = _lib.relabel_wide(S, c)
    print(name, "K", K, "kernel_ms", got["kernel_ms"])
    G.assert_equals_reference(got, ref, S, c)
    if K <= 1024:
        old = _lib.relabel(S, c)
        for key in ("labels", "maps", "overlap", "counts"):
            assert np.array_equal(got[key], old[key]), key
    else:
        with pytest.raises(rc.RedClustHIPError, match="RC_ERR_CAPACITY"):
            _lib.relabel(S, c)


def test_capacity_and_the_public_surface():
    wide, one = np.arange(1, 4098, dtype=np.int64), np.ones(4097, np.int64)
    with pytest.raises(rc.RedClustHIPError, match="rc_relabel_wide: the pivot has 4097 clusters, more than 4096"):
        _lib.relabel_wide(one[None, :], wide)
    with pytest.raises(rc.RedClustHIPError, match="rc_relabel_wide: sample 2 has 4097 clusters, more than 4096"):
        _lib.relabel_wide(np.stack([one, wide]), one)
    S, c, ref, _ = problem("kp1025-vs-16-and-1025")
    rel = rc.relabel_wide(S, c)
    assert isinstance(rel, rc.Relabelling)
    for key in ("labels", "maps", "overlap", "counts", "pivot_labels"):
        assert np.array_equal(getattr(rel, key), ref[key]), key
    pr = rel.probabilities()
    assert pr.shape == (3000, 1026) and np.allclose(pr.sum(1), 1.0)
    S, c, ref, _ = problem("n65")                                    # at most 1024 clusters: relabel's call and arrays
    rel, old = rc.relabel_wide(S, c), rc.relabel(S, c)
    for key in ("labels", "maps", "overlap", "counts", "pivot_labels"):
        assert np.array_equal(getattr(rel, key), getattr(old, key)) and np.array_equal(getattr(rel, key), ref[key]), key
