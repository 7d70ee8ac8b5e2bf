"""Generates search_refs.npz: what the three integer-criterion search references (psm_search_ref with the Binder loss,
vi_search_ref, id_search_ref) return at a grid of small cases, so that a rewrite of the references — which are what pins
the kernels — is itself pinned (tests/test_search_refs_cpu.py).

  python tests/golden/make_search_refs.py

This generator imports the reference modules, so the committed file says something only if it was produced BEFORE they
were rewritten: it was run at the parent of the commit that moved their loop into greedy_search_ref.py.  Re-running it
later merely records the references against themselves.

Cases: n in {1, 2, 13, 40} x m in {1, 7} x maxK in {0, 2} x maxsweeps in {1, 100} x two starts (empty labels in a shuffled
order; a non-trivial init — unallocated points and two non-adjacent labels — in identity order).  DATA only: the table G
the exact criteria decide on (numpy_G(40); its first n entries are numpy_G(n)), one row of integers per case and the runs'
raw slots end to end.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "search_refs.npz")

NS, MS, MAXKS, MAXSWEEPS = (1, 2, 13, 40), (1, 7), (0, 2), (1, 100)
CRITERIA = ("binder", "vi", "id")
COLUMNS = ("criterion", "n", "m", "maxK", "maxsweeps", "start", "loss_num", "sweeps", "moves", "K", "converged", "raw_at")
SEED = 20261019


def inputs(R, n, m):
    """(samples m×n, counts n×n) of the case: planted_counts with min(3, n) clusters and a 30 % noise share"""
    return R.planted_counts(n, m, min(3, n), 0.3, seed=SEED + 100 * n + m)


def starts(n):
    """[(init, order)]: empty labels in a shuffled order, a non-trivial init in identity order (orders are 1-based)"""
    shuffled = np.random.default_rng(SEED + n).permutation(n) + 1
    init = np.array([(0, n, max(n // 2, 1))[j % 3] for j in range(n)], np.int64) if n > 1 else np.ones(1, np.int64)
    return [(np.zeros(n, np.int64), shuffled), (init, np.arange(1, n + 1))]


def cases():
    for n in NS:
        for m in MS:
            for maxK in MAXKS:
                for maxsweeps in MAXSWEEPS:
                    for start in range(2):
                        yield n, m, maxK, maxsweeps, start


def run(mods, G, crit, n, m, maxK, maxsweeps, start):
    """the reference's dict for one case; mods = (psm_search_ref, vi_search_ref, id_search_ref) modules"""
    R, V, I = mods
    samples, counts = inputs(R, n, m)
    init, order = starts(n)[start]
    if crit == 0:
        return R.psm_search_ref(counts, m, R.BINDER, init, order, maxK=maxK, maxsweeps=maxsweeps)
    fn = V.vi_search_ref if crit == 1 else I.id_search_ref
    return fn(samples, G[:n], init, order, maxK=maxK, maxsweeps=maxsweeps)


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import id_search_ref as I
    import psm_search_ref as R
    import vi_search_ref as V
    G = V.numpy_G(max(NS))
    rows, raw = [], []
    for crit in range(len(CRITERIA)):
        for case in cases():
            o = run((R, V, I), G, crit, *case)
            rows.append([crit, *case, int(o["loss_num"]), o["sweeps"], o["moves"], o["K"], int(o["converged"]), sum(map(len, raw))])
            raw.append(np.asarray(o["raw"], np.int16))
    np.savez_compressed(OUT, G=G, columns=np.array(COLUMNS), cases=np.array(rows, np.int64), raw=np.concatenate(raw))
    print(OUT, len(rows), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
