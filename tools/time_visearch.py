"""Wall and kernel time of the exact expected-VI search (rc_vi_search, csrc/visearch.inc.hip) — or, with --loss ID, of the
exact expected-ID search (rc_id_search, the same kernel) — and, at n = 2000, of the NumPy restatement (tests/vi_search_ref.py,
tests/id_search_ref.py) doing ONE run's work on the host — the only yardstick there is: the reference has no such search.

    python tools/time_visearch.py                  # n = 2000 and 8192, 16 runs, median of 5 repetitions
    python tools/time_visearch.py --n 2000 --reps 7
    python tools/time_visearch.py --no-ref         # skip the NumPy restatement
    python tools/time_visearch.py --loss ID        # the same input through rc_id_search
    python tools/time_visearch.py --maxsweeps 1    # the first sweep alone (sequential allocation: every point moves)

Inputs: a planted partition with K = 50 clusters, 20 % of the points relabelled at random in each of m = 1000 samples
(seed 0).  The timed call is _lib.vi_search (_lib.id_search) with 16 runs from empty labels in the orders searchpointestimate draws
(Philox, key 0): the wall time includes the host's re-labelling and transposition of the samples, the copies and the
zeroing of the tables.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import redclust_amd as rc  # noqa: E402
from redclust_amd import _lib  # noqa: E402


def planted_samples(n, m, K, noise, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, size=n)
    samples = np.tile(truth, (m, 1))
    flip = rng.random((m, n)) < noise
    samples[flip] = rng.integers(0, K, size=int(flip.sum()))
    return samples.astype(np.int64) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2000, 8192])
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--nruns", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--loss", choices=["VI", "ID"], default="VI")
    ap.add_argument("--maxsweeps", type=int, default=100)
    a = ap.parse_args()
    search = _lib.vi_search if a.loss == "VI" else _lib.id_search
    expected = rc.expectedvi if a.loss == "VI" else rc.expectedid
    warm = planted_samples(64, 5, 3, 0.1)
    search(warm, np.zeros((2, 64), np.int64), np.tile(np.arange(1, 65, dtype=np.int32), (2, 1)))   # module load, first launch
    for n in a.n:
        S = planted_samples(n, a.m, a.K, a.noise)
        rng = np.random.Generator(np.random.Philox(key=0))
        order = np.stack([rng.permutation(n).astype(np.int32) + 1 for _ in range(a.nruns)])
        init = np.zeros((a.nruns, n), np.int64)
        walls, kms, res = [], [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = search(S, init, order, maxsweeps=a.maxsweeps)
            walls.append(time.perf_counter() - t0)
            kms.append(res["kernel_ms"])
        sw = res["sweeps"]
        best = res["labels"][res["best"]]
        print(json.dumps(dict(what="device", loss=a.loss, maxsweeps=a.maxsweeps, n=n, m=a.m, nruns=a.nruns, reps=a.reps,
                              wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4),
                              wall_s_max=round(max(walls), 4), kernel_ms_median=round(statistics.median(kms), 3),
                              kernel_ms_min=round(min(kms), 3), kernel_ms_max=round(max(kms), 3),
                              sweeps=[int(x) for x in sw], converged=int(res["converged"].sum()), K=[int(x) for x in res["K"]],
                              best_loss=float(res["loss"][res["best"]]), **{f"expected{a.loss.lower()}_of_best": expected(best, S)},
                              us_per_step=round(1e3 * statistics.median(kms) / (n * int(sw.max())), 3),
                              table_reads_per_step=a.m * a.K)), flush=True)
        if n <= 2000 and not a.no_ref:
            import id_search_ref
            import vi_search_ref
            run_ref = vi_search_ref.vi_search_ref if a.loss == "VI" else id_search_ref.id_search_ref
            G = _lib.vi_gtable(n)
            t0 = time.perf_counter()
            ref = run_ref(S, G, init[0], order[0], maxsweeps=a.maxsweeps)
            t_ref = time.perf_counter() - t0
            same = bool(np.array_equal(ref["labels"], res["labels"][0]) and ref["loss_num"] == int(res["loss_num"][0]))
            print(json.dumps(dict(what="numpy_ref_one_run", loss=a.loss, n=n, wall_s=round(t_ref, 3), sweeps=ref["sweeps"], K=ref["K"],
                                  equals_device_run0=same)), flush=True)


if __name__ == "__main__":
    main()
