"""Kernel time of the PEAR search (rc_pear_search, csrc/pointsearch.inc.hip) next to the Binder search's on the same counts,
the two alternating in one process, and the PEAR of the result against the best sample's and the best average-linkage cut's.

    python tools/time_pearsearch.py                   # n = 8192, m = 1000, K = 50, 16 runs, 7 repetitions of each
    python tools/time_pearsearch.py --n 2000 --reps 5 --no-quality
    python tools/time_pearsearch.py --maxsweeps 1 --no-quality   # with the default: time per sweep and time outside the sweeps
    python tools/time_pearsearch.py --psm-only        # Binder and the VI bound only: for comparing two builds of the library
                                                      # (RC_LIB_PATH selects the build), alternating processes

Inputs: a planted partition with K clusters, `noise` of the points relabelled at random in each of m samples (seed 0); the
counts are built from the samples on the device (rc_samples_counts).  Runs: the nruns Philox orders of searchpointestimate
(seed 0) from empty labels, the same for both searches.  One JSON line per measurement."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redclust_amd as rc  # noqa: E402
from redclust_amd import _lib  # noqa: E402
from redclust_amd.pointestimate import _search_starts  # noqa: E402


def planted_samples(n, m, K, noise, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(1, K + 1, size=n)
    samples = np.tile(truth, (m, 1)).astype(np.int64)
    flip = rng.random((m, n)) < noise
    samples[flip] = rng.integers(1, K + 1, size=int(flip.sum()))
    return samples


def stats(ms):
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--nruns", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--maxsweeps", type=int, default=100)
    ap.add_argument("--psm-only", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    a = ap.parse_args()
    S = planted_samples(a.n, a.m, a.K, a.noise)
    C, counts_ms = _lib.samples_counts(S)
    inits, orders = _search_starts(a.n, a.nruns, 0, None)
    base = dict(n=a.n, m=a.m, K=a.K, nruns=a.nruns, reps=a.reps, maxsweeps=a.maxsweeps, lib=os.path.basename(_lib.SO))
    searches = {"binder": lambda: _lib.psm_search(C, a.m, 0, inits, orders, maxsweeps=a.maxsweeps)}
    if a.psm_only:
        searches["VI"] = lambda: _lib.psm_search(C, a.m, 1, inits, orders, maxsweeps=a.maxsweeps)
    else:
        searches["PEAR"] = lambda: _lib.pear_search(C, a.m, inits, orders, maxsweeps=a.maxsweeps)
    for f in searches.values():                                      # module load, first launches, clocks
        f()
    ms, last = {k: [] for k in searches}, {}
    for _ in range(a.reps):                                          # alternating
        for k, f in searches.items():
            last[k] = f()
            ms[k].append(last[k]["kernel_ms"])
    for k in searches:
        r = last[k]
        print(json.dumps(dict(base, what=k, kernel_ms=stats(ms[k]), kernel_ms_all=[round(x, 3) for x in ms[k]],
                              labels_sha=hashlib.sha256(np.ascontiguousarray(r["labels"]).tobytes()).hexdigest()[:16],
                              sweeps=[int(x) for x in r["sweeps"]], converged=int(r["converged"].sum()), K=[int(x) for x in r["K"]])),
              flush=True)
    if a.psm_only:
        return
    ratio = statistics.median(ms["PEAR"]) / statistics.median(ms["binder"])
    print(json.dumps(dict(base, what="PEAR/binder", kernel_ms_ratio=round(ratio, 3), counts_ms=round(counts_ms, 3))), flush=True)
    if a.no_quality:
        return
    r = last["PEAR"]
    best = r["best"]

    class Result:
        clusts = list(S)

    _, draws = rc.maxpear(Result, "draws")
    _, avg = rc.maxpear(C, "avg", numsamples=a.m)
    ari = rc.expectedari(np.stack([r["labels"][best], last["binder"]["labels"][last["binder"]["best"]]]), S)
    print(json.dumps(dict(base, what="quality", pear_search=float(r["pear"][best]), K_search=int(r["K"][best]),
                          pear_best_sample=draws["pear"], pear_best_avg_cut=avg["pear"], K_avg_cut=avg["avg"]["K"],
                          expected_ari_of_pear_result=float(ari[0]), expected_ari_of_binder_result=float(ari[1]),
                          pear_of_binder_result=rc.expectedpears(last["binder"]["labels"][last["binder"]["best"]], C, a.m)[0].tolist())),
          flush=True)


if __name__ == "__main__":
    main()
