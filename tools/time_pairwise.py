"""Times of the metrics from coordinates (csrc/metric.inc.hip, predictpoints.inc.hip, pairwise.inc.hip) on a planted mixture in
dim = 50:

    python tools/time_pairwise.py                          # everything below
    python tools/time_pairwise.py --sizes 8192 --reps 3    # the smaller size only
    python tools/time_pairwise.py --no-contexts --no-predict

  * per n of --sizes (default 8192 32768) and per metric: the kernel time of rc_pairwise's symmetric form (device events around
    the pre-pass and k_pairwise_metric; the n² doubles then cross the bus, which the wall time shows);
  * per n: the whole Context.from_points call with metric=None (k_pairwise, the Gram form) beside each metric — 64-bit storage
    up to n = 8192, 32-bit above, as the benchmark's HBM-resident configuration has it;
  * at n = 8192 only: the host's NumPy evaluation of the same matrix (MCMCData(points, metric=...).D);
  * predict_points at n = 8192, m = 1000 samples, q = 1024 new points: the kernel time per metric beside the Euclidean call of
    the same process.

Inputs (seed 0): K = 50 Gaussian groups, centres 4·N(0, I), unit noise.  Every figure is the minimum and the median over --reps
calls after one call at the timed shape.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redclust_amd as rc  # noqa: E402
from redclust_amd import _lib  # noqa: E402

DIM = 50


def planted(n, K=50, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, size=n)
    return np.ascontiguousarray(4.0 * rng.standard_normal((K, DIM))[truth] + rng.standard_normal((n, DIM))), truth


def stats(xs, digits=3):
    return dict(min=round(min(xs), digits), median=round(statistics.median(xs), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-contexts", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-predict", action="store_true")
    a = ap.parse_args()
    rc.pairwise(planted(64)[0], metric="cosine")                    # module load, first launches
    for n in a.sizes:
        X, _ = planted(n)
        for metric in rc.METRICS:
            _lib.pairwise(X, metric=metric)                         # first call at the timed shape
            kms, walls = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, ms = _lib.pairwise(X, metric=metric, want_ms=True)
                walls.append(time.perf_counter() - t0)
                kms.append(ms)
            print(json.dumps(dict(what="rc_pairwise, symmetric", n=n, dim=DIM, metric=metric, reps=a.reps, kernel_ms=stats(kms),
                                  store_gb_per_s=round(8.0 * n * n / (min(kms) * 1e-3) / 1e9, 1), wall_s=stats(walls, 4))), flush=True)
        if not a.no_contexts:
            bits = 64 if n <= 8192 else 32
            for metric in (None, *rc.METRICS):
                rc.Context.from_points(X, metric=metric, storage_bits=bits).close()
                walls = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ctx = rc.Context.from_points(X, metric=metric, storage_bits=bits)
                    walls.append(time.perf_counter() - t0)
                    ctx.close()
                print(json.dumps(dict(what="Context.from_points", n=n, dim=DIM, storage_bits=bits, metric=metric, reps=a.reps,
                                      wall_s=stats(walls, 4))), flush=True)
        if not a.no_host and n <= 8192:
            for metric in rc.METRICS:
                t0 = time.perf_counter()
                D = rc.MCMCData(X, metric=metric).D
                print(json.dumps(dict(what="host NumPy matrix", n=n, dim=DIM, metric=metric, wall_s=round(time.perf_counter() - t0, 3),
                                      shape=list(D.shape))), flush=True)
    if a.no_predict:
        return
    n, m, q = 8192, 1000, 1024
    X, truth = planted(n + q)
    tr, new = X[:n], X[n:]
    rng = np.random.default_rng(1)
    S = np.tile(truth[:n], (m, 1))
    flip = rng.random((m, n)) < 0.02
    S[flip] = rng.integers(0, 50, size=int(flip.sum()))
    S = S.astype(np.int64) + 1
    r, p = rng.uniform(0.5, 3.0, m), rng.uniform(0.2, 0.8, m)
    sub = rc.pairwise(tr[:1024], metric="euclidean")
    P = rc.likelihood_hyperparams(sub, truth[:1024] + 1)
    for metric in rc.METRICS:                                       # the distance kernel by itself: rc_pairwise's q×n form
        _lib.pairwise(tr, new, metric=metric)
        kms = [_lib.pairwise(tr, new, metric=metric, want_ms=True)[1] for _ in range(a.reps)]
        print(json.dumps(dict(what="rc_pairwise, new against training points", n=n, dim=DIM, q=q, metric=metric, reps=a.reps,
                              kernel_ms=stats(kms, 4))), flush=True)
    for metric in (None, *rc.METRICS):
        _lib.predict_points(tr, new, S, r, p, P, metric=metric)
        kms, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            o = _lib.predict_points(tr, new, S, r, p, P, metric=metric)
            walls.append(time.perf_counter() - t0)
            kms.append(o["kernel_ms"])
        print(json.dumps(dict(what="predict_points", n=n, dim=DIM, m=m, q=q, metric=metric, reps=a.reps, kernel_ms=stats(kms),
                              wall_s=stats(walls, 4))), flush=True)


if __name__ == "__main__":
    main()
