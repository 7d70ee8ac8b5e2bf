"""Kernel and wall time of the hierarchical point estimates (rc_hclust, rc_psm_expected_loss; csrc/hclust.inc.hip) and, for
scale, of the host tools they replace: scipy.cluster.hierarchy.linkage on the same matrix (when SciPy is installed) and
NumPy's expectedloss for one labelling.

    python tools/time_hclust.py                    # n = 2000 and 8192, median of 5 repetitions
    python tools/time_hclust.py --n 2000 --reps 7
    python tools/time_hclust.py --no-host          # skip SciPy and NumPy

Inputs: a planted partition with K = 50 clusters, 20 % of the points relabelled at random in each of m = 1000 samples
(seed 0); the counts are built on the device (rc_samples_counts) and handed to the timed calls as a host matrix, so every
wall time includes the copy of the n×n counts to the device.  Timed: each linkage (_lib.hclust: kernel_ms is the device time
of the initialisation and linkage kernels), hclustpointestimate end to end (average linkage, "VI": the linkage, ⌈n/8⌉ cuts
derived on the host and evaluated on the device, the cut), and the batched expected loss of those ⌈n/8⌉ cuts.  There is no
reference to compare with at n = 8192; there the Binder curve of the linkage is checked at a handful of cuts against
expectedlosses(…, "binder")'s numerators, which come from an independent kernel.  One JSON line per measurement."""
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

LINKAGES = {"average": 0, "complete": 1, "single": 2}


def planted_samples(n, m, K, noise, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, size=n)
    samples = np.tile(truth, (m, 1))
    flip = rng.random((m, n)) < noise
    samples[flip] = rng.integers(0, K, size=int(flip.sum()))
    return samples.astype(np.int64) + 1


def timed(reps, fn):
    """wall seconds and result of every repetition"""
    walls, outs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        outs.append(fn())
        walls.append(time.perf_counter() - t0)
    return walls, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2000, 8192])
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    warm = _lib.samples_counts(planted_samples(64, 5, 3, 0.1))[0]
    for l in LINKAGES.values():
        _lib.hclust(warm, 5, l, maxcut=8)                                   # module load, first launches
    for n in a.n:
        S = planted_samples(n, a.m, a.K, a.noise)
        C = _lib.samples_counts(S)[0]
        runs = {}
        for name, l in LINKAGES.items():
            walls, outs = timed(a.reps, lambda: _lib.hclust(C, a.m, l))
            kms, runs[name] = [o["kernel_ms"] for o in outs], outs[-1]
            print(json.dumps(dict(what="linkage", linkage=name, n=n, m=a.m, reps=a.reps,
                                  kernel_ms_median=round(statistics.median(kms), 3), kernel_ms_min=round(min(kms), 3),
                                  kernel_ms_max=round(max(kms), 3), us_per_step=round(1e3 * statistics.median(kms) / max(n - 1, 1), 3),
                                  wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4))), flush=True)
        walls, outs = timed(a.reps, lambda: rc.hclustpointestimate(C, "VI", "average", numsamples=a.m))
        info = outs[-1][1]
        print(json.dumps(dict(what="hclustpointestimate", loss="VI", linkage="average", n=n, m=a.m, cuts=len(info["loss"]),
                              K=info["K"], loss_of_cut=float(info["loss"][info["K"] - 1]), kernel_ms=round(info["kernel_ms"], 3),
                              wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4))), flush=True)
        ncut = -(-n // 8)
        mg = runs["average"]["merges"]
        labs = np.stack([_lib.hclust_cut(mg, n, K) for K in range(1, ncut + 1)])
        for loss, code in (("binder", 0), ("VI", 1)):
            walls, outs = timed(a.reps, lambda: _lib.psm_expected_loss(labs, C, a.m, code))
            kms, out = [o[2] for o in outs], outs[-1]
            print(json.dumps(dict(what="expectedlosses", loss=loss, n=n, m=a.m, labellings=ncut,
                                  kernel_ms_median=round(statistics.median(kms), 3), kernel_ms_min=round(min(kms), 3),
                                  wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4))), flush=True)
            if loss == "binder":
                # the linkage's Binder curve against the independent kernel, at a handful of cuts
                ks = sorted({1, 2, a.K, ncut // 2, ncut})
                agree = all(int(out[1][K - 1]) == int(runs["average"]["binder_num"][n - K]) for K in ks)
                print(json.dumps(dict(what="check", n=n, cuts=ks, binder_curve_equals_expectedlosses=bool(agree),
                                      num=[int(out[1][K - 1]) for K in ks])), flush=True)
        if a.no_host:
            continue
        t0 = time.perf_counter()
        ref = rc.expectedloss(labs[info["K"] - 1], C, a.m, "VI")
        t_np = time.perf_counter() - t0
        print(json.dumps(dict(what="numpy expectedloss", loss="VI", n=n, labellings=1, wall_s=round(t_np, 4),
                              abs_diff_to_device=abs(ref - float(info["loss"][info["K"] - 1])))), flush=True)
        try:
            from scipy.cluster.hierarchy import linkage
            from scipy.spatial.distance import squareform
        except ImportError:
            print(json.dumps(dict(what="scipy linkage", n=n, skipped="SciPy is not installed")), flush=True)
            continue
        D = 1.0 - C.astype(np.float64) / a.m
        np.fill_diagonal(D, 0.0)
        y = squareform(D, checks=False)
        for name in LINKAGES:
            t0 = time.perf_counter()
            Z = linkage(y, name)
            t_sp = time.perf_counter() - t0
            ours = rc.linkage_matrix(runs[name]["merges"], a.m, name)[:, 2]
            print(json.dumps(dict(what="scipy linkage", linkage=name, n=n, wall_s=round(t_sp, 4),
                                  heights_equal_as_multiset=bool(np.allclose(np.sort(Z[:, 2]), np.sort(ours), rtol=0, atol=1e-12)))),
                  flush=True)


if __name__ == "__main__":
    main()
