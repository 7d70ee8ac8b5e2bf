"""Kernel and wall time of the cluster profiles (rc_cluster_profiles; csrc/profile.inc.hip) and, for scale, of the route there
was before: the n×n matrix pulled back to the host and the definitions evaluated in NumPy (tests/profiles_ref.py, the reference
the tests compare with — `Dq @ membership` for the sums, Python integers for the comparison).

    python tools/time_profiles.py                     # both cases, median of 5 repetitions after a warm-up
    python tools/time_profiles.py --reps 3 --n 8192 --m 1000 --cuts 1024

Cases (seed 0, those of tools/time_score.py), n = 8192 points in 3 dimensions around 50 centres (from_points): "samples" — m =
1000 labellings, the planted partition of 50 clusters with 20 % of the points relabelled at random in each; "cuts" — the K =
1..1024 cuts of the average-linkage dendrogram of those samples.  kernel_ms is the device time of the call's kernels; the wall
time adds the host's part: the label check, the sorted orders and the copies of the L×n results (and, in the clusterprofiles
line, the silhouettes in float64 on the host).  "medoids only" is the call without per-point outputs.  The reference is timed
on --ref-labellings labellings (2 by default) and extrapolated linearly to the whole batch, which is said in its line — for the
samples spread evenly over the batch; for the cuts on those of --ref-cut-K clusters (16 and 64 by default), because its integer
matrix product grows faster than linearly in K: that extrapolation is a lower bound.  Its integers must equal the device's.
The matrix read-back is timed once and reported apart.  One JSON line per measurement."""
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
import profiles_ref as R  # noqa: E402
from score_ref import quantised  # noqa: E402
from time_hclust import planted_samples, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--cuts", type=int, default=1024)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-labellings", type=int, default=2)
    ap.add_argument("--ref-cut-K", type=int, nargs="*", default=[16, 64])
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    truth = planted_samples(a.n, 1, a.K, 0.0)[0]
    X = rng.normal(0, 6, (a.K, 3))[truth - 1] + rng.normal(0, 1, (a.n, 3))
    S = planted_samples(a.n, a.m, a.K, a.noise)
    ctx = rc.Context.from_points(X)
    ctx.profiles(S[:2])                                                    # first launches
    t0 = time.perf_counter()
    Dq = quantised(ctx.get_matrix(0), ctx.profiles(S[:1], points=False)["eD"])
    print(json.dumps(dict(what="matrix read-back and quantised integers", n=a.n, wall_s=round(time.perf_counter() - t0, 2))), flush=True)
    cases = [("samples", S, np.unique(np.linspace(0, a.m - 1, min(a.m, a.ref_labellings)).astype(int)))]
    if a.cuts > 0:
        h = _lib.hclust(None, a.m, 0, samples=S)
        cuts = np.stack([_lib.hclust_cut(h["merges"], a.n, K) for K in range(1, a.cuts + 1)])
        cases.append(("cuts", cuts, np.array([K - 1 for K in a.ref_cut_K if 1 <= K <= a.cuts], dtype=int)))
    for case, labs, pick in cases:
        L = len(labs)
        ctx.profiles(labs[:: max(L // 8, 1)])                              # warm-up at this shape
        walls, outs = timed(a.reps, lambda: ctx.profiles(labs))
        kms = [o["kernel_ms"] for o in outs]
        dev_wall = statistics.median(walls)
        print(json.dumps(dict(what="profiles", case=case, n=a.n, L=L, K_max=int(outs[-1]["K"].max()), reps=a.reps,
                              kernel_ms_median=round(statistics.median(kms), 2), kernel_ms_min=round(min(kms), 2),
                              kernel_ms_max=round(max(kms), 2), us_per_labelling=round(1e3 * statistics.median(kms) / L, 1),
                              wall_s_median=round(dev_wall, 3), wall_s_min=round(min(walls), 3))), flush=True)
        walls_m, outs_m = timed(a.reps, lambda: ctx.profiles(labs, points=False))
        print(json.dumps(dict(what="profiles, medoids only", case=case, L=L,
                              kernel_ms_median=round(statistics.median([o["kernel_ms"] for o in outs_m]), 2),
                              wall_s_median=round(statistics.median(walls_m), 3))), flush=True)
        walls_c, _ = timed(max(a.reps // 2, 1), lambda: rc.clusterprofiles(ctx, labs))
        print(json.dumps(dict(what="clusterprofiles (with the silhouettes on the host)", case=case, L=L,
                              wall_s_median=round(statistics.median(walls_c), 3))), flush=True)
        if len(pick):
            t0 = time.perf_counter()
            refs = [R.profile(Dq, labs[l]) for l in pick]
            t_ref = time.perf_counter() - t0
            same = all(R.mismatches(outs[-1], int(l), ref) == [] for l, ref in zip(pick, refs))
            print(json.dumps(dict(what="NumPy reference per labelling", case=case, labellings_timed=len(pick),
                                  K_timed=[int(outs[-1]["K"][l]) for l in pick], wall_s=round(t_ref, 2), extrapolated_to_labellings=L,
                                  extrapolated_wall_s=round(t_ref / len(pick) * L, 1), lower_bound=case == "cuts",
                                  profiles_wall_s_median=round(dev_wall, 3), speedup=round(t_ref / len(pick) * L / dev_wall, 1),
                                  same_integers=bool(same))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
