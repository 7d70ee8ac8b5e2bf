"""Kernel and wall time of scoring labellings (rc_score_labellings; csrc/score.inc.hip) and, for scale, of the only other route to
a log-likelihood: Context.set_state + Context.loglik, one labelling at a time on the same context.

    python tools/time_score.py                     # both cases, median of 5 repetitions after a warm-up
    python tools/time_score.py --reps 3 --n 8192 --m 1000 --cuts 1024

Cases (seed 0), n = 8192 points in 3 dimensions around 50 centres (from_points: the distances are computed on the device, the
logarithms derived): "samples" — m = 1000 labellings, the planted partition of 50 clusters with 20 % of the points relabelled at
random in each; "cuts" — the K = 1..1024 cuts of the average-linkage dendrogram of those samples.  kernel_ms is the device time
of the call's kernels; the wall time adds the host's part: the label check, the sorted orders, the copies and the scalar part
of every log-likelihood in long double (K(K+1)/2 terms per labelling: at K = 1024 that is the larger share).  The set_state +
loglik route is timed on --route-labellings labellings (20 by default) spread evenly over the batch, after one untimed call,
and extrapolated linearly to the whole batch, which is said in its line; its values must equal the scores bit for bit.  One JSON
line per measurement."""
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
from time_hclust import planted_samples, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--cuts", type=int, default=1024)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route-labellings", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    truth = planted_samples(a.n, 1, a.K, 0.0)[0]
    X = rng.normal(0, 6, (a.K, 3))[truth - 1] + rng.normal(0, 1, (a.n, 3))
    S = planted_samples(a.n, a.m, a.K, a.noise)
    ctx = rc.Context.from_points(X)
    P = rc.likelihood_hyperparams_device(ctx, truth)
    ctx.set_params(**P)
    ctx.score(S[:2])                                                       # first launches
    cases = [("samples", S)]
    if a.cuts > 0:
        h = _lib.hclust(None, a.m, 0, samples=S)
        cases.append(("cuts", np.stack([_lib.hclust_cut(h["merges"], a.n, K) for K in range(1, a.cuts + 1)])))
    for case, labs in cases:
        L = len(labs)
        r, p = np.full(L, 1.0), np.full(L, 0.5)
        ctx.score(labs[:: max(L // 8, 1)], 1.0, 0.5)                       # warm-up at this shape
        walls, outs = timed(a.reps, lambda: ctx.score(labs, r, p))
        kms = [o["kernel_ms"] for o in outs]
        dev_wall = statistics.median(walls)
        print(json.dumps(dict(what="score", case=case, n=a.n, L=L, K_max=int(outs[-1]["K"].max()), reps=a.reps,
                              kernel_ms_median=round(statistics.median(kms), 2), kernel_ms_min=round(min(kms), 2),
                              kernel_ms_max=round(max(kms), 2), us_per_labelling=round(1e3 * statistics.median(kms) / L, 1),
                              wall_s_median=round(dev_wall, 3), wall_s_min=round(min(walls), 3))), flush=True)
        pick = np.unique(np.linspace(0, L - 1, min(L, a.route_labellings)).astype(int))
        ctx.set_state(labs[pick[0]]); ctx.loglik()                         # the route's first call, untimed
        t0 = time.perf_counter()
        ll = []
        for l in pick:
            ctx.set_state(labs[l])
            ll.append(ctx.loglik())
        t_route = time.perf_counter() - t0
        print(json.dumps(dict(what="set_state + loglik per labelling", case=case, labellings_timed=len(pick), wall_s=round(t_route, 3),
                              extrapolated_to_labellings=L, extrapolated_wall_s=round(t_route / len(pick) * L, 2),
                              score_wall_s_median=round(dev_wall, 3), speedup=round(t_route / len(pick) * L / dev_wall, 1),
                              same_bits=bool(np.array_equal(np.array(ll), outs[-1]["loglik"][pick])))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
