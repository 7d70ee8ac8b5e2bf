"""Kernel and wall time of the relabelling (rc_relabel; csrc/relabel.inc.hip) and, for scale, of the host route on the same
inputs: a NumPy cross-tabulation, scipy.optimize.linear_sum_assignment and the renaming, one sample at a time.

    python tools/time_relabel.py                   # both cases, median of 10 repetitions after a warm-up
    python tools/time_relabel.py --reps 15 --no-host

Cases (seed 0): "planted K=50" — n = 8192, m = 1000, a planted partition of 50 clusters with 20 % of the points relabelled at
random in every sample, the pivot the planted partition: the tables (50 × 50) are in LDS; and "large K" — n = 8192, a planted
partition of 1000 clusters, --large-m samples (100 by default), the pivot the planted partition: the tables (about 1000 × 1000)
are in the global slabs.  The first case is also timed with RC_RELABEL_TABLE_GLOBAL=1.  kernel_ms is the device time of the
call's kernels; the wall time adds the host preparation (dense ids) and the copies, labels (m×n int64) among them.  The host route
is timed after a call of its own (SciPy is imported above), on --host-samples samples (200 by default; all of them when 0 or
when there are fewer) and extrapolated linearly to m, which is said in its line; SciPy's choice
among tied optima is not specified, so only its optimum value is compared with the device's overlap.  One JSON line per
measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from redclust_amd import _lib  # noqa: E402
from time_hclust import planted_samples, timed  # noqa: E402


def host_route(S, c):
    """(labels, overlap) by cross-tabulation, linear_sum_assignment and renaming, per sample"""
    cn, ci = np.unique(c, return_inverse=True)
    labels, overlap = np.zeros(S.shape, np.int64), np.zeros(len(S), np.int64)
    for s, z in enumerate(S):
        zn, zi = np.unique(z, return_inverse=True)
        N = np.bincount(ci * len(zn) + zi, minlength=len(cn) * len(zn)).reshape(len(cn), len(zn))
        rows, cols = linear_sum_assignment(N, maximize=True)
        to = np.zeros(len(zn), np.int64)
        to[cols] = cn[rows]
        labels[s] = to[zi]
        overlap[s] = N[rows, cols].sum()
    return labels, overlap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--large-m", type=int, default=100)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-samples", type=int, default=200)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    warm = planted_samples(64, 5, 3, 0.1)
    for env in ("1", "0"):
        os.environ["RC_RELABEL_TABLE_GLOBAL"] = env                        # read at every call
        _lib.relabel(warm, warm[0])                                        # module load, first launches
    host_route(warm, warm[0])                                              # the host route's first call, untimed as well
    for case, K, m in (("planted K=50", 50, a.m), ("large K", 1000, a.large_m)):
        S = planted_samples(a.n, m, K, a.noise)
        c = planted_samples(a.n, 1, K, 0.0)[0]                             # the same seed: the planted partition itself
        outs_by = {}
        for table, env in (("lds" if K == 50 else "global (does not fit LDS)", "0"),) + ((("global (forced)", "1"),) if K == 50 else ()):
            os.environ["RC_RELABEL_TABLE_GLOBAL"] = env
            _lib.relabel(S, c)                                             # warm-up at this shape
            walls, outs = timed(a.reps, lambda: _lib.relabel(S, c))
            kms = [o["kernel_ms"] for o in outs]
            outs_by[table] = outs[-1]
            if env == "0":
                dev_wall = statistics.median(walls)                        # the default route's
            print(json.dumps(dict(what="relabel", case=case, n=a.n, m=m, K_pivot=len(np.unique(c)), K_samples_max=outs[-1]["maps"].shape[1],
                                  table=table, reps=a.reps, kernel_ms_median=round(statistics.median(kms), 3), kernel_ms_min=round(min(kms), 3),
                                  kernel_ms_max=round(max(kms), 3), us_per_sample=round(1e3 * statistics.median(kms) / m, 2),
                                  wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4))), flush=True)
        os.environ["RC_RELABEL_TABLE_GLOBAL"] = "0"
        first = next(iter(outs_by.values()))
        same = all(all(np.array_equal(first[k], o[k]) for k in ("labels", "maps", "overlap", "counts")) for o in outs_by.values())
        print(json.dumps(dict(what="check", case=case, all_variants_equal=bool(same),
                              mean_disagreement=round(float(1 - first["overlap"].mean() / a.n), 4))), flush=True)
        if a.no_host:
            continue
        mh = m if a.host_samples <= 0 else min(m, a.host_samples)
        host_route(S[:2], c)                                               # warm-up at this shape
        t0 = time.perf_counter()
        _, ov = host_route(S[:mh], c)
        t_np = time.perf_counter() - t0
        print(json.dumps(dict(what="host route (numpy + scipy)", case=case, n=a.n, samples_timed=mh, wall_s=round(t_np, 3),
                              extrapolated_to_samples=m, extrapolated_wall_s=round(t_np / mh * m, 3), device_wall_s_median=round(dev_wall, 4),
                              device_is_faster=bool(dev_wall < t_np / mh * m),
                              optimum_equals_device_overlap=bool(np.array_equal(ov, first["overlap"][:mh])))), flush=True)


if __name__ == "__main__":
    main()
