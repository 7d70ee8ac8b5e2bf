"""Kernel and wall time of the partition distances (rc_partition_distances; csrc/partdist.inc.hip) and, for scale, of the
host loop they replace: expectedvi, one labelling at a time.

    python tools/time_partdist.py                  # n = 8192, m = 1000, median of 5 repetitions
    python tools/time_partdist.py --n 2000 --reps 7
    python tools/time_partdist.py --no-host        # skip the NumPy loop

Inputs: a planted partition with K = 50 clusters, 20 % of the points relabelled at random in each of m = 1000 samples (seed 0).
Timed: L = 1 — the distances a credible ball around one estimate needs (the estimate is the planted partition) — and
L = ⌈n/8⌉ — every cut of the average-linkage dendrogram up to that many clusters, what hclustpointestimate(exact=True)
evaluates — each with the histograms in LDS and in global memory (RC_PARTDIST_HIST_GLOBAL=1), and the LDS form also with
Gq read from global memory instead of its copy in LDS (RC_PARTDIST_GQ_GLOBAL=1); then credibleball and
hclustpointestimate(exact=True) end to end.  kernel_ms is the device time of the call's kernels; the wall time adds the host
preparation (dense ids, the samples' sorted orders) and the copies.  The host loop is timed on --host-labellings cuts (3 by
default) spread over the range and extrapolated linearly to all of them, which is said in its line; its values are compared
with the device's.  One JSON line per measurement."""
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
    ap.add_argument("--n", type=int, nargs="*", default=[8192])
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-labellings", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    warm = planted_samples(64, 5, 3, 0.1)
    for hist_env in ("0", "1"):
        for gq_env in ("0", "1"):
            os.environ["RC_PARTDIST_HIST_GLOBAL"], os.environ["RC_PARTDIST_GQ_GLOBAL"] = hist_env, gq_env   # read at every call
            _lib.partition_distances(warm[:2], warm)                       # module load, first launches
    os.environ["RC_PARTDIST_GQ_GLOBAL"] = "0"
    for n in a.n:
        S = planted_samples(n, a.m, a.K, a.noise)
        truth = planted_samples(n, 1, a.K, 0.0)                            # the same seed: the planted partition itself
        ncut = -(-n // 8)
        os.environ["RC_PARTDIST_HIST_GLOBAL"] = "0"
        merges = _lib.hclust(None, a.m, 0, samples=S)["merges"]
        cuts = np.stack([_lib.hclust_cut(merges, n, K) for K in range(1, ncut + 1)])
        results = {}
        for what, labs in (("one estimate", truth), ("dendrogram cuts", cuts)):
            for hist, env, gq_env in (("lds", "0", "0"), ("lds, Gq global", "0", "1"), ("global", "1", "0")):
                os.environ["RC_PARTDIST_HIST_GLOBAL"], os.environ["RC_PARTDIST_GQ_GLOBAL"] = env, gq_env
                walls, outs = timed(a.reps, lambda: _lib.partition_distances(labs, S, want_sq=False))
                kms = [o["kernel_ms"] for o in outs]
                results[(what, hist)] = outs[-1]
                print(json.dumps(dict(what="partition_distances", labellings=what, L=len(labs), n=n, m=a.m, histogram=hist, reps=a.reps,
                                      kernel_ms_median=round(statistics.median(kms), 3), kernel_ms_min=round(min(kms), 3),
                                      kernel_ms_max=round(max(kms), 3),
                                      ns_per_pair=round(1e6 * statistics.median(kms) / (len(labs) * a.m), 2),
                                      wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4))), flush=True)
            same = all(np.array_equal(results[(what, "lds")]["phi"], results[(what, k)]["phi"]) for k in ("lds, Gq global", "global"))
            print(json.dumps(dict(what="check", labellings=what, n=n, all_variants_equal=bool(same))), flush=True)
        os.environ["RC_PARTDIST_HIST_GLOBAL"], os.environ["RC_PARTDIST_GQ_GLOBAL"] = "0", "0"
        walls, outs = timed(a.reps, lambda: rc.credibleball(truth[0], S, "VI", 0.05))
        print(json.dumps(dict(what="credibleball", loss="VI", n=n, m=a.m, epsilon=outs[-1]["epsilon"], level=outs[-1]["level"],
                              wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4))), flush=True)
        walls, outs = timed(max(a.reps // 2, 1), lambda: rc.hclustpointestimate(argparse.Namespace(clusts=S), "VI", "average", exact=True))
        info = outs[-1][1]
        print(json.dumps(dict(what="hclustpointestimate exact", loss="VI", n=n, m=a.m, cuts=len(info["loss"]), K=info["K"],
                              loss_of_cut=float(info["loss"][info["K"] - 1]), distances_ms=round(info["distances_ms"], 3),
                              wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4))), flush=True)
        if a.no_host:
            continue
        ks = sorted({int(round(x)) for x in np.linspace(1, ncut, a.host_labellings)})
        t0 = time.perf_counter()
        host = [rc.expectedvi(cuts[K - 1], S) for K in ks]
        t_np = time.perf_counter() - t0
        dev, _ = rc.expecteddistances(cuts[[K - 1 for K in ks]], S, "VI")
        wall_dev = statistics.median(timed(a.reps, lambda: rc.expecteddistances(cuts, S, "VI"))[0])
        print(json.dumps(dict(what="numpy expectedvi", n=n, m=a.m, labellings_timed=len(ks), cuts_timed=ks, wall_s=round(t_np, 3),
                              extrapolated_to_labellings=ncut, extrapolated_wall_s=round(t_np / len(ks) * ncut, 1),
                              device_expecteddistances_wall_s=round(wall_dev, 4),
                              device_is_faster=bool(wall_dev < t_np / len(ks) * ncut),
                              max_abs_diff_to_device=float(np.max(np.abs(np.array(host) - dev))))), flush=True)


if __name__ == "__main__":
    main()
