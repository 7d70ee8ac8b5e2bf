"""Where the time of a point estimate from an MCMCResult goes: the co-clustering counts (rc_samples_counts,
csrc/samplecounts.inc.hip) and the three searches searchpointestimate offers on a result.

    python tools/time_pointestimate.py                          # n = 2000 and 8192, median and range of 5 repetitions
    python tools/time_pointestimate.py --n 2000 --reps 1        # one full pass (what a commit with host-built counts can afford)
    python tools/time_pointestimate.py --n 8192 --host-samples 3 --no-search
                                                                # the host cocluster_counts on the first 3 samples only

Inputs (tools/time_visearch.py's): a planted partition with K = 50 clusters, 20 % of the points relabelled at random in each
of m = 1000 samples, seed 0.  After a warm-up call at n = 64 (module load, first launches) it prints one JSON line per
measurement:
  counts   _lib.samples_counts: kernel ms and wall s (narrowing the labels on the host, the copies in and the n×n copy out)
  search   wall s of searchpointestimate(result, "binder"), (result, "VI") and (result, "VI", exact=True), 16 runs each, with the
           call's counts_ms and kernel_ms (for exact=True the exact search's kernel_ms and the inner lower-bound call's two)
  host     --host-samples k: wall s of the host NumPy cocluster_counts on the first k samples and its LINEAR EXTRAPOLATION to
           all m (labelled as such: k samples are measured, not m)
The script also runs on a commit whose searchpointestimate still builds the counts on the host: there `counts` is skipped
and counts_ms is null, so both sides of a comparison come from the same file.  On a shared machine run every invocation
under its own time limit and chain them: timeout -k 10 600 python tools/time_pointestimate.py --n 2000 && timeout -k 10 ..."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redclust_amd as rc  # noqa: E402
from redclust_amd import _lib  # noqa: E402


def planted_samples(n, m, K, noise, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, size=n)
    samples = np.tile(truth, (m, 1))
    flip = rng.random((m, n)) < noise
    samples[flip] = rng.integers(0, K, size=int(flip.sum()))
    return samples.astype(np.int64) + 1


def spread(xs, digits):
    xs = [x for x in xs if x is not None]
    if not xs:
        return None
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2000, 8192])
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--nruns", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=0)
    ap.add_argument("--no-search", action="store_true")
    a = ap.parse_args()
    on_device = hasattr(_lib, "samples_counts")
    warm = types.SimpleNamespace(clusts=list(planted_samples(64, 5, 3, 0.1)))
    if on_device:
        _lib.samples_counts(np.stack(warm.clusts))
    if not a.no_search:
        for kw in (dict(loss="binder"), dict(loss="VI"), dict(loss="VI", exact=True)):
            rc.searchpointestimate(warm, nruns=2, **kw)
    for n in a.n:
        S = planted_samples(n, a.m, a.K, a.noise)
        result = types.SimpleNamespace(clusts=list(S))
        base = dict(n=n, m=a.m, reps=a.reps)
        if on_device:
            walls, kms = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, ms = _lib.samples_counts(S)
                walls.append(time.perf_counter() - t0)
                kms.append(ms)
            print(json.dumps(dict(what="counts", **base, kernel_ms=spread(kms, 3), wall_s=spread(walls, 4),
                                  comparisons_per_s=round(n * (n + 128) / 2 * a.m / (statistics.median(kms) * 1e-3), -9))), flush=True)
        if a.host_samples:
            k = min(a.host_samples, a.m)
            t0 = time.perf_counter()
            rc.cocluster_counts(result.clusts[:k])
            t = time.perf_counter() - t0
            print(json.dumps(dict(what="host", n=n, m=a.m, samples_measured=k, wall_s_measured=round(t, 3),
                                  wall_s_per_sample=round(t / k, 4), wall_s_all_m_LINEAR_EXTRAPOLATION=round(t / k * a.m, 1),
                                  cpus=os.cpu_count())), flush=True)
        if a.no_search:
            continue
        for name, kw in (("binder", dict(loss="binder")), ("VI", dict(loss="VI")), ("VI exact", dict(loss="VI", exact=True))):
            walls, cms, kms, lb_kms, info = [], [], [], [], None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, info = rc.searchpointestimate(result, nruns=a.nruns, **kw)
                walls.append(time.perf_counter() - t0)
                inner = info.get("lower_bound", info)
                cms.append(inner.get("counts_ms"))
                kms.append(info["kernel_ms"])
                lb_kms.append(inner["kernel_ms"] if inner is not info else None)
            print(json.dumps(dict(what="search", call=name, **base, nruns=a.nruns, counts_on="device" if on_device else "host",
                                  wall_s=spread(walls, 3), counts_ms=spread(cms, 3), kernel_ms=spread(kms, 3),
                                  lower_bound_kernel_ms=spread(lb_kms, 3), sweeps_max=int(np.max(info["sweeps"])),
                                  best_loss=float(info["loss"][info["best"]]))), flush=True)


if __name__ == "__main__":
    main()
