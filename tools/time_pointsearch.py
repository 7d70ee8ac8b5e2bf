"""Wall and kernel time of searchpointestimate (csrc/pointsearch.inc.hip) and, at n = 2000, of the NumPy restatement
(tests/psm_search_ref.py) doing ONE run's work on the host — the only yardstick there is: the reference has no such search.

    python tools/time_pointsearch.py                  # n = 2000 and 8192, both losses, 16 runs, median of 5 repetitions
    python tools/time_pointsearch.py --n 2000 --reps 7
    python tools/time_pointsearch.py --no-ref         # skip the NumPy restatement

Inputs: a planted partition with K = 50 clusters, 20 % of the points relabelled at random in each of m = 1000 samples
(seed 0); the counts are Σ_s adjacency(sample_s), formed as one-hot products (on the device through torch when it is
there: exact, every count is below 2^24).  One JSON line per measurement."""
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


def planted_counts(n, m, K, noise, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, size=n)
    samples = np.tile(truth, (m, 1))
    flip = rng.random((m, n)) < noise
    samples[flip] = rng.integers(0, K, size=int(flip.sum()))
    try:
        import torch
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    except ImportError:
        torch, dev = None, None
    if torch is None:
        counts = np.zeros((n, n), np.float32)
        for s in range(m):
            oh = np.zeros((n, K), np.float32)
            oh[np.arange(n), samples[s]] = 1.0
            counts += oh @ oh.T
        return counts.astype(np.uint32)
    acc = torch.zeros((n, n), dtype=torch.float32, device=dev)
    S = torch.from_numpy(samples).to(dev)
    for s0 in range(0, m, 50):
        oh = torch.nn.functional.one_hot(S[s0:s0 + 50], K).to(torch.float32)      # chunk × n × K
        oh = oh.permute(1, 0, 2).reshape(n, -1)
        acc += oh @ oh.T
    return acc.cpu().numpy().astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2000, 8192])
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--nruns", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    warm = planted_counts(64, 5, 3, 0.1)
    for loss in ("binder", "VI"):
        rc.searchpointestimate(warm, loss, numsamples=5, nruns=2)                   # module load, first launches
    for n in a.n:
        t0 = time.perf_counter()
        C = planted_counts(n, a.m, a.K, a.noise)
        t_gen = time.perf_counter() - t0
        for loss in ("binder", "VI"):
            walls, kms, info = [], [], None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, info = rc.searchpointestimate(C, loss, numsamples=a.m, nruns=a.nruns, seed=0)
                walls.append(time.perf_counter() - t0)
                kms.append(info["kernel_ms"])
            sw = info["sweeps"]
            print(json.dumps(dict(what="device", n=n, m=a.m, loss=loss, nruns=a.nruns, reps=a.reps,
                                  wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4),
                                  wall_s_max=round(max(walls), 4), kernel_ms_median=round(statistics.median(kms), 3),
                                  sweeps=[int(x) for x in sw], converged=int(info["converged"].sum()),
                                  K=[int(x) for x in info["K"]], best_loss=float(info["loss"][info["best"]]),
                                  us_per_step=round(1e3 * statistics.median(kms) / (n * int(sw.max())), 3),
                                  counts_gen_s=round(t_gen, 2))), flush=True)
            if n <= 2000 and not a.no_ref:
                import psm_search_ref as R
                order = np.random.Generator(np.random.Philox(key=0)).permutation(n) + 1
                t0 = time.perf_counter()
                ref = R.psm_search_ref(C, a.m, {"binder": R.BINDER, "VI": R.VILB}[loss], np.zeros(n, np.int64), order)
                t_ref = time.perf_counter() - t0
                same = bool(np.array_equal(ref["labels"], info["labels"][0]))
                print(json.dumps(dict(what="numpy_ref_one_run", n=n, loss=loss, wall_s=round(t_ref, 3), sweeps=ref["sweeps"],
                                      K=ref["K"], equals_device_run0=same)), flush=True)


if __name__ == "__main__":
    main()
