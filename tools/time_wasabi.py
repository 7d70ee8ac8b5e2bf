"""Times of the several-partition summary (redclust.jl_amd/wasabi.py; rc_vi_search_groups, csrc/visearch.inc.hip), in the
pattern of tools/time_visearch.py.  Three measurements, one JSON line each:

  grouped_vs_sequential  the kernel time (and the wall time) of ONE rc_vi_search_groups launch against the summed kernel times
                         (and walls) of the same groups searched by consecutive rc_vi_search calls in the same process — the
                         existing entry is the yardstick; the results are checked to be equal
  wasabi                 the wall time of one wasabi call
  vi_search_vs_parent    (--against PARENT_SO) rc_vi_search of this build against a library built from the parent commit, in
                         alternating child processes of tools/time_visearch.py (RC_LIB_PATH selects the library)

    python tools/time_wasabi.py                                  # n = 8192, m = 1000, L = 2, 4, 8
    python tools/time_wasabi.py --n 2000 --L 2 4
    python tools/time_wasabi.py --against /path/to/parent/libredclust_hip.so --rounds 3

Inputs: two planted partitions with K = 50 clusters each ("modes"); every sample is one of them (alternately) with 20 % of its
points relabelled at random (seed 0).  The grouped measurement gives every sample the group s mod L and each group two runs:
from empty labels in searchpointestimate's first Philox order (key 0) and from the group's first sample in identity order —
the shape of wasabi's update step with nruns = 1."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redclust_amd as rc  # noqa: E402
from redclust_amd import _lib  # noqa: E402


def two_mode_samples(n, m, K, noise, seed=0):
    rng = np.random.default_rng(seed)
    modes = rng.integers(0, K, size=(2, n))
    samples = modes[np.arange(m) % 2].copy()
    flip = rng.random((m, n)) < noise
    samples[flip] = rng.integers(0, K, size=int(flip.sum()))
    return samples.astype(np.int64) + 1


def stats(x, digits):
    return dict(median=round(statistics.median(x), digits), min=round(min(x), digits), max=round(max(x), digits))


def grouped_vs_sequential(S, L, reps):
    m, n = S.shape
    group = (np.arange(m) % L).astype(np.int32)
    order0 = np.random.Generator(np.random.Philox(key=0)).permutation(n).astype(np.int32) + 1
    ident = np.arange(1, n + 1, dtype=np.int32)
    init = np.stack([x for g in range(L) for x in (np.zeros(n, np.int64), S[g])])
    order = np.stack([x for g in range(L) for x in (order0, ident)])
    run_group = np.repeat(np.arange(L, dtype=np.int32), 2)
    gk, gw, sk, sw, same = [], [], [], [], True
    for _ in range(reps):
        t0 = time.perf_counter()
        grouped = _lib.vi_search_groups(S, group, init, order, run_group)
        gw.append(time.perf_counter() - t0)
        gk.append(grouped["kernel_ms"])
        k = w = 0.0
        for g in range(L):
            t0 = time.perf_counter()
            one = _lib.vi_search(S[group == g], init[2 * g:2 * g + 2], order[2 * g:2 * g + 2])
            w += time.perf_counter() - t0
            k += one["kernel_ms"]
            same = same and np.array_equal(one["labels"], grouped["labels"][2 * g:2 * g + 2]) and \
                np.array_equal(one["loss_num"], grouped["loss_num"][2 * g:2 * g + 2])
        sk.append(k)
        sw.append(w)
    print(json.dumps(dict(what="grouped_vs_sequential", n=n, m=m, L=L, runs=2 * L, reps=reps, grouped_kernel_ms=stats(gk, 3),
                          sequential_kernel_ms=stats(sk, 3), grouped_wall_s=stats(gw, 4), sequential_wall_s=stats(sw, 4),
                          sweeps=[int(x) for x in grouped["sweeps"]], equal=bool(same))), flush=True)


def wasabi_wall(S, L, nstarts, maxiter):
    t0 = time.perf_counter()
    res = rc.wasabi(S, L, nstarts=nstarts, maxiter=maxiter)
    wall = time.perf_counter() - t0
    print(json.dumps(dict(what="wasabi", n=S.shape[1], m=S.shape[0], L=L, nstarts=nstarts, maxiter=maxiter, wall_s=round(wall, 3),
                          kernel_ms=round(res.kernel_ms, 1), iterations=res.iterations, converged=res.converged,
                          wasserstein=res.wasserstein, weights=[round(float(w), 4) for w in res.weights], start=res.start)), flush=True)


def vi_search_vs_parent(parent_so, rounds, n):
    """alternating processes: this build, the parent, this build, … — one process has the GPU at a time"""
    meds, reps = {"this": [], "parent": []}, []                          # reps: the parent's fastest and slowest repetition
    for _ in range(rounds):
        for which in ("this", "parent"):
            env = dict(os.environ)
            if which == "parent":
                env["RC_LIB_PATH"] = parent_so
            else:
                env.pop("RC_LIB_PATH", None)
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_visearch.py"), "--n", str(n), "--no-ref"], env=env,
                                 check=True, capture_output=True, text=True).stdout
            line = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
            meds[which].append(line["kernel_ms_median"])
            if which == "parent":
                reps += [line["kernel_ms_min"], line["kernel_ms_max"]]
            print(json.dumps(dict(what="vi_search_process", library=which, n=n, kernel_ms_median=line["kernel_ms_median"],
                                  kernel_ms_min=line["kernel_ms_min"], kernel_ms_max=line["kernel_ms_max"],
                                  wall_s_median=line["wall_s_median"])), flush=True)
    # the parent's run-to-run range: its fastest and slowest single repetition over all its processes
    print(json.dumps(dict(what="vi_search_vs_parent", n=n, this_medians=meds["this"], parent_medians=meds["parent"],
                          parent_repetitions_min=min(reps), parent_repetitions_max=max(reps),
                          within_parent_range=bool(all(min(reps) <= x <= max(reps) for x in meds["this"])))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--L", type=int, nargs="*", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nstarts", type=int, default=2)
    ap.add_argument("--maxiter", type=int, default=20)
    ap.add_argument("--no-wasabi", action="store_true")
    ap.add_argument("--against", help="a libredclust_hip.so built from the parent commit: only the rc_vi_search comparison is run")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.against:
        vi_search_vs_parent(os.path.abspath(a.against), a.rounds, a.n)
        return
    warm = two_mode_samples(64, 6, 3, 0.1)
    rc.wasabi(warm, 2, nstarts=1)                                        # module load, first launches
    S = two_mode_samples(a.n, a.m, a.K, a.noise)
    for L in a.L:
        grouped_vs_sequential(S, L, a.reps)
    if not a.no_wasabi:
        for L in a.L:
            wasabi_wall(S, L, a.nstarts, a.maxiter)


if __name__ == "__main__":
    main()
