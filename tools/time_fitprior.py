"""Wall time of the batched k-medoids scan, of fitprior and fitprior2 (prior.py) and of sampleK on the device, of the
batched k-means scan and of fitprior_kmeans / fitprior2_kmeans, and of the NumPy restatements (tests/kmedoids_ref.py,
tests/kmeans_ref.py) doing a scan's work on one CPU core.  fitprior2 - fitprior is the cost of the
per-k split plus sampleK; the sampleK line has its default count for n, max(10^4, 100 n), with rc_sample_k's kernel time.

    python tools/time_fitprior.py                 # device: n = 2000 (Kmax 1000) and n = 8192 (Kmax 4096)
    python tools/time_fitprior.py --ref           # + the k-medoids restatement's scan at n = 2000 (no GPU needed; minutes)
    python tools/time_fitprior.py --ref-kmeans    # + the k-means restatement's scan at n = 2000 (no GPU needed; minutes)
    python tools/time_fitprior.py --only kmeans   # only the k-means lines (or: --only kmedoids)
    OMP_NUM_THREADS=1 taskset -c 0 python tools/time_fitprior.py --ref --no-gpu   # the restatement on one core

Inputs: generatemixture(n, 20, seed=0).  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import redclust_amd as rc  # noqa: E402
from redclust_amd._lib import sample_k  # noqa: E402


def device(n):
    D = rc.generatemixture(n, 20, seed=0)["distancematrix"]
    ctx = rc.Context(D)
    ctx.kmedoids_scan(1, 8, maxiter=1000)   # warm-up: module load, first launches
    t0 = time.perf_counter()
    scan = ctx.kmedoids_scan(1, n // 2, maxiter=1000)
    t_scan = time.perf_counter() - t0
    ctx.close()
    t0 = time.perf_counter()
    P = rc.fitprior(D, "k-medoids", True, verbose=False)
    t_fit = time.perf_counter() - t0
    it = scan["iterations"]
    print(json.dumps(dict(what="device", n=n, Kmax=n // 2, scan_s=round(t_scan, 3), fitprior_s=round(t_fit, 3),
                          K=P.K_initial, iterations_max=int(it.max()), iterations_mean=round(float(it.mean()), 2),
                          not_converged=int((~scan["converged"]).sum()))), flush=True)
    ctx = rc.Context(D)
    t0 = time.perf_counter()
    ctx.kmedoids_scan(1, n // 2, maxiter=1000, split=True)
    t_split = time.perf_counter() - t0
    ctx.close()
    t0 = time.perf_counter()
    P2 = rc.fitprior2(D, "k-medoids", True, verbose=False)
    t_fit2 = time.perf_counter() - t0
    print(json.dumps(dict(what="device_fitprior2", n=n, Kmax=n // 2, scan_split_s=round(t_split, 3),
                          split_minus_scan_s=round(t_split - t_scan, 3), fitprior2_s=round(t_fit2, 3),
                          fitprior2_minus_fitprior_s=round(t_fit2 - t_fit, 3), K=P2.K_initial)), flush=True)
    m = max(10000, 100 * n)
    rng = np.random.default_rng(0)
    r, p = rng.gamma(P.eta, 1 / P.sigma, m), rng.beta(P.u, P.v, m)
    t0 = time.perf_counter()
    _, kms = sample_k(n, r, p, seed=1)
    t_sk = time.perf_counter() - t0
    print(json.dumps(dict(what="device_sampleK", n=n, numsamples=m, scores=m * n, wall_s=round(t_sk, 3),
                          kernel_ms=round(kms, 2), scores_per_s=float(f"{m * n / (kms * 1e-3):.3g}"))), flush=True)


def device_kmeans(n):
    pts = rc.generatemixture(n, 20, seed=0, points_only=True)["points"]
    ctx = rc.Context.from_points(pts)
    ctx.kmeans_scan(1, 8, maxiter=1000)   # warm-up: module load, first launches
    t0 = time.perf_counter()
    scan = ctx.kmeans_scan(1, n // 2, maxiter=1000)
    t_scan = time.perf_counter() - t0
    t0 = time.perf_counter()
    ctx.kmeans_scan(1, n // 2, maxiter=1000, split=True)
    t_split = time.perf_counter() - t0
    ctx.close()
    t0 = time.perf_counter()
    P = rc.fitprior_kmeans(pts, verbose=False)
    t_fit = time.perf_counter() - t0
    t0 = time.perf_counter()
    P2 = rc.fitprior2_kmeans(pts, verbose=False)
    t_fit2 = time.perf_counter() - t0
    it = scan["iterations"]
    rounds = int(it.max()) + 1   # assignment passes of the slowest run; every pass of a run costs n·k·dim·3 flop
    flop = float(sum(3.0 * n * k * pts.shape[1] * (int(t) + 1) for k, t in zip(range(1, n // 2 + 1), it)))
    print(json.dumps(dict(what="device_kmeans", n=n, dim=int(pts.shape[1]), Kmax=n // 2, scan_s=round(t_scan, 3),
                          scan_split_s=round(t_split, 3), fitprior_kmeans_s=round(t_fit, 3), fitprior2_kmeans_s=round(t_fit2, 3),
                          K=P.K_initial, K2=P2.K_initial, iterations_max=int(it.max()), iterations_mean=round(float(it.mean()), 2),
                          not_converged=int((~scan["converged"]).sum()), rounds_max=rounds,
                          assign_tflop=round(flop / 1e12, 4), assign_tflops=round(flop / 1e12 / t_scan, 3))), flush=True)


def restatement_kmeans(n):
    import kmeans_ref as KM
    pts = rc.generatemixture(n, 20, seed=0, points_only=True)["points"]
    t0 = time.perf_counter()
    for k in range(1, n // 2 + 1):
        KM.kmeans(pts, k, maxiter=1000)
    t = time.perf_counter() - t0
    print(json.dumps(dict(what="kmeans_restatement_one_core", n=n, Kmax=n // 2, scan_s=round(t, 2))), flush=True)


def restatement(n):
    import kmedoids_ref as KR
    D = rc.generatemixture(n, 20, seed=0)["distancematrix"]
    ex = int(np.frexp(D.max())[1])
    eD = 47 - ex   # the device's exponent for such a matrix (derived logD); the timing does not depend on it
    Dq = np.rint(np.ldexp(D, eD)).astype(np.int64)
    t0 = time.perf_counter()
    for k in range(1, n // 2 + 1):
        KR.kmedoids(Dq, eD, k, maxiter=1000)
    t = time.perf_counter() - t0
    print(json.dumps(dict(what="restatement_one_core", n=n, Kmax=n // 2, scan_s=round(t, 2))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,8192")
    ap.add_argument("--ref", action="store_true", help="also time the NumPy restatement at n = 2000")
    ap.add_argument("--ref-kmeans", action="store_true", help="also time the k-means restatement at n = 2000")
    ap.add_argument("--only", choices=("kmedoids", "kmeans"), help="only that family's device lines")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    if not a.no_gpu:
        for n in [int(x) for x in a.sizes.split(",")]:
            if a.only != "kmeans":
                device(n)
            if a.only != "kmedoids":
                device_kmeans(n)
    if a.ref:
        restatement(2000)
    if a.ref_kmeans:
        restatement_kmeans(2000)
