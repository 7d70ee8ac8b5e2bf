"""Wall time of the batched k-medoids scan and of fitprior (prior.py) on the device, and of the NumPy restatement
(tests/kmedoids_ref.py) doing the scan's work on one CPU core.

    python tools/time_fitprior.py                 # device: n = 2000 (Kmax 1000) and n = 8192 (Kmax 4096)
    python tools/time_fitprior.py --ref           # + the restatement's scan at n = 2000 (no GPU needed; minutes)
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
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    if not a.no_gpu:
        for n in [int(x) for x in a.sizes.split(",")]:
            device(n)
    if a.ref:
        restatement(2000)
