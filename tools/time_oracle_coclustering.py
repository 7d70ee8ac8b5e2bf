"""Device time and rate of generatemixture's oracle co-clustering matrix (rc_oracle_coclustering) at (N, K) = (2000, 20),
(8192, 50) and (32768, 200), T = 5000, and the NumPy restatement (tests/mixture_ref.py) at N = 2000 on the host.  Rate:
N²·T·K flop, the upper triangle of the product.

  python tools/time_oracle_coclustering.py [--sizes 2000,8192,32768] [--numiters 5000] [--no-host]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import redclust_amd as rc                                # noqa: E402
from redclust_amd._lib import oracle_coclustering as device_oracle   # noqa: E402
import mixture_ref as MR                                  # noqa: E402

KS = {2000: 20, 8192: 50, 32768: 200}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,8192,32768")
    ap.add_argument("--numiters", type=int, default=5000)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    T = a.numiters
    for n in [int(s) for s in a.sizes.split(",")]:
        K = KS.get(n, 50)
        g = rc.generatemixture(n, K, seed=1, points_only=True)
        W = MR.dirichlet_weights(K, K, T, 1)
        t0 = time.perf_counter()
        R, ms = device_oracle(g["points"], K, 1.0, 0.1, W)
        wall = time.perf_counter() - t0
        rec = dict(N=n, K=K, T=T, device_s=ms / 1e3, call_s=wall, tflops=n * n * T * K / (ms / 1e3) / 1e12)
        if n == 2000 and not a.no_host:
            t0 = time.perf_counter()
            ref = MR.oracle(g["points"], K, W, 1.0, 0.1)
            rec["host_numpy_s"] = time.perf_counter() - t0
            rec["max_abs_diff"] = float(abs(R - ref).max())
        print(json.dumps(rec), flush=True)
        del R


if __name__ == "__main__":
    main()
