"""Kernel and wall time of the MAP search (rc_map_search, csrc/mapsearch.inc.hip) and what the climb gains over mapestimate, beside
the NumPy restatement (tests/map_search_ref.py) doing a few visits of one run on the host — the only yardstick there is: there
is no earlier device implementation, and the reference has no such search.

    python tools/time_mapsearch.py                     # the chain case and the 1024-slot worst case
    python tools/time_mapsearch.py --n 2048 --m 200    # a smaller chain case
    python tools/time_mapsearch.py --no-ref            # skip the NumPy restatement
    python tools/time_mapsearch.py --no-chain          # the worst case alone (--no-worst: the chain case alone)

Chain case (seed 0): n = 8192 points in 3 dimensions around 50 centres (from_points: the distances are computed on the device,
the logarithms derived), the likelihood's hyperparameters fitted to the planted partition, an m = 1000 chain from the planted
partition with 30 % of the points relabelled at random.  Timed: searchmapestimate from the 16 best distinct samples plus empty
labels (17 runs, one launch) — the whole call, with the scoring of the candidates beforehand taken out of it (scores=), the
search kernel, the sweeps of every run — and the log-posterior gained over mapestimate on the same samples.
Worst case: n = 1024, every distance within 10 % of 1, parameters and a p under which every point is a cluster of its own and
stays one (the line says so: K = 1024, moves = 0): 1024 occupied slots, with repulsion 1024² partner terms per visit; one run,
one sweep, kernel time per visit.
The NumPy restatement is timed on --ref-visits visits of one run (at --ref-n points for the chain case: its matrices at n = 8192
would need several GiB of host memory) and reported per visit; nothing is extrapolated here.  One JSON line per measurement."""
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


def chain_case(n, K, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, n).astype(np.int64) + 1
    X = rng.normal(0, 6, (K, 3))[truth - 1] + rng.normal(0, 1, (n, 3))
    init = np.where(rng.random(n) < 0.3, rng.integers(1, K + 1, n), truth).astype(np.int64)
    return X, truth, init


def ref_per_visit(ctx, P, init, order, r, p, visits):
    import map_search_ref as R
    import score_ref as SR
    sc = ctx.score(np.ones(ctx.n, np.int64))
    Dq, Lq = SR.quantised(ctx.get_matrix(0), sc["eD"]), SR.quantised(ctx.get_matrix(1), sc["eL"])
    t0 = time.perf_counter()
    R.search(Dq, Lq, sc["eD"], sc["eL"], init, order, r, p, P, max_visits=1)         # the starting blocks and one visit
    t1 = time.perf_counter()
    R.search(Dq, Lq, sc["eD"], sc["eL"], init, order, r, p, P, max_visits=1 + visits)
    t2 = time.perf_counter()
    return 1e3 * ((t2 - t1) - (t1 - t0)) / visits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--nruns", type=int, default=16)
    ap.add_argument("--maxsweeps", type=int, default=100)
    ap.add_argument("--ref-n", type=int, default=2048)
    ap.add_argument("--ref-visits", type=int, default=20)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--no-worst", action="store_true")
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    if not a.no_chain:
        chain(a)
    if not a.no_worst:
        worst(a)


def chain(a):
    X, truth, init = chain_case(a.n, a.K)
    ctx = rc.Context.from_points(X)
    P = rc.likelihood_hyperparams_device(ctx, truth)
    ctx.set_params(**P)
    params = rc.PriorHyperparamsList(**{k: P[k] for k in ("delta1", "delta2", "alpha", "beta", "zeta", "gamma")})
    options = rc.MCMCOptionsList(numiters=a.m, burnin=0, thin=1, numGibbs=1, numMH=0)
    t0 = time.perf_counter()
    result = rc.runsampler(rc.MCMCData(X), options, params, rc.MCMCState(init, 1.0, 0.5), verbose=False, seed=0, ctx=ctx)
    t_chain = time.perf_counter() - t0
    sc = rc.scorelabellings(ctx, result)
    _, mi = rc.mapestimate(ctx, result, scores=sc)
    ctx.map_search(np.zeros((1, a.n), np.int64), np.arange(1, a.n + 1, dtype=np.int32)[None, :], 1.0, 0.5, maxsweeps=1)   # first launch
    t0 = time.perf_counter()
    clust, info = rc.searchmapestimate(ctx, result, nruns=a.nruns, maxsweeps=a.maxsweeps, scores=sc)
    wall = time.perf_counter() - t0
    top = float(info["logposterior"].max())
    visits = int(info["sweeps"].max()) * a.n
    print(json.dumps(dict(what="device", case="chain", n=a.n, m=a.m, runs=len(info["runs"]), chain_wall_s=round(t_chain, 2),
                          kernel_ms=round(info["kernel_ms"], 1), wall_s=round(wall, 3), sweeps=[int(x) for x in info["sweeps"]],
                          converged=int(info["converged"].sum()), K=[int(x) for x in info["K"]], moves=[int(x) for x in info["moves"]],
                          us_per_visit_of_the_longest_run=round(1e3 * info["kernel_ms"] / visits, 2),
                          mapestimate_logposterior=float(mi["logposterior"][mi["index"]]), search_logposterior=top,
                          gained=top - float(mi["logposterior"][mi["index"]]), planted_logposterior=float(
                              rc.scorelabellings(ctx, truth, None, float(np.mean(result.r)), float(np.mean(result.p)))["logposterior"][0]),
                          K_of_result=int(len(np.unique(clust))))), flush=True)
    ctx.close()
    if not a.no_ref:
        Xr, tr, ir = chain_case(a.ref_n, a.K)
        c2 = rc.Context.from_points(Xr)
        P2 = rc.likelihood_hyperparams_device(c2, tr)
        c2.set_params(**P2)
        ms = ref_per_visit(c2, P2, ir, np.random.default_rng(0).permutation(a.ref_n) + 1, 1.0, 0.5, a.ref_visits)
        print(json.dumps(dict(what="numpy_ref", case="chain", n=a.ref_n, K=a.K, visits_timed=a.ref_visits, ms_per_visit=round(ms, 2))), flush=True)
        c2.close()


def worst(a):
    n = 1024
    g = np.random.default_rng(77)
    D = np.triu(g.uniform(0.9, 1.1, (n, n)), 1)
    D = D + D.T
    Pw = dict(delta1=2.0, alpha=8.0, beta=0.01, delta2=3.0, zeta=600.0, gamma=1e4, repulsion=True)   # singletons are stable under these
    cw = rc.Context(D)
    cw.set_params(**Pw)
    start, order = np.arange(1, n + 1, dtype=np.int64)[None, :], (g.permutation(n) + 1).astype(np.int32)[None, :]
    for rep in (True, False):
        res = cw.map_search(start, order, 1.5, 1e-12, params=dict(Pw, repulsion=rep), maxsweeps=1)
        print(json.dumps(dict(what="device", case="worst", n=n, repulsion=rep, K=int(res["K"][0]), moves=int(res["moves"][0]),
                              kernel_ms=round(res["kernel_ms"], 1), us_per_visit=round(1e3 * res["kernel_ms"] / n, 1))), flush=True)
        if not a.no_ref:
            ms = ref_per_visit(cw, dict(Pw, repulsion=rep), start[0], order[0], 1.5, 1e-12, 3 if rep else a.ref_visits)
            print(json.dumps(dict(what="numpy_ref", case="worst", n=n, repulsion=rep, visits_timed=3 if rep else a.ref_visits,
                                  ms_per_visit=round(ms, 1))), flush=True)
    cw.close()


if __name__ == "__main__":
    main()
