"""Wall and kernel time of the exact expected-VI search (rc_vi_search, csrc/visearch.inc.hip) — or, with --loss ID, of the
exact expected-ID search (rc_id_search, the same kernel) — and, at n = 2000, of the NumPy restatement (tests/vi_search_ref.py,
tests/id_search_ref.py) doing ONE run's work on the host — the only yardstick there is: the reference has no such search.

    python tools/time_visearch.py                  # n = 2000 and 8192, 16 runs, median of 5 repetitions
    python tools/time_visearch.py --n 2000 --reps 7
    python tools/time_visearch.py --no-ref         # skip the NumPy restatement
    python tools/time_visearch.py --loss ID        # the same input through rc_id_search
    python tools/time_visearch.py --loss omARI     # or NVI, NID: rc_ratio_search (csrc/ratiosearch.inc.hip) on the same input, and for
                                                   # comparison rc_vi_search alternating with it in the same process; no NumPy run
    python tools/time_visearch.py --maxsweeps 1    # the first sweep alone (sequential allocation: every point moves)
    python tools/time_visearch.py --large          # rc_vi_search_large at n = 8192, 16384, 32767; at 8192 alternating with rc_vi_search
    python tools/time_visearch.py --large --loss ID   # rc_id_search_large likewise, against rc_id_search; and at every size alternating
                                                      # with itself under RC_ID_TABLE_GLOBAL=1: the fenced placement of F's table
    python tools/time_visearch.py --fence-probe    # rc_id_search_large where the host fences F's table unasked (n = 32767, m = 2048)

Inputs: a planted partition with K = 50 clusters, 20 % of the points relabelled at random in each of m = 1000 samples
(seed 0).  The timed call is _lib.vi_search (_lib.id_search) with 16 runs from empty labels in the orders searchpointestimate draws
(Philox, key 0): the wall time includes the host's re-labelling and transposition of the samples, the copies and the
zeroing of the tables.  One JSON line per measurement."""
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
from redclust_amd import _lib  # noqa: E402


def planted_samples(n, m, K, noise, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, size=n)
    samples = np.tile(truth, (m, 1))
    flip = rng.random((m, n)) < noise
    samples[flip] = rng.integers(0, K, size=int(flip.sum()))
    return samples.astype(np.int64) + 1


def time_large(a):
    """k_vilarge (k_idlarge with --loss ID) at the sizes of a.n; where rc_vi_search (rc_id_search) runs too (n <= 8192) the two
    alternate on the same inputs in this process and the runs are compared, and so does, for ID, the same call with F's table
    fenced.  µs per step = the kernel's median over n · (the largest sweep count of any run)."""
    large, small = (_lib.id_search_large, _lib.id_search) if a.loss == "ID" else (_lib.vi_search_large, _lib.vi_search)
    same = lambda x, y: bool(all(np.array_equal(x[k], y[k]) for k in ("labels", "loss_num", "sweeps", "moves", "K")))
    for n in a.n:
        S = planted_samples(n, a.m, a.K, a.noise)
        rng = np.random.Generator(np.random.Philox(key=0))
        order = np.stack([rng.permutation(n).astype(np.int32) + 1 for _ in range(a.nruns)])
        init = np.zeros((a.nruns, n), np.int64)
        new, old, fenced, res, res_old, res_fenced = [], [], [], None, None, None
        for _ in range(a.reps):
            res = large(S, init, order, maxsweeps=a.maxsweeps)
            new.append(res["kernel_ms"])
            if n <= 8192:
                res_old = small(S, init, order, maxsweeps=a.maxsweeps)
                old.append(res_old["kernel_ms"])
            if a.loss == "ID":
                os.environ["RC_ID_TABLE_GLOBAL"] = "1"                 # read by the library at every call
                try:
                    res_fenced = large(S, init, order, maxsweeps=a.maxsweeps)
                finally:
                    del os.environ["RC_ID_TABLE_GLOBAL"]
                fenced.append(res_fenced["kernel_ms"])
        out = dict(what="large", loss=a.loss, n=n, m=a.m, nruns=a.nruns, reps=a.reps, kernel_ms_median=round(statistics.median(new), 3),
                   kernel_ms_min=round(min(new), 3), kernel_ms_max=round(max(new), 3), sweeps_max=int(res["sweeps"].max()),
                   us_per_step=round(1e3 * statistics.median(new) / (n * int(res["sweeps"].max())), 3))
        if old:
            out.update(old_kernel_ms_median=round(statistics.median(old), 3), old_kernel_ms_min=round(min(old), 3),
                       old_kernel_ms_max=round(max(old), 3), new_over_old=round(statistics.median(new) / statistics.median(old), 4),
                       same_bytes=same(res, res_old))
        if fenced:
            out.update(fenced_kernel_ms_median=round(statistics.median(fenced), 3), fenced_kernel_ms_min=round(min(fenced), 3),
                       fenced_kernel_ms_max=round(max(fenced), 3), fenced_over_whole=round(statistics.median(fenced) / statistics.median(new), 4),
                       fenced_same_bytes=same(res, res_fenced))
        print(json.dumps(out), flush=True)


def fence_probe(a):
    """rc_id_search_large where the table of F does not fit LDS whole, so that the host chooses the fence's shift itself (the first
    shape; at these samples' slot cap of 5 the second still fits whole), against the same call with the forced, coarser fence: the
    same bytes are expected.  Samples with ~95 % of the points in one
    cluster (the tests' skewed()), two runs in the identity order — from empty labels and from the first sample — two sweeps."""
    from test_gpu_visearch_large import skewed
    for n, m in ((32767, 2048), (24001, 2700)):
        S = skewed(n, m)
        init = np.stack([np.zeros(n, np.int64), S[0]])
        order = np.tile(np.arange(1, n + 1, dtype=np.int32), (2, 1))
        chosen = _lib.id_search_large(S, init, order, maxsweeps=2)
        os.environ["RC_ID_TABLE_GLOBAL"] = "1"
        try:
            forced = _lib.id_search_large(S, init, order, maxsweeps=2)
        finally:
            del os.environ["RC_ID_TABLE_GLOBAL"]
        same = all(np.array_equal(chosen[k], forced[k]) for k in ("labels", "loss", "loss_num", "sweeps", "moves", "K"))
        print(json.dumps(dict(what="fence_probe", n=n, m=m, same_bytes=bool(same), kernel_ms=round(chosen["kernel_ms"], 3),
                              forced_kernel_ms=round(forced["kernel_ms"], 3), K=[int(x) for x in chosen["K"]],
                              largest_cluster=[int(np.bincount(x).max()) for x in chosen["labels"]])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2000, 8192])
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--nruns", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--loss", choices=["VI", "ID", "omARI", "NVI", "NID"], default="VI")
    ap.add_argument("--maxsweeps", type=int, default=100)
    ap.add_argument("--large", action="store_true", help="rc_vi_search_large / rc_id_search_large; default sizes 8192 16384 32767")
    ap.add_argument("--fence-probe", action="store_true", help="rc_id_search_large with the fence the host chooses against the forced one")
    a = ap.parse_args()
    if a.fence_probe:
        return fence_probe(a)
    if a.large and a.n == [2000, 8192]:
        a.n = [8192, 16384, 32767]
    ratio = a.loss in _lib.RATIO_LOSSES
    if ratio and a.large:
        ap.error("--large has no ratio-loss kernel")
    search = {"VI": _lib.vi_search, "ID": _lib.id_search}.get(a.loss, lambda S, *rest, **kw: _lib.ratio_search(S, a.loss, *rest, **kw))
    expected = {"VI": rc.expectedvi, "ID": rc.expectedid, "omARI": rc.expectedomari, "NVI": rc.expectednvi, "NID": rc.expectednid}[a.loss]
    warm = planted_samples(64, 5, 3, 0.1)
    search(warm, np.zeros((2, 64), np.int64), np.tile(np.arange(1, 65, dtype=np.int32), (2, 1)))   # module load, first launch
    if a.large:
        return time_large(a)
    for n in a.n:
        S = planted_samples(n, a.m, a.K, a.noise)
        rng = np.random.Generator(np.random.Philox(key=0))
        order = np.stack([rng.permutation(n).astype(np.int32) + 1 for _ in range(a.nruns)])
        init = np.zeros((a.nruns, n), np.int64)
        walls, kms, vi_kms, res, vi = [], [], [], None, None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = search(S, init, order, maxsweeps=a.maxsweeps)
            walls.append(time.perf_counter() - t0)
            kms.append(res["kernel_ms"])
            if ratio:
                vi = _lib.vi_search(S, init, order, maxsweeps=a.maxsweeps)
                vi_kms.append(vi["kernel_ms"])
        compare = {} if not ratio else dict(vi_kernel_ms_median=round(statistics.median(vi_kms), 3), vi_sweeps=[int(x) for x in vi["sweeps"]],
                                            vi_us_per_step=round(1e3 * statistics.median(vi_kms) / (n * int(vi["sweeps"].max())), 3))
        sw = res["sweeps"]
        best = res["labels"][res["best"]]
        print(json.dumps(dict(what="device", loss=a.loss, maxsweeps=a.maxsweeps, n=n, m=a.m, nruns=a.nruns, reps=a.reps,
                              wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4),
                              wall_s_max=round(max(walls), 4), kernel_ms_median=round(statistics.median(kms), 3),
                              kernel_ms_min=round(min(kms), 3), kernel_ms_max=round(max(kms), 3),
                              sweeps=[int(x) for x in sw], converged=int(res["converged"].sum()), K=[int(x) for x in res["K"]],
                              best_loss=float(res["loss"][res["best"]]), **{f"expected{a.loss.lower()}_of_best": expected(best, S)},
                              us_per_step=round(1e3 * statistics.median(kms) / (n * int(sw.max())), 3),
                              table_reads_per_step=a.m * a.K, **compare)), flush=True)
        if n <= 2000 and not a.no_ref and not ratio:
            import id_search_ref
            import vi_search_ref
            run_ref = vi_search_ref.vi_search_ref if a.loss == "VI" else id_search_ref.id_search_ref
            G = _lib.vi_gtable(n)
            t0 = time.perf_counter()
            ref = run_ref(S, G, init[0], order[0], maxsweeps=a.maxsweeps)
            t_ref = time.perf_counter() - t0
            same = bool(np.array_equal(ref["labels"], res["labels"][0]) and ref["loss_num"] == int(res["loss_num"][0]))
            print(json.dumps(dict(what="numpy_ref_one_run", loss=a.loss, n=n, wall_s=round(t_ref, 3), sweeps=ref["sweeps"], K=ref["K"],
                                  equals_device_run0=same)), flush=True)


if __name__ == "__main__":
    main()
