"""Kernel and wall time of predict (rc_predict; csrc/predict.inc.hip) and, for scale, of its NumPy restatement on the CPU;
with --joint also of the joint predict (rc_predict_joint; csrc/predictjoint.inc.hip) on the same inputs.

    python tools/time_predict.py                       # n = 8192, K = 50, m = 1000 samples, q = 1024 new points
    python tools/time_predict.py --n 2048 --q 256 --reps 3
    python tools/time_predict.py --joint --sweeps 0 2  # rc_predict, then rc_predict_joint with 0 and with 2 Gibbs passes
    python tools/time_predict.py --points              # predict_points from coordinates (dim = 50): q = 1024 with the labels,
                                                       # q = 65536 counts only, and predict(new_points=, points=) at q = 1024

Inputs (seed 0): n + q observations from K Gaussian groups in 8 dimensions, the last q held out; the m samples are the true
training labels with 2 % of the points relabelled at random in each; r and p drawn once per sample; the likelihood
hyperparameters are likelihood_hyperparams of the first 1024 training points under the truth.  Timed, after a small call
that loads the module and a first full call: `reps` calls of rc_predict on the q×n distances (logarithms taken by the
library).  kernel_ms is the device time of the call's kernels (events around them), wall the whole call: the host's checks,
quantisation and sorted orders, the copies, the kernels.  The NumPy reference (tests/predict_ref.py: np.add.at for the sums,
math.log1p per candidate, the oracle's uniforms) is timed on a few (sample, point) cases and extrapolated to q·m; the device's
labels of those cases are compared with it.  --joint: after rc_predict, `reps` calls of rc_predict_joint per value of --sweeps
on the same distances and the q×q distances among the new points; its kernel_ms covers the base sums (k_predict_sums) and
k_joint; a sample's workgroup makes (sweeps + 1)·q visits one after the other, all samples at once, so kernel_ms over that
number is the time of one visit.  Its NumPy reference (tests/predict_joint_ref.py) is timed on the first visits of sample 0
and extrapolated to a sample and to the call; the device's labels of those visits are compared with it.  One JSON line per
measurement."""
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


def planted(n, q, K, m, noise, dim=8, seed=0):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, size=n + q)
    X = 4.0 * rng.standard_normal((K, dim))[truth] + rng.standard_normal((n + q, dim))
    samples = np.tile(truth[:n], (m, 1))
    flip = rng.random((m, n)) < noise
    samples[flip] = rng.integers(0, K, size=int(flip.sum()))
    return X[:n], X[n:], truth, samples.astype(np.int64) + 1, rng.uniform(0.5, 3.0, m), rng.uniform(0.2, 0.8, m)


def distances(A, B, rows=64):
    out = np.empty((len(A), len(B)))
    for i in range(0, len(A), rows):
        out[i:i + rows] = np.sqrt(((A[i:i + rows, None, :] - B[None, :, :]) ** 2).sum(axis=2))
    return out


def joint(a, Dnew, Dnn, S, r, p, P):
    for sweeps in a.sweeps:
        out = _lib.predict_joint(Dnew, Dnn, S, r, p, P, sweeps=sweeps)          # first call at the timed shape
        walls, kms = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            o = _lib.predict_joint(Dnew, Dnn, S, r, p, P, sweeps=sweeps)
            walls.append(time.perf_counter() - t0)
            kms.append(o["kernel_ms"])
            assert np.array_equal(o["labels"], out["labels"])
        visits = (sweeps + 1) * a.q
        Ktr = np.array([len(np.unique(z)) for z in S])
        print(json.dumps(dict(what="rc_predict_joint", n=a.n, q=a.q, m=a.m, K=a.K, sweeps=sweeps, reps=a.reps,
                              kernel_ms_median=round(statistics.median(kms), 3), kernel_ms_min=round(min(kms), 3),
                              kernel_ms_max=round(max(kms), 3), us_per_visit=round(statistics.median(kms) * 1e3 / visits, 3),
                              visits_per_s=round(visits * a.m / (statistics.median(kms) * 1e-3), 0),
                              wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4),
                              wall_s_max=round(max(walls), 4), new_clusters_mean=round(float((out["K"] - Ktr).mean()), 3),
                              moves_per_pass=[round(float(x), 2) for x in out["moves"].mean(axis=0)])), flush=True)
    if a.no_host:
        return
    import oracle_lib as O
    import predict_joint_ref as J
    k = min(a.ref_visits, a.q)
    logDnew, logDnn = J.log_blocks(Dnew, Dnn)
    given = _lib.predict_joint(Dnew, Dnn, S[:1], r[:1], p[:1], P, sweeps=0, logDnew=logDnew, logDnn=logDnn)
    Dq, Lq, eD, eL = J.quantise_rows(Dnew[:k], Dnn[:k], logDnew[:k], logDnn[:k])
    A = O.size_table(P, a.n + a.q)
    y = np.zeros(a.q, np.int64)
    t0 = time.perf_counter()
    for i in range(k):
        cands, newlab, _, sc = J.visit_scores(i, S[0], y, Dq[i], Lq[i], eD[i], eL[i], float(r[0]), float(p[0]), P, A)
        t, _ = J.draw(cands, sc, 0, 0, i)
        y[i] = cands[t] if cands[t] else newlab
    per_visit = (time.perf_counter() - t0) / k
    agree = int((y[:k] == given["first"][0, :k]).sum())
    print(json.dumps(dict(what="numpy joint reference", visits=k, s_per_visit=round(per_visit, 6),
                          extrapolated_s_per_sample={str(sw): round(per_visit * (sw + 1) * a.q, 2) for sw in a.sweeps},
                          extrapolated_s={str(sw): round(per_visit * (sw + 1) * a.q * a.m, 1) for sw in a.sweeps},
                          device_labels_equal=f"{agree}/{k}")), flush=True)


def _rss_mib():
    import resource
    return round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1)   # the process's peak so far


def points(a):
    """--points: rc.predict_points from coordinates (dim = 50) at q = a.q with the labels kept and at q = a.q_large with only the
    counts coming back, then, for comparison at q = a.q, rc.predict(new_points=, points=), which builds the distances on the
    host in chunks and calls rc_predict per chunk.  Peak host RSS is read after each stage, in this order, so a later stage's
    figure is at least the earlier one's."""
    dim = 50
    big = max(a.q, a.q_large)
    tr, new, truth, S, r, p = planted(a.n, big, a.K, a.m, a.noise, dim=dim)
    sub = min(a.n, 1024)
    P = rc.likelihood_hyperparams(distances(tr[:sub], tr[:sub]), truth[:sub] + 1)
    kw = dict(r=r, p=p, params=P)
    rc.predict_points(S[:3, :64] % 64 + 1, tr[:64], new[:2], r=r[:3], p=p[:3], params=P)       # module load, first launches
    rel = rc.relabel(S, truth[:a.n] + 1)

    def timed(what, q, call, reps):
        first = call()
        walls, kms = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            o = call()
            walls.append(time.perf_counter() - t0)
            kms.append(o.kernel_ms)
        print(json.dumps(dict(what=what, n=a.n, dim=dim, q=q, m=a.m, K=a.K, reps=reps, kernel_ms_median=round(statistics.median(kms), 3),
                              kernel_ms_min=round(min(kms), 3), kernel_ms_max=round(max(kms), 3),
                              wall_s_median=round(statistics.median(walls), 4), wall_s_min=round(min(walls), 4),
                              wall_s_max=round(max(walls), 4), peak_rss_mib=_rss_mib())), flush=True)
        return first

    kept = timed("predict_points, labels kept", a.q, lambda: rc.predict_points(S, tr, new[:a.q], **kw), a.reps)
    hit = float((kept.map_labels == (truth[a.n:a.n + a.q] + 1)[None, :]).mean())
    only = timed("predict_points, counts only", a.q_large, lambda: rc.predict_points(S, tr, new[:a.q_large], relabelling=rel, **kw),
                 max(1, min(a.reps, 3)))
    hard = only.hard_allocation()
    print(json.dumps(dict(what="predict_points checks", map_equals_truth=round(hit, 4),
                          hard_allocation_equals_truth=round(float((hard == truth[a.n:a.n + a.q_large] + 1).mean()), 4),
                          rows_sum_to_m=bool(np.all(only.counts.sum(axis=1) == a.m)))), flush=True)
    host = timed("predict(new_points=, points=): host distances, rc_predict per chunk", a.q,
                 lambda: rc.predict(S, new_points=new[:a.q], points=tr, **kw), max(1, min(a.reps, 2)))
    print(json.dumps(dict(what="predict_points against predict(new_points=, points=)", q=a.q,
                          labels_equal_share=round(float((host.labels == kept.labels).mean()), 6),
                          map_labels_equal_share=round(float((host.map_labels == kept.map_labels).mean()), 6))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", action="store_true")
    ap.add_argument("--q-large", type=int, default=65536)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-cases", type=int, default=6)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--joint", action="store_true")
    ap.add_argument("--sweeps", type=int, nargs="+", default=[2])
    ap.add_argument("--ref-visits", type=int, default=24)
    a = ap.parse_args()
    if a.points:
        return points(a)
    tr, new, truth, S, r, p = planted(a.n, a.q, a.K, a.m, a.noise)
    sub = min(a.n, 1024)
    P = rc.likelihood_hyperparams(distances(tr[:sub], tr[:sub]), truth[:sub] + 1)
    Dnew = distances(new, tr)
    _lib.predict(Dnew[:2, :64], S[:3, :64] % 64 + 1, r[:3], p[:3], P)           # module load, first launches
    out = _lib.predict(Dnew, S, r, p, P)                                        # first call at the timed shape
    walls, kms = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        o = _lib.predict(Dnew, S, r, p, P)
        walls.append(time.perf_counter() - t0)
        kms.append(o["kernel_ms"])
        assert np.array_equal(o["labels"], out["labels"])
    adds = float(a.q) * a.m * a.n
    hit = float((out["map"] == (truth[a.n:] + 1)[None, :]).mean())
    print(json.dumps(dict(what="rc_predict", n=a.n, q=a.q, m=a.m, K=a.K, reps=a.reps, kernel_ms_median=round(statistics.median(kms), 3),
                          kernel_ms_min=round(min(kms), 3), kernel_ms_max=round(max(kms), 3),
                          gathers_per_s=round(adds / (statistics.median(kms) * 1e-3), 0), wall_s_median=round(statistics.median(walls), 4),
                          wall_s_min=round(min(walls), 4), wall_s_max=round(max(walls), 4), map_equals_truth=round(hit, 4),
                          new_cluster_share=round(float((out["labels"] == 0).mean()), 6))), flush=True)
    if a.joint:
        joint(a, Dnew, distances(new, new), S, r, p, P)
    if a.no_host:
        return
    import oracle_lib as O
    import predict_ref as R
    logD = np.log(Dnew)
    given = _lib.predict(Dnew, S, r, p, P, logDnew=logD)                        # the reference's own logarithms
    rng = np.random.default_rng(1)
    cases = [(int(rng.integers(a.m)), int(rng.integers(a.q))) for _ in range(a.ref_cases)]
    A = O.size_table(P, a.n)
    t0 = time.perf_counter()
    agree = 0
    for s, i in cases:
        Dq, Lq, eD, eL = R.quantise_rows(Dnew[i:i + 1], logD[i:i + 1], a.n)
        cands, _, sc, _ = R.score_point(Dq[0], Lq[0], eD[0], eL[0], S[s], float(r[s]), float(p[s]), P, A)
        lab, mp, _, _ = R.draw(cands, sc, 0, s, i)
        agree += int(lab == given["labels"][s, i] and mp == given["map"][s, i])
    per_case = (time.perf_counter() - t0) / len(cases)
    print(json.dumps(dict(what="numpy reference", cases=len(cases), s_per_case=round(per_case, 6),
                          extrapolated_s=round(per_case * a.q * a.m, 1), device_labels_equal=f"{agree}/{len(cases)}")), flush=True)


if __name__ == "__main__":
    main()
