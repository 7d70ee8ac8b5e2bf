"""Wall time of rc_psm_search, rc_hclust_samples and rc_psm_expected_loss_ctx at n = 2048, m = 200 against the library
RC_LIB_PATH selects: 3 warm-up calls, then the median (min, max) of CALLS (21) calls each, every call ending in the library's own
synchronise (it returns results to the host).  usage: RC_LIB_PATH=<a build of another commit, or unset> tools/time_counts_forms.py TAG OUTFILE [CALLS]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redclust_amd as rc
from redclust_amd import _lib

N, M, WARM, REPS = 2048, 200, 3, int(sys.argv[3]) if len(sys.argv) > 3 else 21
L = _lib.lib()
rng = np.random.default_rng(0)
truth = rng.integers(1, 51, N)
samples = np.tile(truth, (M, 1)).astype(np.int64)
flip = rng.random((M, N)) < 0.2
samples[flip] = rng.integers(1, 51, int(flip.sum()))
counts = np.zeros((N, N), np.uint32)
for s in samples:
    counts += (s[:, None] == s[None, :])


def p(a):
    return a.ctypes.data_as(C.c_void_p)


ms, cms = C.c_double(), C.c_double()
init, order = np.zeros((4, N), np.int64), np.stack([rng.permutation(N).astype(np.int32) + 1 for _ in range(4)])
labels, runs, best = np.zeros((4, N), np.int64), (_lib.RcPsmRun * 4)(), C.c_int32()
merges, bnum, vilb = np.zeros(N, _lib.HCLUST_MERGE), np.zeros(N, np.int64), np.zeros(N)
labs = np.ascontiguousarray(samples[:16])
lo, nu = np.zeros(16), np.zeros(16, np.int64)

pts = rng.normal(size=(N, 2))
ctx = rc.Context.from_points(pts)
ctx.set_params(delta1=1.0, delta2=1.0, alpha=1.0, beta=1.0, zeta=1.0, gamma=1.0)
for s in samples:
    ctx.set_state(s)
    ctx.record_sample(want_labels=False)

CALLS = {
    "rc_psm_search": lambda: L.rc_psm_search(0, p(counts), M, N, 0, 4, p(init), p(order), 0, 100, p(labels), runs, C.byref(best), C.byref(ms)),
    "rc_hclust_samples": lambda: L.rc_hclust_samples(0, p(samples), M, N, 0, p(merges), p(bnum), 0, None, C.byref(ms), C.byref(cms)),
    "rc_psm_expected_loss_ctx": lambda: L.rc_psm_expected_loss_ctx(ctx.h, M, 0, 16, p(labs), p(lo), p(nu), C.byref(ms)),
}
out = {"tag": sys.argv[1], "n": N, "m": M, "warmup": WARM, "calls": REPS}
for name, call in CALLS.items():
    t = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        code = call()
        t1 = time.perf_counter()
        if code != 0:
            sys.exit(f"{name}: code {code}: {L.rc_last_error(None).decode()}")
        if i >= WARM:
            t.append((t1 - t0) * 1e3)
    out[name] = dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t), kernel_ms=ms.value)
    print(sys.argv[1], name, out[name], flush=True)
out["checksum"] = [int(labels.sum()), int(bnum.sum()), int(nu.sum())]
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
json.dump(out, open(sys.argv[2], "w"), indent=1)
