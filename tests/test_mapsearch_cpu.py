"""The MAP search without a GPU: the NumPy reference (tests/map_search_ref.py) against brute-force differences of the full
log-posterior, the monotone climb, the decision gaps of every fixed input the GPU tests use, the kernel's lgamma and log1p
against libm, and the interface — header / SIGNATURES / Julia agreement and the argument errors that need no device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib
import map_search_ref as R
import oracle_lib as O
from helpers import with_diagonal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("what", ["zero diagonal", "positive diagonal", "repulsion off"])
def test_the_chosen_candidate_is_the_brute_force_argmax(what):
    """n = 40, random 4-cluster labels: at each of the first 10 visits the reference's choice — from its incremental blocks and
    the Δ of the issue — is the candidate of largest lp(c with i in it) − lp(c without i), lp evaluated from scratch."""
    n = 40
    D, _ = R.planted(n, 3, 0.3, 5)
    if what == "positive diagonal":
        D = with_diagonal(D, "positive")
    P = dict(R.P0, repulsion=what != "repulsion off")
    orc = O.Oracle(D, P)
    if what == "positive diagonal":
        assert orc.Dq.diagonal().all() and not orc.Lq.diagonal().any()
    g = np.random.default_rng(0)
    init = g.integers(1, 5, n).astype(np.int64)
    order = g.permutation(n) + 1
    r, p = 1.5, 0.1
    trace = []
    R.search(orc.Dq, orc.Lq, orc.eD, orc.eL, init, order, r, p, P, max_visits=10, trace=trace)
    assert len(trace) == 10
    moved = 0
    for i, out, w in trace:
        used = sorted(set(int(x) for x in out if x))
        new = next(k for k in range(1, n + 1) if k not in used)
        gains = {}
        for k in used + [new]:
            z = out.copy(); z[i] = k
            gains[k] = R.logposterior(orc.Dq, orc.Lq, orc.eD, orc.eL, z, r, p, P)
        best = max(gains, key=gains.get)
        second = sorted(gains.values())[-2]
        assert gains[best] - second > 1e-6                               # no tie to argue about
        assert (w == best) or (w not in used and best == new), (i, w, best, gains)
        moved += 1
    assert moved == 10


def test_every_run_ends_no_lower_than_it_started():
    """lp from scratch (R.logposterior) of the final labels against the start's: never lower, and higher wherever a point moved —
    every accepted move gains at least the run's min_gap, far above the rounding of two sums of this size."""
    for name in R.CASES:
        c, runs, orc = R.host_ref(name)
        for q, run in enumerate(runs):
            if not c["init"][q].all():
                continue                                                # unallocated points do not exist: no lp to compare with
            args = (orc.Dq, orc.Lq, orc.eD, orc.eL)
            lp0 = R.logposterior(*args, c["init"][q], float(c["r"][q]), float(c["p"][q]), c["P"])
            lp1 = R.logposterior(*args, run["labels"], float(c["r"][q]), float(c["p"][q]), c["P"])
            print(name, q, lp0, lp1, run["moves"])
            assert lp1 >= lp0, (name, q, lp0, lp1)
            assert (lp1 > lp0) == (run["moves"] > 0), (name, q, lp0, lp1, run["moves"])


@pytest.mark.parametrize("name", ["n65", "n130", "norep", "diag"])
def test_the_references_criterion_is_the_oracles_loglik_plus_logprior(name):
    """R.logposterior shares its term with search(), so a wrong sign or constant there would agree with itself.  The C oracle
    (oracle/rc_oracle.c: the reference's loglik in its stable regrouping, long double, and logprior) is independent of both:
    on the starts and the results of a fixed input the two agree to 1e-10 relative — f64 against long double over at most
    K² + K + 10 terms of magnitude below |lp|."""
    c, runs, orc = R.host_ref(name)
    seen = 0
    for q, run in enumerate(runs):
        for z in (c["init"][q], run["labels"]):
            if not np.asarray(z).all():
                continue
            r, p = float(c["r"][q]), float(c["p"][q])
            orc.set_state(np.asarray(z, np.int64))
            want = orc.loglik_stable() + orc.logprior(r, p)
            got = R.logposterior(orc.Dq, orc.Lq, orc.eD, orc.eL, z, r, p, c["P"])
            assert abs(got - want) <= 1e-10 * abs(want), (name, q, got, want)
            seen += 1
    assert seen >= 4


def test_gap_guard_of_every_fixed_gpu_input():
    """The device's Δ differ from the reference's by the rounding of f64 sums and of lgamma / log1p: at these sizes the
    arguments of lgamma stay below about 1e5, so some tens of ulp over 2K + 2 terms are below 1e-7.  Exact equality of the
    labels is a fair demand of the device only if no decision of the reference is closer than that: a seed that violates it is
    replaced here, not tolerated there."""
    for name in R.CASES:
        _, runs, _ = R.host_ref(name)
        for q, run in enumerate(runs):
            print(name, q, run["min_gap"])
            assert run["min_gap"] > 1e-6, (name, q)


def test_fixed_inputs_cover_what_they_claim():
    c, runs, _ = R.host_ref("n130")
    assert runs[4]["K"] < 64 and len(np.unique(c["init"][4])) == 130     # the singletons start crosses 64 slots and empties most
    assert all(x["K"] == 3 for x in R.host_ref("maxK3")[1]) and runs[0]["K"] > 3
    cap = R.host_ref("capped")[1][0]
    assert cap["K"] == 1024 and cap["capped"] == 76
    big = R.host_ref("n1025")[1][0]
    assert big["sweeps"] == 2 and not big["converged"]
    assert R.host_ref("diag")[2].Dq.diagonal().all()
    assert any(x["moves"] > 0 for x in R.host_ref("norep")[1])


def test_the_kernels_lgamma_and_log1p_against_libm(tmp_path):
    """lgamma_pos and log1p_lean (csrc/mapmath.inc.hpp) are host functions too: the header is compiled here with the host
    compiler — the one the oracle is built with — and compared with libm over the range the search uses: relative error of a few
    ulp of the result or of the dominating product (y − ½)·log y."""
    prog = tmp_path / "lg.cpp"
    prog.write_text("#include <cmath>\n#include <cstdio>\n#define __host__\n#define __device__\nusing std::log;\n"
                    f"#include \"{os.path.join(ROOT, 'redclust.jl_amd', 'csrc', 'mapmath.inc.hpp')}\"\n"
                    "int main(){double x; while (scanf(\"%lf\", &x) == 1) printf(\"%.17g %.17g\\n\", x > 0 ? lgamma_pos(x) : 0.0, log1p_lean(x));}\n")
    exe = tmp_path / "lg"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-o", str(exe), str(prog)])
    g = np.random.default_rng(1)
    xs = np.concatenate([10.0 ** g.uniform(-3, 8, 4000), [0.5, 1.0, 2.0, 15.999, 16.0, 8.0 + 3.0 * 8192 * 8192]])
    out = subprocess.run([str(exe)], input="\n".join(repr(float(x)) for x in xs), capture_output=True, text=True, check=True).stdout.split()
    got = np.array(out, dtype=np.float64).reshape(-1, 2)
    for x, (lg, l1) in zip(xs, got):
        y = max(x, 16.0)
        scale = max(abs(math.lgamma(x)), (y - 0.5) * math.log(y))
        assert abs(lg - math.lgamma(x)) <= 8 * 2.0 ** -52 * scale, (x, lg, math.lgamma(x))
        assert abs(l1 - math.log1p(x)) <= 4 * 2.0 ** -52 * abs(math.log1p(x)), (x, l1)
    for x in (-0.5, -1e-9, 1e-17, 0.0, -0.999):
        o = subprocess.run([str(exe)], input=repr(x), capture_output=True, text=True, check=True).stdout.split()
        assert abs(float(o[1]) - math.log1p(x)) <= 4 * 2.0 ** -52 * abs(math.log1p(x)), x


# ---------------------------------------------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_julia_agree_on_rc_map_search():
    import test_oracle_cpu as T
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    ret, args = T._header_prototypes(hdr)["rc_map_search"]
    assert ret == "int32_t"
    assert args == ["rc_ctx*", "int32_t", "int64_t*", "int32_t*", "double*", "double*", "rc_params*", "int32_t", "int32_t", "int64_t*",
                    "void*", "int64_t*", "int64_t*", "int32_t*", "double*"]
    res, sig = rc.SIGNATURES["rc_map_search"]
    assert res is C.c_int32 and len(sig) == len(args)
    for k, (ct, py) in enumerate(zip(args, sig)):
        if ct == "int32_t":
            assert py is C.c_int32, (k, ct, py)
        else:
            assert py in (C.c_void_p, C.POINTER(_lib.RcParams), C.POINTER(C.c_double), C.POINTER(C.c_int32)), (k, ct, py)
    fields = T._header_structs(hdr)["rc_map_run_t"]
    ctype = {"double": C.c_double, "int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(nm, ctype[ty]) for nm, ty in fields] == list(_lib.RcMapRun._fields_)
    assert C.sizeof(_lib.RcMapRun) == 56
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    calls = [c for c in T._julia_ccalls(jl) if c[0] == "rc_map_search"]
    assert len(calls) == 1
    _, jret, jargs, npassed = calls[0]
    assert jret == "Int32" and len(jargs) == npassed == len(args)
    for jt, ct in zip(jargs, args):
        assert ct in T._JL2C[jt], (jt, ct)
    body = re.search(r"^struct RcMapRun\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jfields = [tuple(x.strip() for x in f.split("::")) for line in body.splitlines() for f in line.split("#")[0].split(";") if f.strip()]
    assert [(nm, T._JLFIELD2C[ty]) for nm, ty in jfields] == fields
    assert re.search(r"function searchmapestimate\(b::HIPBackend, data::MCMCData, candidates", jl) and "export searchmapestimate" in jl
    T.test_julia_glue_ccalls_match_the_header()


def test_the_source_is_part_of_the_build():
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    assert '#include "mapsearch.inc.hip"' in open(os.path.join(csrc, "redclust_hip.hip")).read()
    assert os.path.join(csrc, "mapsearch.inc.hip") in _lib._sources()    # build() watches it
    assert '#include "mapmath.inc.hpp"' in open(os.path.join(csrc, "redclust_hip.hip")).read()
    assert os.path.join(csrc, "mapmath.inc.hpp") in _lib._sources()
    src = re.sub(r"//.*", "", open(os.path.join(csrc, "mapsearch.inc.hip")).read())
    assert "asm" not in src                                              # plain C++ and vector memory operations only
    assert "greedy::Visit" in src and "greedy::group_argmin" in src and "greedy::offer_new" in src and "key_f64" in src
    assert "rc_map_search" in rc.SIGNATURES and callable(rc.searchmapestimate)


def test_python_argument_errors_need_no_device():
    import inspect
    sig = inspect.signature(rc.searchmapestimate)
    assert list(sig.parameters) == ["data_or_ctx", "candidates", "params", "r", "p", "nruns", "maxK", "maxsweeps", "seed", "init", "scores", "device"]
    assert [sig.parameters[k].default for k in ("nruns", "maxK", "maxsweeps", "seed", "init", "scores", "device")] == [16, 0, 100, 0, None, None, 0]
    assert inspect.signature(rc.hclustpointestimate).parameters["polish"].default is False
    with pytest.raises(ValueError, match="polish"):
        rc.hclustpointestimate(np.ones((3, 3), np.uint32), numsamples=1, polish=True)
