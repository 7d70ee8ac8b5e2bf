"""The model's host statistics as the library ships them (csrc/hostmodel.inc.hpp: loglik from block sums, logprior, the whole
split–merge proposal) in a program of their own, tests/hostmodel_host.cpp: compiled with the host compiler under AddressSanitizer
and UndefinedBehaviorSanitizer (without them where their runtimes are missing) and run as an ordinary executable on a case file
written here.  Every proposal of a walk in "intended" semantics — 25 iterations × 2 proposals, r = 1.0, p = 0.5, numGibbs = 5,
n = 100: the arguments of test_gpu_parity.py::test_splitmerge_intended_mode_and_runsampler_defaults — is held against
O.Oracle.mh_proposal(mode=1) on the same sequence: flags, labels and K exactly, the log-likelihood before the proposal, the
log-prior after it and the two log-ratios within the tolerances the GPU tests and test_splitmerge_cpu.py use for them."""
import functools
import os
import subprocess

import numpy as np
import pytest

import np_transcription as T
import oracle_lib as O
from helpers import load_golden
from redclust_amd._lib import _params_struct
from test_gpu_parity import LL_RTOL
from test_splitmerge_cpu import MH_CASES, mh_case

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "redclust.jl_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]
R, PP, NUM_GIBBS, ITERS, NMH = 1.0, 0.5, 5, 25, 2
LP_RTOL = 1e-12      # ctx.logprior against orc.logprior in test_gpu_parity.py::test_golden_sweeps
RATIO_RTOL = 1e-7    # the proposal's log-ratios between oracle and transcription, test_splitmerge_cpu.py
CASES = MH_CASES + ["halved", "d3_merged_maxK"]


@functools.lru_cache(maxsize=None)
def case(tag):
    """(D, P, start labels, seed)"""
    if tag == "halved":     # paper dataset 1, every true cluster cut in two at random: merges get accepted
        _, d = load_golden()
        D, truth = d["D1"], d["labels1"].astype(np.int64)
        cut = truth + len(np.unique(truth)) * np.random.default_rng(101).integers(0, 2, len(truth))
        init = np.unique(cut, return_inverse=True)[1].astype(np.int64) + 1
        assert len(np.unique(init)) == 20
        return D, T.likelihood_hyperparams(D, truth), init, 5
    if tag == "d3_merged_maxK":   # no split once K is at maxK: proposals are skipped
        _, D, P, init, seed = mh_case("d3_merged")
        assert len(np.unique(init)) == 7
        return D, dict(P, maxK=7), init, seed
    _, D, P, init, seed = mh_case(tag)
    return D, P, init, seed


@functools.lru_cache(maxsize=None)
def oracle_walk(tag):
    """per proposal: the oracle's log-likelihood before it, its OrcMHInfo, and labels, K and log-prior after it"""
    D, P, init, seed = case(tag)
    orc = O.Oracle(D, P)
    orc.set_state(init)
    out = []
    for it in range(ITERS):
        for mh in range(NMH):
            ll = orc.loglik_stable()
            inf = orc.mh_proposal(R, PP, NUM_GIBBS, seed, it, mh, mode=1)   # replaces the oracle's state on acceptance
            out.append(dict(ll=ll, flags=(int(inf.accept), int(inf.split), int(inf.skipped)), lpr=inf.log_prior_ratio,
                            lprop=inf.log_proposal_ratio, clusts=orc.clusts.copy(), K=orc.K, lp=orc.logprior(R, PP)))
    return orc, out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("hostmodel") / "hostmodel_host")
    # (-Wno-unknown-pragmas: philox.inc.hpp keeps its "#pragma unroll" for the device compiler)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", path,
           os.path.join(HERE, "hostmodel_host.cpp")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:
        print("built without the sanitizers")
        subprocess.check_call(cmd)
    return path


def test_the_walks_reach_every_path():
    """a condition on the inputs: a comparison that never reaches a path cannot pass"""
    flags = [w["flags"] for tag in CASES for w in oracle_walk(tag)[1]]
    for accept, split in ((1, 1), (1, 0), (0, 1), (0, 0)):
        assert any(f == (accept, split, 0) for f in flags), (accept, split)
    assert any(f[2] == 1 for f in flags)


@pytest.mark.parametrize("tag", CASES)
def test_proposals_match_the_oracle(exe, tmp_path, tag):
    D, P, init, seed = case(tag)
    orc, want = oracle_walk(tag)
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        np.array([len(init), NUM_GIBBS, seed, ITERS, NMH, orc.eD, orc.eL], np.int64).tofile(f)
        np.array([R, PP], np.float64).tofile(f)
        np.frombuffer(bytes(_params_struct(P)), np.uint8).tofile(f)
        for a in (orc.D, orc.logD, orc.Dq, orc.Lq, init.astype(np.int64)):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2] == f"ok {ITERS * NMH}", (r.stdout[-2000:], r.stderr[-4000:])
    assert len(lines) == ITERS * NMH + 2
    worst = {"ll_cur": 0.0, "logprior": 0.0, "log_prior_ratio": 0.0, "log_proposal_ratio": 0.0}

    def close(name, x, y, rtol, where):
        if np.isnan(x) and np.isnan(y):
            return
        worst[name] = max(worst[name], abs(x - y) / max(1.0, abs(y)))
        assert x == y or abs(x - y) <= rtol * max(1.0, abs(y)), (name, where, x, y)

    for q, (line, w) in enumerate(zip(lines, want)):
        tok = line.split()
        where = (tag, q // NMH, q % NMH)
        assert tok[0] == "p" and len(tok) == 9 + len(init), where
        assert tuple(int(t) for t in tok[1:4]) == w["flags"], where
        assert int(tok[8]) == w["K"] and np.array_equal(np.array(tok[9:], np.int64), w["clusts"]), where
        close("log_prior_ratio", float(tok[4]), w["lpr"], RATIO_RTOL, where)
        close("log_proposal_ratio", float(tok[5]), w["lprop"], RATIO_RTOL, where)
        close("ll_cur", float(tok[6]), w["ll"], LL_RTOL, where)
        close("logprior", float(tok[7]), w["lp"], LP_RTOL, where)
    print(tag, "largest relative differences:", worst)


def test_the_translation_unit_includes_the_headers():
    src = open(os.path.join(CSRC, "redclust_hip.hip")).read()
    assert '#include "hostmodel.inc.hpp"' in src and '#include "philox.inc.hpp"' in src
