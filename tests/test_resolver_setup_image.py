"""The end of a stationary sweep is known when the resolver's first grid barrier releases (DESIGN.md §3 "Grid barrier"): "some
block announced a changer in this pass" rides in the barrier's arrivals, and "nobody did" ends the sweep without the pass over
the chunk words.  A lost announcement would lose a move, so the sweeps here have exactly ONE changer, in a chunk of the first
block, of another block and of the last block.  n = 96 / 257: 3 / 9 chunks of 32 points on as many blocks, the last chunk of 257
one point wide.  (The packed set-up image for the resolver's prologue, which this file was also meant for, did not move the
prologue's time and was taken out again with its option and tests: DESIGN.md §3 "Which limit a change moves".)"""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as O
import redclust_amd as rc
from isa import one, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "redclust.jl_amd", "csrc", "redclust_hip.hip")
RESLAYOUT = os.path.join(ROOT, "redclust.jl_amd", "csrc", "reslayout.inc.hpp")


@pytest.fixture(scope="module")
def separated():
    out = {}

    def get(n):
        if n not in out:
            d = rc.generatemixture(n, 3, seed=103 + n, sigma=0.05)
            D, truth = d["distancematrix"], d["clusts"].astype(np.int64)
            out[n] = (D, truth, rc.likelihood_hyperparams(D, truth))
        return out[n]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["full", "incremental"])
@pytest.mark.parametrize("n", [96, 257])
@pytest.mark.parametrize("where", ["first chunk", "other block", "last chunk"])
def test_single_changer(separated, n, where, mode):
    """Well-separated data, the generating labels with ONE point mislabelled: the sweep moves exactly that point back, as the
    oracle does, and the next sweeps change nothing and end in their first round (n_rounds = 1, what a sweep without changes
    reported before the barrier carried the flag)."""
    D, truth, P = separated(n)
    x = {"first chunk": 5, "other block": 40, "last chunk": n - 1}[where]
    init = truth.copy()
    init[x] = truth[x] % 3 + 1
    orc = O.Oracle(D, P)
    orc.set_state(init)
    ctx = rc.Context(D, logD=orc.logD)
    ctx.set_params(**P); ctx.set_mode(mode); ctx.set_state(init)
    ctx.gibbs_sweep(1.0, 0.5, 11, 0)
    orc.sweep_stable(1.0, 0.5, 11, 0)
    s = ctx.sweep_stats()
    assert orc.last_changes == 1 and np.array_equal(orc.clusts, truth)       # (what the scenario is built to be)
    assert s["n_changes"] == 1, s
    assert np.array_equal(ctx.get_state()[0], orc.clusts), where
    for t in (1, 2, 3):
        ctx.gibbs_sweep(1.0, 0.5, 11, t, blocking=bool(t & 1))
        orc.sweep_stable(1.0, 0.5, 11, t)
        s = ctx.sweep_stats()
        assert orc.last_changes == 0 and s["n_changes"] == 0 and s["n_rounds"] == 1, (t, s)
        assert np.array_equal(ctx.get_state()[0], truth), t
    # ... and a changer announced AFTER sweeps that ended at the barrier (counters re-armed, both generations used)
    again = truth.copy()
    again[x] = truth[x] % 3 + 1
    ctx.set_state(again); orc.set_state(again)
    for t in (4, 5):
        ctx.gibbs_sweep(1.0, 0.5, 11, t)
        orc.sweep_stable(1.0, 0.5, 11, t)
        assert ctx.sweep_stats()["n_changes"] == orc.last_changes == (1 if t == 4 else 0), t
        assert np.array_equal(ctx.get_state()[0], orc.clusts), t
    ctx.close()


def test_resolver_keeps_its_registers():
    assert one(resources("k_resolve"), "k_resolve4View")["next_free_vgpr"] <= 128


def test_resolver_has_no_scratch():
    """k_resolve had 212 bytes of scratch at its 128 registers: 53 dwords of per-thread values the compiler hoisted out of the
    round loop (LDS addresses, lane masks, 64-bit offsets), stored in the prologue and reloaded inside the rounds.  The
    resolver's code now reads the thread index through rc_tid(), which the optimiser cannot see through, so those values are
    recomputed where they are used and nothing is spilled."""
    assert one(resources("k_resolve"), "k_resolve4View")["private_segment_fixed_size"] == 0


# tab_bytes(kcap, n, waves per block, batch capacity) before the barrier carried the flag (bytes of dynamic LDS)
TAB_BYTES = {(64, 8192, 4, 512): 24160, (128, 8192, 4, 512): 26912, (256, 32768, 4, 512): 32928, (2047, 1000, 8, 512): 110144,
             (4096, 8192, 8, 64): 153040, (37, 257, 1, 512): 20064}


def test_tab_bytes_did_not_grow():
    """The resolver's dynamic LDS (tab_layout of csrc/reslayout.inc.hpp, compiled here as host code) is what it was — the announcement flag lives in a
    spare misc word — and the headline's tables still fit 39 KiB beside three reduction blocks."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    assert '#include "reslayout.inc.hpp"' in open(SRC).read()
    prog = ('#include <cstdio>\n#define __host__\n#define __device__\n#include "' + RESLAYOUT + '"\n'
            "int main() { size_t off[RC_TAB_NOFF];\n" +
            "".join(f'  std::printf("%zu\\n", tab_layout({k}, {n}, {nw}, off, {mb}));\n' for (k, n, nw, mb) in TAB_BYTES) + "  return 0; }\n")
    tmp = tempfile.mkdtemp(prefix="rc_tab_")
    try:
        with open(os.path.join(tmp, "t.cpp"), "w") as f:
            f.write(prog)
        subprocess.run([cxx, "-std=c++17", "-O0", "-o", os.path.join(tmp, "t"), os.path.join(tmp, "t.cpp")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(tmp, "t")], check=True, capture_output=True, text=True).stdout.split()]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert got == list(TAB_BYTES.values()), dict(zip(TAB_BYTES, got))
    assert got[0] <= 39 * 1024 and got[1] <= 39 * 1024
