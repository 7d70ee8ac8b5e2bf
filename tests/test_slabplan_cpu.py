"""The planner of the slab driver's chunks (csrc/slabplan.inc.hpp) in a program of its own, tests/slabplan_host.cpp: compiled with
the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer (without them where their runtimes are missing) and run as
an ordinary executable.  The program plans the chunks of rc_score_labellings, rc_cluster_profiles, rc_predict (q = 1, 3, 600, without
and with the optional columns) and rc_predict_joint for n = 1, 65, 257, 8192, for 1, 3, 65, 1025 labellings of 1, min(n, 4096) or
alternately 1 and sqrt(n) clusters, in workspaces of 4 KiB, 64 KiB, 1 MiB and 1 GiB, and checks every chunk by brute force; the
(labellings, rows) sequences it prints, run-length encoded, are held against tests/golden/slab_plans.json, recorded from the four
loops as they stood in the entry points before the planner became a header of its own (the joint predict's loop cut no rows: its
recorded rows are min(q, workspace / Σ 16 K), which that entry point does not use)."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]
CASES = 4 * 4 * 3 * 4 * (2 + 3 * 3)


def test_chunk_plans_fit_their_workspace_and_match_the_recorded_ones(tmp_path):
    exe = str(tmp_path / "slabplan_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "slabplan_host.cpp")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:
        print("built without the sanitizers")
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2] == f"ok {CASES}", (r.stdout[-2000:], r.stderr)
    got = {}
    for line in lines[:-2]:
        tag, key, plan = line.split()
        assert tag == "plan"
        got[key] = plan
    with open(os.path.join(HERE, "golden", "slab_plans.json")) as f:
        want = json.load(f)
    assert len(want) == CASES
    assert got == want, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))[:20]
    # the case of the GPU tests of the plain-store path: 1025 labellings of n = 65 points are one chunk of all 65 rows
    # at every number of clusters, so whatever their labellings are
    for entry in ("score", "profiles"):
        for pattern in range(3):
            assert want[f"{entry},65,1025,{pattern},1048576"] == "1025:65*1"
