"""The planner of k_bulk_syml2's unit lists (csrc/s2plan.inc.hpp) in a program of its own, tests/s2plan_host.cpp: compiled with the
host compiler under AddressSanitizer and UndefinedBehaviorSanitizer (without them where their runtimes are missing) and run as an
ordinary executable.  The program checks every plan by brute force for n = 1, 7, 8, 127, 128, 129, 135, 1000, 2561, 8192, for 4,
512 and 768 resident blocks, with the unit length searched and fixed at 24 rows; the hashes of the plans it prints are held
against tests/golden/s2_plans.json, recorded from the list building as it stood inside build_syml2_lists before the planner
became a header of its own."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]


def test_unit_plans_cover_the_triangle_and_match_the_recorded_ones(tmp_path):
    exe = str(tmp_path / "s2plan_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "s2plan_host.cpp")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:
        print("built without the sanitizers")
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2] == "ok 60", (r.stdout[-2000:], r.stderr)
    got = {}
    for line in lines[:-2]:
        tag, n, cap, sw, h = line.split()
        assert tag == "plan"
        got[f"{n},{cap},{sw}"] = h
    with open(os.path.join(HERE, "golden", "s2_plans.json")) as f:
        want = json.load(f)
    assert len(want) == 60
    assert got == want, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
