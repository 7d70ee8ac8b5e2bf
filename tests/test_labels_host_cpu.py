"""The host label toolkit (csrc/labels.inc.hpp) in a program of its own, tests/labels_host.cpp: compiled with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer (without them where their runtimes are missing) and run as an ordinary
executable.  The program checks compact_labels, dense_ids, cluster_order, count_clusters and find_bad_label against brute-force
restatements for n = 1, 2, 7, 64."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]


def test_label_toolkit_matches_its_restatement(tmp_path):
    exe = str(tmp_path / "labels_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "labels_host.cpp")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:
        print("built without the sanitizers")
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr)
