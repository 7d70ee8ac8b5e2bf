"""The gfx950 ISA the compiler emits for the whole translation unit (hipcc cross-compiles without a GPU), compiled once per test
process and shared by every module that reads kernel resources or instructions from it."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "redclust.jl_amd", "csrc", "redclust_hip.hip")
KEYS = ("next_free_vgpr", "group_segment_fixed_size", "private_segment_fixed_size")


@functools.lru_cache(maxsize=None)
def listing():
    """{kernel symbol: its three .amdhsa_ numbers (KEYS) and "text", the lines after its label up to .Lfunc_end}"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tempfile.mkdtemp(prefix="rc_isa_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, "rc.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC],
                   check=True, cwd=os.path.dirname(SRC), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    texts, res, label, body, name, cur = {}, {}, None, None, None, {}
    for line in open(out):
        if body is None:
            m = re.match(r"([A-Za-z_]\w*):", line)
            if m:
                label, body = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            texts[label] = "".join(body); body = None
        else:
            body.append(line)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name, cur = m.group(1), {}
        for key in KEYS:
            m = re.match(r"\s*\.amdhsa_" + key + r"\s+(\d+)", line)
            if m and name:
                cur[key] = int(m.group(1))
        if ".end_amdhsa_kernel" in line and name:
            res[name] = cur; name = None
    return {k: dict(v, text=texts.get(k, "")) for k, v in res.items()}    # (.Lfunc_end follows the kernel's .amdhsa_ block)


def resources(pattern=""):
    """the numbers alone (no text: they are printed when an assertion fails) of the kernels whose symbol matches pattern"""
    return {k: {key: v[key] for key in KEYS} for k, v in listing().items() if re.search(pattern, k)}


def one(d, fragment):
    hits = [k for k in d if fragment in k]
    assert len(hits) == 1, (fragment, hits)
    return d[hits[0]]
