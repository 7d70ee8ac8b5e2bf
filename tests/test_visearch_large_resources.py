"""Register, scratch and LDS budgets of the large-n exact VI search (csrc/visearch_large.inc.hip) from the gfx950 ISA: one
1024-thread workgroup per run leaves a lane 128 VGPRs, and the largest carve must fit the 160 KiB of a CU beside the static
scratch.  And the builder of the split table's thresholds (csrc/gqsplit.inc.hpp) in a program of its own under ASan / UBSan."""
import os
import re
import subprocess

import pytest

from isa import listing
from test_hostmodel_cpu import SANITIZE

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kernels():
    return {m.groups(): v for k, v in listing().items() for m in [re.search(r"k_vilarge(_groups)?ILi(\d)EE", k)] if m}


def test_every_instantiation_fits_its_registers_without_scratch(kernels):
    assert set(kernels) == {(k, q) for k in (None, "_groups") for q in "014"}, list(kernels)
    for name, k in kernels.items():
        assert k["text"], name
        assert k["private_segment_fixed_size"] == 0 and not re.search(r"\bscratch_", k["text"]), name
        assert k["next_free_vgpr"] <= 128, name


def test_the_lds_fits_a_cu_at_the_largest_sizes(kernels):
    """n = 32767, Kcap = 1024, PQ = 4: lo u32[n+1], acc u64[kpad], the partials, sz u16[Kcap+2], the stage u16[2][1024·4]"""
    up16 = lambda x: (x + 15) // 16 * 16
    dynamic = up16(4 * 32768) + up16(8 * 1024) + up16(16 * 28) + up16(2 * 1026) + up16(2 * 2 * 1024 * 4)
    assert dynamic == 158160
    for name, k in kernels.items():
        assert k["group_segment_fixed_size"] + dynamic <= 160 * 1024, (name, k["group_segment_fixed_size"])


def test_the_threshold_builder_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "gqsplit_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "gqsplit_host.cpp")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:
        print("built without the sanitizers")
        subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "thresholds 1 3 7 20 55 148 403 1097 2981 8103 22026" in out.stdout
