"""Register, scratch and LDS budgets of the MAP-search kernel (csrc/mapsearch.inc.hip), read from the gfx950 ISA the compiler
emits (hipcc cross-compiles without a GPU).  k_mapsearch runs as one persistent 512-thread workgroup per run — 8 waves, two per
SIMD — so a lane may own at most 512 / 2 = 256 VGPRs or the kernel cannot be launched.  (1024 threads would leave a lane 128:
the f64 lgamma and log1p beside the cell arithmetic do not fit that without scratch, which is why it is 512.)  Its LDS is
dynamic — the slots of the points, the sizes, two generations of the per-slot (s, l) accumulators — and must fit the 160 KiB of
a CU at the largest n and slot cap; the accumulators are 64-bit integer LDS atomics, the block cells plain global loads and
stores.  Neither instantiation may touch scratch."""
import os
import re

import pytest

from isa import SRC, listing

TPB, LDS_MAX = 512, 160 * 1024
MAPSRC = os.path.join(os.path.dirname(SRC), "mapsearch.inc.hip")


@pytest.fixture(scope="module")
def kernels():
    return {k: v for k, v in listing().items() if "9mapsearch" in k and "k_mapsearch" in k}


def variant(name):
    """repulsion as "0" / "1" """
    return re.search(r"11k_mapsearchILb(\d)EE", name).group(1)


def test_every_instantiation_is_there(kernels):
    assert sorted(variant(k) for k in kernels) == ["0", "1"], sorted(kernels)


def test_no_kernel_spills_or_exceeds_the_launchable_registers(kernels):
    assert len(kernels) == 2
    src = open(MAPSRC).read()
    assert re.search(r"constexpr int TPB = 512\b", src) and "__launch_bounds__(TPB)" in src
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["text"], name
        assert k["private_segment_fixed_size"] == 0, name
        assert not re.search(r"\bscratch_", k["text"]), name
        assert k["next_free_vgpr"] <= 512 // (TPB // 64 // 4), name       # 8 waves on 4 SIMDs: two per SIMD, 256 VGPRs each


def test_the_lds_fits_a_cu_at_the_largest_sizes(kernels):
    """static + the largest dynamic carve: lab u16[8192], sz u16[1026], the accumulators u64[4][1025], the argmin's partials"""
    up16 = lambda x: (x + 15) // 16 * 16
    n, Kcap, nwave = 8192, 1024, 16
    dynamic = up16(4 * 8 * (Kcap + 1)) + up16(nwave * (8 + 4 + 4 + 4) + 8) + up16(2 * (Kcap + 2)) + up16(2 * n)
    src = open(MAPSRC).read()
    for piece in ("up16(4 * 8 * (size_t)(Kcap + 1))", "up16((size_t)NWAVE * (8 + 4 + 4 + 4) + 8)", "up16(2 * (size_t)(Kcap + 2))", "up16(2 * (size_t)n)"):
        assert piece in src, piece                                       # the carve this test restates
    for name, k in kernels.items():
        assert k["group_segment_fixed_size"] + dynamic <= LDS_MAX, (name, k["group_segment_fixed_size"], dynamic)
    assert dynamic == 51584


def test_the_accumulators_are_lds_atomics_and_the_cells_plain_memory(kernels):
    for name, k in kernels.items():
        assert len(re.findall(r"\bds_add_u64\b", k["text"])) >= 2, name   # s and l
        assert not re.findall(r"\b(global|flat)_atomic_\w+", k["text"]), name
