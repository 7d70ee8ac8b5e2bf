"""Register, scratch and LDS budgets of the large-n point-estimate search (csrc/pointsearch_large.inc.hip), read from the gfx950
ISA the compiler emits (hipcc cross-compiles without a GPU).  k_search_large<LOSS, Q4, PF> runs as one persistent 1024-thread
workgroup per run — 16 waves, four per SIMD — so a lane may own 512 / 4 = 128 VGPRs; PF, the part of the next row held in
registers, is chosen per instantiation so that none touches scratch.  lab, sz and the accumulator window are dynamic LDS and
must fit the 160 KiB of a CU beside the static reduction scratch at n = 32767."""
import os
import re

import pytest

from isa import SRC, listing

LARGE = os.path.join(os.path.dirname(SRC), "pointsearch_large.inc.hip")


@pytest.fixture(scope="module")
def kernels():
    return {re.search(r"k_search_largeILi(\d)ELi(\d)ELi(\d)EE", k).groups(): v for k, v in listing().items() if "k_search_large" in k}


def test_every_instantiation_fits_its_registers_without_scratch(kernels):
    assert sorted((l, q) for l, q, _ in kernels) == [(l, q) for l in "01" for q in "1248"], sorted(kernels)
    assert "__launch_bounds__(TPB)" in open(LARGE).read()
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["text"], name
        assert k["private_segment_fixed_size"] == 0 and not re.search(r"\bscratch_", k["text"]), name
        assert k["next_free_vgpr"] <= 128, name


@pytest.mark.parametrize("loss,per_slot", [("0", 4), ("1", 12)])
def test_the_lds_fits_a_cu_at_the_largest_n(kernels, loss, per_slot):
    """static + the largest dynamic carve at n = 32767: lab u16[32768], sz u16[32769], and the window in what is left of the
    budget — S u32[W], and L u64[W] for VI"""
    n, budget = 32767, 160 * 1024 - 1024
    fixed = 2 * 32768 + 2 * (n + 2) + 16
    W = (budget - fixed) // per_slot
    dynamic = (fixed + per_slot * W + 15) // 16 * 16
    src = open(LARGE).read()
    for piece in ("2 * (size_t)n4 + 2 * (size_t)(n + 2) + 16", "per_slot = vi ? 12 : 4", "(LDS_BUDGET - fixed) / per_slot"):
        assert piece in src, piece                                       # the carve this test restates
    assert W == {4: 7931, 12: 2643}[per_slot] and dynamic <= budget
    for name, k in kernels.items():
        if name[0] == loss:
            assert k["group_segment_fixed_size"] + dynamic <= 160 * 1024, (name, k["group_segment_fixed_size"], dynamic)
