"""Register, scratch and LDS budgets of the large-n hierarchical point estimates (csrc/hclust_large.inc.hip) from the gfx950 ISA:
k_hclust_large<LINK> is one 1024-thread workgroup and k_eloss_large<EGT> runs 1024-thread workgroups, so a lane has 128 VGPRs;
neither may touch scratch, and the largest carve must fit the 160 KiB of a CU beside the static reduction scratch."""
import re

import pytest

from isa import listing


@pytest.fixture(scope="module")
def kernels():
    return {m.groups(): v for k, v in listing().items() for m in [re.search(r"3hcl\d+k_(hclust|eloss)_largeILi(\d)EE", k)] if m}


def test_every_instantiation_fits_its_registers_without_scratch(kernels):
    assert set(kernels) == {("hclust", l) for l in "012"} | {("eloss", g) for g in "1248"}, list(kernels)
    for name, k in kernels.items():
        print(name, {key: k[key] for key in k if key != "text"})
        assert k["private_segment_fixed_size"] == 0 and not re.search(r"\bscratch_", k["text"]), name
        assert k["next_free_vgpr"] <= 128, name


def test_the_lds_fits_a_cu_at_n_32767(kernels):
    """part u16[32768], sz u16[32768], rescan u32[1024], dirty u8[1024]; two labellings of 32767 u16 for the expected loss"""
    dynamic = 2 * 32768 + 2 * 32768 + 4 * 1024 + 1024
    assert dynamic == 136192
    for name, k in kernels.items():
        assert k["group_segment_fixed_size"] + (dynamic if name[0] == "hclust" else 2 * 32767 * 2) <= 160 * 1024, name
