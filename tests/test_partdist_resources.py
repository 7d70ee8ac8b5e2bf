"""Register, scratch and LDS budgets of the partition-distance kernel (csrc/partdist.inc.hip), read from the gfx950 ISA the
compiler emits (hipcc cross-compiles without a GPU).  k_partdist runs as 512-thread workgroups — 8 waves, two per SIMD — so a
lane may own at most 512 / 2 = 256 VGPRs or the kernel cannot be launched; three workgroups share a CU at n = 8192 (48 KiB of
LDS each), six waves per SIMD, which needs no more than 80.  Its LDS is dynamic (the sample's order, sized per call, and the
histograms).  The LDS variant counts with returning LDS atomics and touches global memory with plain loads and stores only; the
global variant counts and clears with global atomics and has no LDS atomic.  Neither may touch scratch."""
import re
import pytest

from isa import listing


@pytest.fixture(scope="module")
def kernels():
    return {k: v for k, v in listing().items() if "8partdist" in k and "k_partdist" in k}


def variant(name):
    """(histograms in global memory, Gq copied to LDS) as "0" / "1" each"""
    return re.search(r"10k_partdistILb(\d)ELb(\d)EE", name).groups()


def test_every_instantiation_is_there(kernels):
    assert sorted(variant(k) for k in kernels) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(kernels)


def test_no_kernel_spills_or_exceeds_the_launchable_registers(kernels):
    assert len(kernels) == 4
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["private_segment_fixed_size"] == 0, name
        assert not re.search(r"\bscratch_", k["text"]), name
        assert k["group_segment_fixed_size"] == 0, name                   # the order and the histograms are dynamic LDS
        assert k["next_free_vgpr"] <= 256, name                           # what 512 threads can launch with
        assert k["next_free_vgpr"] <= 80, name                            # ... and three workgroups per CU


def test_the_histogram_atomics_are_in_the_right_memory(kernels):
    for name, k in kernels.items():
        assert k["text"], name
        lds_atomics = len(re.findall(r"\bds_add_rtn_u32\b", k["text"]))
        global_atomics = len(re.findall(r"\bglobal_atomic_\w+", k["text"]))
        flat_atomics = len(re.findall(r"\bflat_atomic_\w+", k["text"]))
        print(name, lds_atomics, global_atomics, flat_atomics)
        assert flat_atomics == 0, name                                    # the address space is known at compile time
        if variant(name)[0] == "0":
            assert lds_atomics >= 1 and global_atomics == 0, name
        else:
            assert lds_atomics == 0 and re.search(r"\bglobal_atomic_add\b", k["text"]) and re.search(r"\bglobal_atomic_swap\b", k["text"]), name
        # Gq: 64-bit LDS reads where it was copied, none where it was not (the order is read as u16, the histograms as u32)
        assert bool(re.search(r"\bds_read_b64\b", k["text"])) == (variant(name)[1] == "1"), name
