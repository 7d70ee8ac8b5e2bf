"""Register, scratch and LDS budgets of the relabelling kernel (csrc/relabel.inc.hip), read from the gfx950 ISA the compiler
emits (hipcc cross-compiles without a GPU).  k_relabel runs as 256-thread workgroups — 4 waves, one per SIMD — so a lane may own
up to 512 VGPRs before the kernel cannot be launched; eight workgroups share a CU when the tables are small, eight waves per
SIMD, which needs no more than 64 (asked of the LDS-table variant; the global-table variant holds a row's cells in registers and
runs one workgroup per CU at the most).  Its LDS is dynamic (the assignment's vectors and the table, sized per launch).  The
LDS-table variant counts the table with non-returning LDS atomics and has one global atomic, the count of phase 3; the
global-table variant counts the table with a global atomic too and has no LDS atomic.  Neither may touch scratch."""
import re
import pytest

from isa import listing


@pytest.fixture(scope="module")
def kernels():
    return {k: v for k, v in listing().items() if "7relabel" in k and "k_relabel" in k}


def variant(name):
    """the table in global memory: "0" / "1" """
    return re.search(r"9k_relabelILb(\d)EE", name).group(1)


def test_every_instantiation_is_there(kernels):
    assert sorted(variant(k) for k in kernels) == ["0", "1"], sorted(kernels)


def test_no_kernel_spills_or_exceeds_the_launchable_registers(kernels):
    assert len(kernels) == 2
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["private_segment_fixed_size"] == 0, name
        assert not re.search(r"\bscratch_", k["text"]), name
        assert k["group_segment_fixed_size"] == 0, name                   # the vectors and the table are dynamic LDS
        assert k["next_free_vgpr"] <= 512, name                           # what 256 threads can launch with
        # the LDS variant: eight workgroups per CU, eight waves per SIMD; the slab variant, whose grid is capped at one workgroup
        # per CU and which keeps a row's cells in registers: four waves per SIMD
        assert k["next_free_vgpr"] <= (64 if variant(name) == "0" else 128), name


def test_the_table_atomics_are_in_the_right_memory(kernels):
    assert len(kernels) == 2
    for name, k in kernels.items():
        assert k["text"], name
        lds_atomics = len(re.findall(r"\bds_add_u32\b", k["text"]))
        lds_returning = len(re.findall(r"\bds_add_rtn_u32\b", k["text"]))
        global_atomics = len(re.findall(r"\bglobal_atomic_\w+", k["text"]))
        flat_atomics = len(re.findall(r"\bflat_atomic_\w+", k["text"]))
        print(name, lds_atomics, lds_returning, global_atomics, flat_atomics)
        assert flat_atomics == 0 and lds_returning == 0, name             # the address space is known; no count is read back
        if variant(name) == "0":
            assert lds_atomics == 1 and global_atomics == 1, name         # phase 1 in LDS; the one global atomic is phase 3's
        else:
            assert lds_atomics == 0 and global_atomics == 2, name
        assert len(re.findall(r"\bglobal_atomic_add\b", k["text"])) == global_atomics, name
        assert not re.search(r"\bv_(add|mul|fma|cvt)_f(16|32|64)\b", k["text"]), name      # integers only
