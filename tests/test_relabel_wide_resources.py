"""Register, scratch and LDS budgets of k_relabel_wide (csrc/relabel_wide.inc.hip), read from the gfx950 ISA the compiler emits.
It runs as one workgroup of 1024 threads per CU — sixteen waves, four per SIMD — so a lane may own 128 VGPRs at the most, and its
LDS is a small static part plus the dynamic carve that the source states in one place, restated here."""
from isa import one, resources


def test_registers_scratch_and_lds_fit_one_workgroup_of_1024_threads():
    k = one(resources("k_relabel_wide"), "14k_relabel_wide")
    print(k)
    assert k["next_free_vgpr"] <= 128
    assert k["private_segment_fixed_size"] == 0
    # the carve at 4096 columns: cw = 4097 rounded up to 8; rowptr and rownnz u16[cw], sixteen 64-bit partial minima, and the
    # overlay, whose largest tenant is the sixteen waves' dense u16 rows of the table's construction (n does not enter: the
    # points' column ids and the table's entries are in global slabs, 6 bytes a point)
    cw = (4096 + 1 + 7) // 8 * 8
    carve = 2 * 2 * cw + 16 * 8 + 16 * 2 * cw
    assert carve == 147872 and k["group_segment_fixed_size"] + carve <= 160 * 1024
