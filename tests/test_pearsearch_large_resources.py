"""Register, scratch and LDS budgets of the large-n PEAR search (k_pear_large of csrc/pointsearch_large.inc.hip) from the gfx950
ISA: one persistent 1024-thread workgroup per run leaves a lane 128 VGPRs, and head, lab, sz and the accumulator window must fit
the 160 KiB of a CU beside the static reduction scratch at n = 32767."""
import re

from isa import listing


def test_every_instantiation_fits_its_registers_and_the_largest_carve_a_cu():
    kernels = {m.groups(): v for k, v in listing().items() for m in [re.search(r"k_pear_largeILi(\d)ELi(\d)ELi(\d)EE", k)] if m}
    assert sorted(q for q, _, _ in kernels) == list("1248"), sorted(kernels)
    n, budget = 32767, 160 * 1024 - 1024
    fixed = 2 * 32768 + 2 * (n + 2) + 16 + 8 * 4                       # lab, sz, the carve's slack, and the head u64[4]
    W = (budget - fixed) // 4
    dynamic = (fixed + 4 * W + 15) // 16 * 16
    assert W == 7923 and dynamic <= budget
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["text"] and k["private_segment_fixed_size"] == 0 and not re.search(r"\bscratch_", k["text"]), name
        assert k["next_free_vgpr"] <= 128, name
        assert k["group_segment_fixed_size"] + dynamic <= 160 * 1024, (name, k["group_segment_fixed_size"], dynamic)
