"""Register, scratch and LDS budgets of the large-n MAP search (k_map_large and k_map_cells of csrc/mapsearch_large.inc.hip) from
the gfx950 ISA: 512-thread workgroups leave a lane 256 VGPRs, and k_map_large's carve — mapsearch.inc.hip's Carve at the padded
n — must fit the 160 KiB of a CU at n = 32767 and 1024 slots."""
import re

from isa import listing


def test_every_instantiation_fits_its_registers_and_the_largest_carve_a_cu():
    large = {m.groups(): v for k, v in listing().items() for m in [re.search(r"k_map_largeILi(\d+)ELb(\d)ELb(\d)EE", k)] if m}
    cells = {m.groups(): v for k, v in listing().items() for m in [re.search(r"k_map_cellsILi(\d+)ELb(\d)EE", k)] if m}
    kinds = [("32", "1"), ("64", "0"), ("64", "1")]                      # (storage bits, log stored): a derived log is 64-bit
    assert sorted(large) == sorted(k + (rep,) for k in kinds for rep in "01") and sorted(cells) == kinds
    up16 = lambda x: (x + 15) // 16 * 16
    n, Kcap = 32767, 1024
    carve = up16(4 * 8 * (Kcap + 1)) + up16(16 * (8 + 4 + 4 + 4) + 8) + up16(2 * (Kcap + 2)) + up16(2 * ((n + 3) // 4 * 4))
    assert carve == 100736
    for name, k in {**large, **cells}.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["text"] and k["private_segment_fixed_size"] == 0 and not re.search(r"\bscratch_", k["text"]), name
        assert k["next_free_vgpr"] <= 256, name
        assert k["group_segment_fixed_size"] + carve <= 160 * 1024, (name, k["group_segment_fixed_size"])
