"""Budgets of the large-n exact ID search (k_idlarge of csrc/visearch_large.inc.hip) from the gfx950 ISA: one 1024-thread workgroup
per run leaves a lane 128 VGPRs, and both placements of F's table must fit a CU's 160 KiB beside the carve and the static LDS."""
import re

from isa import listing


def test_every_instantiation_fits_its_registers_and_both_table_placements_a_cu():
    """n = 32767, Kcap = 1024.  m = 2048, PQ = 4: the carve, 16 B for Aq, the fence i64[m >> s] at the host's s — the smallest that
    fits beside the static LDS it counts (STATIC_L = 144).  m = 1024, PQ = 1: the carve and 16·(m + 1) B."""
    kernels = {m.group(1): v for k, v in listing().items() for m in [re.search(r"k_idlargeILi(\d)EE", k)] if m}
    assert set(kernels) == set("014"), list(kernels)
    up16 = lambda x: (x + 15) // 16 * 16
    carve = lambda pq: up16(4 * 32768) + up16(8 * 1024) + up16(16 * 28) + up16(2 * 1026) + up16(2 * 2 * 1024 * pq)
    s = next(s for s in range(13) if carve(4) + 16 + 8 * (2048 >> s) <= 160 * 1024 - 144)
    fenced, whole = carve(4) + 16 + 8 * (2048 >> s), carve(1) + 16 * 1025
    assert (carve(4), carve(1), s, fenced, whole) == (158160, 145872, 2, 162272, 162272)
    for name, k in kernels.items():
        assert k["text"] and k["private_segment_fixed_size"] == 0 and not re.search(r"\bscratch_", k["text"]), name
        assert k["next_free_vgpr"] <= 128, name
        assert k["group_segment_fixed_size"] <= 144 and k["group_segment_fixed_size"] + max(fenced, whole) <= 160 * 1024, name
