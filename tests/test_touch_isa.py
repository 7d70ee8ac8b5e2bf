"""Static checks of the L2 warm-up touches in k_bulk_syml2<true, true>, read from the gfx950 ISA the compiler emits (hipcc
cross-compiles without a GPU).

A touch is a load whose value nothing reads.  Left to itself its destination is a free register that the next VALU result
takes, and the compiler then puts a wait for the touch — with the in-order counter: for every row requested before it — in
front of that instruction.  syml2_fast keeps the value alive to a never-true store at its end, so that the touches share one
register that only the next touch rewrites.  Nothing in the language guarantees that allocation; these checks are what notices
when a compiler stops making it:
  * the kernel still fits the 128 registers beside the resolver, without scratch, in its 39 936 bytes of LDS;
  * the touches are plain dword loads (no nt, no sc bits: they must fill L2) and those of the steady loop share one destination;
  * the kernel has no more vmcnt waits than the listing this was written against (26: every one of them a row take, a slot
    read or a flush; a wait per touch would add one per touch site).  A failure here after a compiler update means: read the
    listing, not: raise the number.
k_bulk_syml2w and the stored form carry no touches: no plain dword load in their steady loops beyond the parent's slot reads."""
import collections
import re

import isa

FOLDED = "k_bulk_syml2ILb1ELb1E"
WAITS_WITHOUT_TOUCH_WAITS = 26


def loop_dword_loads(text):
    """(destination, line) of every global_load_dword (one dword) in the innermost loop (blocks the listing marks Depth=3)"""
    out, depth = [], 0
    for line in text.split("\n"):
        if re.match(r"^(\.LBB\S+:|; %bb\.\d+:)", line):
            d = re.search(r"Depth=(\d)", line)
            depth = int(d.group(1)) if d else 0
        m = re.match(r"\s+global_load_dword\s+(v\d+),", line)
        if m and depth == 3:
            out.append((m.group(1), line.strip()))
    return out


def test_folded_kernel_resources():
    k = isa.one(isa.listing(), FOLDED)
    assert k["next_free_vgpr"] <= 128 and k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 39936, \
        {key: k[key] for key in isa.KEYS}


def test_touches_share_one_register_and_fill_l2():
    k = isa.one(isa.listing(), FOLDED)
    loads = loop_dword_loads(k["text"])
    assert all(re.search(r"\boff$", line) for _, line in loads), loads          # no cache bits behind the address
    by_dest = collections.Counter(d for d, _ in loads)
    dest, count = by_dest.most_common(1)[0]
    # four requests per 8-row group and one touch behind each; the two slot reads of the wave's next unit have their own registers
    assert count >= 3 and len(loads) - count <= 3, by_dest
    waits = len(re.findall(r"s_waitcnt[^\n]*vmcnt", k["text"]))
    assert waits <= WAITS_WITHOUT_TOUCH_WAITS, waits


def test_other_forms_carry_no_touches():
    L = isa.listing()
    for fragment in ("k_bulk_syml2wILb1ELb1E", "k_bulk_syml2wILb1ELb0E", "k_bulk_syml2ILb0ELb0E"):
        loads = loop_dword_loads(isa.one(L, fragment)["text"])
        assert len(loads) <= 2, (fragment, loads)                               # the next unit's two column-slot reads
