"""Static checks of k_bulk_syml2 with the exponent folded into its log table, read from the gfx950 ISA the compiler emits (hipcc
cross-compiles without a GPU), as tests/test_kernel_resources.py does:
  * the fallback for contexts over more than four binades, k_bulk_syml2w, keeps the three budgets of the kernel it was (128 registers,
    40 KiB of LDS, no scratch: three of its waves and one resolver wave share a SIMD);
  * the body of k_bulk_syml2<true, true> holds fewer int -> double conversions of the exponent (v_cvt_f64_i32) and fewer subtractions
    of the rounding bias (literal 0xbcc80000 = -bits(1.5·2^52) >> 32) than before the fold: 16 of each then (four entries x four row
    pairs, one copy of the row-pair block).  What remains: no conversion; four bias constants, one per row pair, inside the branch
    taken only by units with lanes that are not whole (their element-wise atomics), none in the streaming path."""
import pytest

from isa import listing, one, resources

PARENT_CVT_F64_I32 = 16        # k_bulk_syml2<true, true> before the fold
PARENT_BIAS_ADDS = 16


@pytest.fixture(scope="module")
def isa():
    """(every kernel's lines, every kernel's numbers)"""
    return {k: v["text"].splitlines() for k, v in listing().items()}, resources()


@pytest.mark.parametrize("fragment", ["k_bulk_syml2wILb1ELb1E", "k_bulk_syml2wILb1ELb0E"])
def test_fallback_kernel_keeps_the_budgets(isa, fragment):
    k = one(isa[1], fragment)
    assert k["next_free_vgpr"] <= 128, k
    assert k["group_segment_fixed_size"] <= 40960, k
    assert k["private_segment_fixed_size"] == 0, k


def test_folded_kernel_lost_the_exponent_conversions_and_bias_adds(isa):
    body = one(isa[0], "k_bulk_syml2ILb1ELb1E")
    cvt = sum("v_cvt_f64_i32" in ln for ln in body)
    bias = sum("0xbcc80000" in ln for ln in body)
    print("v_cvt_f64_i32:", cvt, "of", PARENT_CVT_F64_I32, " bias constants:", bias, "of", PARENT_BIAS_ADDS)
    assert len(body) > 1000                                # the whole kernel was read
    assert cvt < PARENT_CVT_F64_I32, cvt
    assert bias < PARENT_BIAS_ADDS, bias
    fb = one(isa[0], "k_bulk_syml2wILb1ELb1E")             # the fallback is the kernel as it was
    assert sum("v_cvt_f64_i32" in ln for ln in fb) == PARENT_CVT_F64_I32
    assert sum("0xbcc80000" in ln for ln in fb) == PARENT_BIAS_ADDS
