"""Register, scratch and LDS budgets of predict's kernels (csrc/predict.inc.hip), read from the gfx950 ISA the compiler emits
(hipcc cross-compiles without a GPU).  k_predict_sums runs as 1024-thread workgroups — 16 waves, four per SIMD — so a lane may
own at most 512 / 4 = 128 VGPRs or the kernel cannot be launched; its row is dynamic LDS (no static LDS), and the LDS variants
must gather it with 128-bit LDS reads (one read for both addends), the global variants with none.  k_predict_draw runs as
256-thread workgroups (one wave per SIMD: 512 VGPRs).  No kernel may touch scratch."""
import re
import pytest

from isa import listing


@pytest.fixture(scope="module")
def kernels():
    return {k: v for k, v in listing().items() if "3prd" in k and "k_predict" in k}


def test_every_instantiation_is_there(kernels):
    sums = sorted(m.group(1) + m.group(2) for m in (re.search(r"14k_predict_sumsILb(\d)ELb(\d)EE", k) for k in kernels) if m)
    assert sums == ["00", "01", "10", "11"], sorted(kernels)
    assert sum("14k_predict_draw" in k for k in kernels) == 1, sorted(kernels)


def test_no_kernel_spills_or_exceeds_the_launchable_registers(kernels):
    assert len(kernels) == 5
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == 0, name                   # the row is dynamic LDS, sized per call
        assert k["next_free_vgpr"] <= (128 if "k_predict_sums" in name else 512), name


def test_the_row_gather_is_one_128_bit_read_in_the_right_memory(kernels):
    for name, k in kernels.items():
        m = re.search(r"k_predict_sumsILb(\d)ELb(\d)EE", name)
        if not m:
            continue
        assert k["text"], name
        lds_reads = len(re.findall(r"\bds_read_b128\b", k["text"]))
        if m.group(1) == "1":
            assert lds_reads >= 1, name
            assert not re.search(r"\bds_read_b64\b", k["text"]), name       # not two 64-bit halves
        else:
            assert lds_reads == 0 and re.search(r"\bglobal_load_dwordx4\b", k["text"]), name
        atomics = len(re.findall(r"\bglobal_atomic_add_x2\b", k["text"]))
        assert (atomics >= 2) == (m.group(2) == "1"), (name, atomics)
