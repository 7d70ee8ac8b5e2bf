"""Register, scratch and LDS budgets of the joint predict's kernel (csrc/predictjoint.inc.hip), read from the gfx950 ISA the
compiler emits (hipcc cross-compiles without a GPU).  k_joint runs as 256-thread workgroups, one wave per SIMD, so a lane could
own 512 VGPRs and still launch — but a sample's workgroup is small and its CU should hold several (DESIGN.md §8 "Joint
predict"): at most 128 VGPRs keep four workgroups per CU launchable beside each other.  Its slots are dynamic LDS, sized per
launch; the static LDS is the four waves' argmax partials (8 + 3·4 bytes each) and two counters.  No scratch."""
import pytest

from isa import listing


@pytest.fixture(scope="module")
def kernels():
    return {k: v for k, v in listing().items() if "4prdj" in k}


def test_the_kernel_is_there_and_named_apart_from_predicts(kernels):
    assert len(kernels) == 1 and "7k_joint" in next(iter(kernels)), sorted(kernels)
    assert not any("k_predict" in k for k in kernels)                      # test_predict_resources.py counts those


def test_no_scratch_static_lds_as_declared_and_launchable_registers(kernels):
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["private_segment_fixed_size"] == 0, name
        declared = 4 * (8 + 3 * 4) + 2 * 4
        assert k["group_segment_fixed_size"] == -(-declared // 16) * 16, name   # rounded up to the dynamic part's alignment
        assert k["next_free_vgpr"] <= 128, name

