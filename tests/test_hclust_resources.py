"""Register and scratch budgets of the hierarchical point estimates' 1024-thread kernels (csrc/hclust.inc.hip), read from the
metadata of the gfx950 ISA the compiler emits (hipcc cross-compiles without a GPU): k_hclust<LINK> runs as ONE 1024-thread
workgroup and k_eloss as 1024-thread workgroups — 16 waves, four per SIMD — so a lane may own at most 512 / 4 = 128 VGPRs or
the kernel cannot be launched, and a scratch access inside k_hclust's step loop would sit between its barriers."""
import re
import pytest

from isa import resources


@pytest.fixture(scope="module")
def kernels():
    return resources(r"3hcl(8k_hclustILi\dEE|7k_eloss)")


def test_every_instantiation_is_there(kernels):
    # k_hclust<LINK> as the Itanium ABI mangles it: 8k_hclustILi<LINK>EE; k_eloss is no template
    assert sorted(m.group(1) for m in (re.search(r"k_hclustILi(\d)E", k) for k in kernels) if m) == ["0", "1", "2"], sorted(kernels)
    assert sum("7k_eloss" in k for k in kernels) == 1, sorted(kernels)


def test_no_kernel_spills_or_exceeds_the_launchable_registers(kernels):
    assert len(kernels) == 4
    for name, k in kernels.items():
        print(name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["next_free_vgpr"] <= 128, (name, k)
        assert k["group_segment_fixed_size"] <= 1024, (name, k)       # the state is dynamic LDS, sized per call; static: the reductions' scratch
