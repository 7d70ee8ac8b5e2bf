"""Register and scratch budgets of the exact searches' kernel (csrc/visearch.inc.hip), read from the metadata of the gfx950 ISA
the compiler emits (hipcc cross-compiles without a GPU): k_visearch<PQ, LOSS> runs as ONE 1024-thread workgroup — 16 waves, four
per SIMD — so a lane may own at most 512 / 4 = 128 VGPRs or the kernel cannot be launched, and a scratch access inside the
step loop would sit between its two barriers.  Six instantiations: PQ = 0 / 1 / 4 for the expected VI and the expected ID."""
import re
import pytest

from isa import resources


@pytest.fixture(scope="module")
def kernels():
    return resources("k_visearch")


def test_every_instantiation_is_there(kernels):
    # template arguments <PQ, LOSS> as the Itanium ABI mangles them: ILi<PQ>ELi<LOSS>E
    assert sorted(re.search(r"k_visearchILi(\d)ELi(\d)E", k).groups() for k in kernels) == \
        [(pq, loss) for pq in "014" for loss in "01"], sorted(kernels)


def test_no_instantiation_spills_or_exceeds_the_launchable_registers(kernels):
    assert len(kernels) == 6
    for name, k in kernels.items():
        print(name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["next_free_vgpr"] <= 128, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)          # all of the LDS is dynamic: the host sizes it per call
