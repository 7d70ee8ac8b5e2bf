"""Register, scratch and LDS budgets of the kernels behind rc_cluster_profiles (csrc/profile.inc.hip), read from the metadata of
the gfx950 ISA the compiler emits (hipcc cross-compiles without a GPU).  k_profile_rows (staging), k_profile_points (one wave
per (row, labelling): the exact selection of the neighbour cluster) and k_profile_medoids (one workgroup per labelling) all run
as 256-thread workgroups — 4 waves, one per SIMD — so any lane count up to 512 VGPRs launches; the sums between them are
predict's k_predict_sums, which tests/test_predict_resources.py and tests/test_score_resources.py count and budget.  The
per-cluster minima of k_profile_medoids are dynamic LDS, sized per launch.  No kernel may touch scratch."""
import pytest

from isa import listing

NAMES = ("k_profile_rows", "k_profile_points", "k_profile_medoids")


@pytest.fixture(scope="module")
def kernels():
    return {k: v for k, v in listing().items() if "3prf" in k}


def test_the_new_kernels_are_all_there_once_each_and_named_apart(kernels):
    assert len(kernels) == len(NAMES), sorted(kernels)
    for name in NAMES:
        assert sum(name in k for k in kernels) == 1, (name, sorted(kernels))
    assert not any("k_score_" in k or "k_predict_sums" in k for k in kernels)      # the siblings' tests count those


def test_no_scratch_no_static_lds_and_launchable_registers(kernels):
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == 0, name                   # the minima are dynamic LDS
        assert k["next_free_vgpr"] <= 512, name                           # what a 256-thread workgroup can launch with
        # gathers, one 128-bit comparison per candidate and two minima: far from that limit, and they should stay there
        assert k["next_free_vgpr"] <= 64, name
