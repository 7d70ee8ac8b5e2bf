"""Register, scratch and LDS budgets of the kernels behind rc_score_labellings (csrc/score.inc.hip), read from the gfx950 ISA the
compiler emits (hipcc cross-compiles without a GPU).  k_score_rows (staging) and k_score_blocks (the reduction into the
upper-triangle blocks) run as 256-thread workgroups — 4 waves, one per SIMD — so any lane count up to 512 VGPRs launches; the
sums between them are predict's k_predict_sums, four instantiations of 1024 threads — 16 waves, four per SIMD, at most 128
VGPRs a lane.  The bins of k_score_blocks and the staged row of k_predict_sums are dynamic LDS, sized per call.  No kernel may
touch scratch, and every atomic's address space is known at compile time: the bins are LDS atomics, the parts' flushes
global ones."""
import re
import pytest

from isa import listing


@pytest.fixture(scope="module")
def kernels():
    return {k: v for k, v in listing().items() if re.search(r"3scr\d+k_score_|3prd\d+k_predict_sums", k)}


def pick(kernels, fragment):
    return {k: v for k, v in kernels.items() if fragment in k}


def test_every_instantiation_is_there(kernels):
    assert len(pick(kernels, "k_score_rows")) == 1 and len(pick(kernels, "k_score_blocks")) == 1, sorted(kernels)
    sums = pick(kernels, "k_predict_sums")
    variants = sorted(re.search(r"k_predict_sumsILb(\d)ELb(\d)EE", k).groups() for k in sums)
    assert variants == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(sums)      # (row in LDS, parts with atomics)


def test_no_kernel_spills_or_exceeds_the_launchable_registers(kernels):
    assert len(kernels) == 6
    for name, k in kernels.items():
        print(name, {x: y for x, y in k.items() if x != "text"})
        assert k["text"], name
        assert k["private_segment_fixed_size"] == 0, name
        assert not re.search(r"\bscratch_", k["text"]), name
        assert k["group_segment_fixed_size"] == 0, name                   # the bins and the staged row are dynamic LDS
        assert k["next_free_vgpr"] <= (128 if "k_predict_sums" in name else 512), name
    # the two new kernels are reductions and gathers: far from any limit, and they should stay there
    for name, k in {**pick(kernels, "k_score_rows"), **pick(kernels, "k_score_blocks")}.items():
        assert k["next_free_vgpr"] <= 64, name


def test_the_atomics_are_in_the_right_memory(kernels):
    for name, k in kernels.items():
        lds_atomics = len(re.findall(r"\bds_add_(?:rtn_)?u64\b", k["text"]))
        global_atomics = len(re.findall(r"\bglobal_atomic_\w+", k["text"]))
        flat_atomics = len(re.findall(r"\bflat_atomic_\w+", k["text"]))
        print(name, lds_atomics, global_atomics, flat_atomics)
        assert flat_atomics == 0, name                                    # the address space is known at compile time
        if "k_score_blocks" in name:
            assert lds_atomics >= 4 and global_atomics == 0, name         # the four halves of a bin; blocks are plain read-modify-writes
        elif "k_score_rows" in name:
            assert lds_atomics == 0 and global_atomics == 0, name
        else:
            parts = re.search(r"k_predict_sumsILb\dELb(\d)EE", name).group(1) == "1"
            assert lds_atomics == 0 and (global_atomics >= 2) == parts, name
