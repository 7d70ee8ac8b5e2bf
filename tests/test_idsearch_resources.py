"""Register and scratch budgets of the exact searches' kernel (csrc/visearch.inc.hip), read from the metadata of the gfx950 ISA
the compiler emits (hipcc cross-compiles without a GPU): k_visearch<PQ, LOSS> runs as ONE 1024-thread workgroup — 16 waves, four
per SIMD — so a lane may own at most 512 / 4 = 128 VGPRs or the kernel cannot be launched, and a scratch access inside the
step loop would sit between its two barriers.  Six instantiations: PQ = 0 / 1 / 4 for the expected VI and the expected ID."""
import os, re, shutil, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "redclust.jl_amd", "csrc", "redclust_hip.hip")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "rc.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC],
                   check=True, cwd=os.path.dirname(SRC), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    res, name, cur = {}, None, {}
    for line in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name, cur = m.group(1), {}
        for key in ("next_free_vgpr", "group_segment_fixed_size", "private_segment_fixed_size"):
            m = re.match(r"\s*\.amdhsa_" + key + r"\s+(\d+)", line)
            if m and name:
                cur[key] = int(m.group(1))
        if ".end_amdhsa_kernel" in line and name:
            res[name] = cur; name = None
    return {k: v for k, v in res.items() if "k_visearch" in k}


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
