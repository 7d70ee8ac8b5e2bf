"""Static checks of k_bulk_syml2 with the exponent folded into its log table, read from the gfx950 ISA the compiler emits (hipcc
cross-compiles without a GPU), as tests/test_kernel_resources.py does:
  * the fallback for contexts over more than four binades, k_bulk_syml2w, keeps the three budgets of the kernel it was (128 registers,
    40 KiB of LDS, no scratch: three of its waves and one resolver wave share a SIMD);
  * the body of k_bulk_syml2<true, true> holds fewer int -> double conversions of the exponent (v_cvt_f64_i32) and fewer subtractions
    of the rounding bias (literal 0xbcc80000 = -bits(1.5·2^52) >> 32) than before the fold: 16 of each then (four entries x four row
    pairs, one copy of the row-pair block).  What remains: no conversion; four bias constants, one per row pair, inside the branch
    taken only by units with lanes that are not whole (their element-wise atomics), none in the streaming path."""
import os, re, shutil, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "redclust.jl_amd", "csrc", "redclust_hip.hip")
PARENT_CVT_F64_I32 = 16        # k_bulk_syml2<true, true> before the fold
PARENT_BIAS_ADDS = 16


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "rc.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC],
                   check=True, cwd=os.path.dirname(SRC), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    bodies, meta, name, cur = {}, {}, None, None
    for line in open(out):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name, cur = m.group(1), []
        if cur is not None:
            cur.append(line)
            if ".Lfunc_end" in line:
                bodies[name] = cur; cur = None
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kname = m.group(1); meta[kname] = {}
        for key in ("next_free_vgpr", "group_segment_fixed_size", "private_segment_fixed_size"):
            m = re.match(r"\s*\.amdhsa_" + key + r"\s+(\d+)", line)
            if m:
                meta[kname][key] = int(m.group(1))
    return bodies, meta


def one(d, fragment):
    hits = [k for k in d if fragment in k]
    assert len(hits) == 1, (fragment, hits)
    return d[hits[0]]


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
