"""Counts from samples without a GPU: the ABI declarations of rc_samples_counts / rc_psm_search_samples, the Julia glue's
calls, and the argument errors of posterior_counts / posterior_coclustering / searchpointestimate that need no device."""
import os
import re

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nargs(proto):
    return len([a for a in proto.split(",") if a.strip()])


def test_header_and_signatures_agree_on_the_new_entries():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "redclust_hip.h")).read(), flags=re.S)
    for name, nargs in (("rc_samples_counts", 6), ("rc_psm_search_samples", 15)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert name in rc.SIGNATURES and _nargs(m.group(1)) == len(rc.SIGNATURES[name][1]) == nargs, name
    # the search entry is rc_psm_search with the samples in place of the counts and one more timing output
    assert len(rc.SIGNATURES["rc_psm_search_samples"][1]) == len(rc.SIGNATURES["rc_psm_search"][1]) + 1


def test_the_source_is_part_of_the_build():
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "samplecounts.inc.hip"))
    assert '#include "samplecounts.inc.hip"' in open(os.path.join(csrc, "redclust_hip.hip")).read()
    assert os.path.join(csrc, "samplecounts.inc.hip") in _lib._sources()  # build() watches it


def test_every_include_is_built_and_listed():
    """The *.inc.hip and *.inc.hpp files of csrc/, the ones redclust_hip.hip includes and the ones build() watches are the same set."""
    csrc = os.path.join(ROOT, "redclust.jl_amd", "csrc")
    on_disk = {f for f in os.listdir(csrc) if f.endswith((".inc.hip", ".inc.hpp"))}
    included = set(re.findall(r'^#include "([^"]+\.inc\.h(?:ip|pp))"', open(os.path.join(csrc, "redclust_hip.hip")).read(), flags=re.M))
    listed = {os.path.basename(s) for s in _lib._sources() if os.path.dirname(s) == csrc} - {"redclust_hip.hip"}
    assert on_disk and on_disk == included == listed, (sorted(on_disk), sorted(included), sorted(listed))


def test_julia_glue_calls_the_new_entries():
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    assert "ccall((:rc_psm_search_samples, LIB)" in jl and "ccall((:rc_samples_counts, LIB)" in jl
    assert "ccall((:rc_psm_search, LIB)" in jl                   # the count-matrix method stays
    assert re.search(r"function searchpointestimate\(b::HIPBackend, result;", jl)
    assert re.search(r"function searchpointestimate\(b::HIPBackend, counts::Matrix\{UInt32\}, numsamples::Integer;", jl)
    assert re.search(r"function posteriorcounts\(b::HIPBackend, result\)", jl)
    # the n²·m loop over the samples is gone
    assert not re.search(r"for c in result\.clusts, j in 1:n, i in 1:n", jl)
    import test_oracle_cpu
    test_oracle_cpu.test_julia_glue_ccalls_match_the_header()


@pytest.mark.parametrize("fn", ["posterior_counts", "posterior_coclustering"])
def test_argument_errors_that_need_no_device(fn):
    f = getattr(rc, fn)
    with pytest.raises(TypeError, match="vector of integers"):
        f(np.array([1, 2, 2], np.int64))                          # one labelling is not a list of samples
    with pytest.raises(TypeError, match="vector of integers"):
        f(np.ones((2, 3)))                                        # floats are not labels
    with pytest.raises(ValueError, match="no samples"):
        f([])
    import types
    with pytest.raises(ValueError, match="no samples"):
        f(types.SimpleNamespace(clusts=[]))


def test_searchpointestimate_argument_errors_are_unchanged():
    C = np.full((3, 3), 2, np.uint32)
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.searchpointestimate(C, "omARI", numsamples=2)
    with pytest.raises(ValueError, match="numsamples"):
        rc.searchpointestimate(C, "binder")
    with pytest.raises(ValueError, match="square"):
        rc.searchpointestimate(np.zeros((2, 3), np.uint32), "binder", numsamples=2)
    with pytest.raises(ValueError, match="n entries"):
        rc.searchpointestimate(C, "binder", numsamples=2, init=[[1, 1]])
    with pytest.raises(ValueError):
        rc.searchpointestimate(None, "VI")
    # with samples: the init check still comes before any device work
    import types
    samples = types.SimpleNamespace(clusts=[np.array([1, 1, 2]), np.array([1, 2, 2])])
    with pytest.raises(ValueError, match="n entries"):
        rc.searchpointestimate(samples, "binder", init=[[1, 1]])
    with pytest.raises(ValueError, match='exact=True needs loss="VI"'):
        rc.searchpointestimate(samples, "binder", exact=True)
