"""The eight entry points that consume a co-clustering count matrix — the search, the dendrogram and the expected loss, each
for host counts, for samples (not the expected loss) and for a live context — report a bad source the same way and in the
same order of precedence: how the counts reach the device is shared (cnt:: in csrc/samplecounts.inc.hip), and the codes and
texts in EXPECT are what the library said for these inputs at the parent of the commit that shared it.  Called through
_lib.lib() directly; n = 5, m = 3 with the SAMPLES / COUNTS of test_gpu_search_errors.py, n = 6 where the host form's
leading dimension must differ from n.  The order every form keeps: the source is there; the consumer's argument checks; the
device; the acquisition (sample labels, a context's recorded samples); the run's own checks; the counts themselves.

Besides the text each case pins the buffer that holds it.  Before every call a context's buffer is given one marker text and
the thread's another: a device form leaves the context's alone ("thread"), a context form writes its own buffer, which the
library mirrors into the thread's ("both")."""
import ctypes as C
import re

import numpy as np
import pytest

import redclust_amd as rc
from redclust_amd import _lib

from test_gpu_search_errors import M, N, SAMPLES

pytestmark = pytest.mark.gpu

SAMPLES6 = np.c_[SAMPLES, [3, 2, 6]].astype(np.int64)
MARK_CTX = "rc_set_option: prune must be -1 (automatic), 0 (never) or 1 (always)"
MARK_THREAD = "rc_hclust_cut: NULL argument"
ARG = -1

# entry point -> (consumer, form)
FORMS = {
    "rc_psm_search": ("search", "host"), "rc_psm_search_samples": ("search", "samples"), "rc_psm_search_ctx": ("search", "ctx"),
    "rc_hclust": ("hclust", "host"), "rc_hclust_samples": ("hclust", "samples"), "rc_hclust_ctx": ("hclust", "ctx"),
    "rc_psm_expected_loss": ("eloss", "host"), "rc_psm_expected_loss_ctx": ("eloss", "ctx"),
}

# Sources.  Every form: "ok", "null".  Device forms: "dev64" (device 64), "ok6" (n = 6), "ok1" (the first sample alone: what
# the context below has recorded).  Samples: "label" (a label n + 1).  Host: "asym", "asym6" (counts[1, 3] != counts[3, 1]).
# Context: "empty" (nothing recorded), "two" (one sample recorded, numsamples = 2).
# The consumer's own offence: "loss" (specifier 7), "linkage" (specifier 9), "maxsweeps" (0), "maxcut" (n + 1), "labelling"
# (a label n + 1 in the second labelling), "init" (a label n + 1 in the second run's start), or None.
EXPECT = {
    ("rc_psm_search", "null", None): (-1, "rc_psm_search: NULL argument", "thread"),
    ("rc_psm_search", "null", "loss"): (-1, "rc_psm_search: NULL argument", "thread"),
    ("rc_psm_search", "null", "maxsweeps"): (-1, "rc_psm_search: NULL argument", "thread"),
    ("rc_psm_search", "null", "init"): (-1, "rc_psm_search: NULL argument", "thread"),
    ("rc_psm_search", "dev64", None): (-1, "rc_psm_search: device 64 not available (", "thread"),
    ("rc_psm_search", "dev64", "loss"): (-1, "rc_psm_search: invalid loss specifier 7", "thread"),
    ("rc_psm_search", "dev64", "maxsweeps"): (-1, "rc_psm_search: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)", "thread"),
    ("rc_psm_search", "dev64", "init"): (-1, "rc_psm_search: device 64 not available (", "thread"),
    ("rc_psm_search", "asym", None): (-1, "point search: the counts are not symmetric", "thread"),
    ("rc_psm_search", "asym", "loss"): (-1, "rc_psm_search: invalid loss specifier 7", "thread"),
    ("rc_psm_search", "asym", "maxsweeps"): (-1, "rc_psm_search: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)", "thread"),
    ("rc_psm_search", "asym", "init"): (-1, "point search: label 6 of run 2 outside 0..n", "thread"),
    ("rc_psm_search", "asym6", None): (-1, "point search: the counts are not symmetric", "thread"),
    ("rc_psm_search", "asym6", "loss"): (-1, "rc_psm_search: invalid loss specifier 7", "thread"),
    ("rc_psm_search", "asym6", "maxsweeps"): (-1, "rc_psm_search: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)", "thread"),
    ("rc_psm_search", "asym6", "init"): (-1, "point search: label 7 of run 2 outside 0..n", "thread"),
    ("rc_psm_search_samples", "null", None): (-1, "rc_psm_search_samples: NULL argument", "thread"),
    ("rc_psm_search_samples", "null", "loss"): (-1, "rc_psm_search_samples: NULL argument", "thread"),
    ("rc_psm_search_samples", "null", "maxsweeps"): (-1, "rc_psm_search_samples: NULL argument", "thread"),
    ("rc_psm_search_samples", "null", "init"): (-1, "rc_psm_search_samples: NULL argument", "thread"),
    ("rc_psm_search_samples", "dev64", None): (-1, "rc_psm_search_samples: device 64 not available (", "thread"),
    ("rc_psm_search_samples", "dev64", "loss"): (-1, "rc_psm_search_samples: invalid loss specifier 7", "thread"),
    ("rc_psm_search_samples", "dev64", "maxsweeps"): (-1, "rc_psm_search_samples: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)", "thread"),
    ("rc_psm_search_samples", "dev64", "init"): (-1, "rc_psm_search_samples: device 64 not available (", "thread"),
    ("rc_psm_search_samples", "label", None): (-1, "rc_psm_search_samples: label 6 of sample 2 at position 3 outside 1..n", "thread"),
    ("rc_psm_search_samples", "label", "loss"): (-1, "rc_psm_search_samples: invalid loss specifier 7", "thread"),
    ("rc_psm_search_samples", "label", "maxsweeps"): (-1, "rc_psm_search_samples: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)", "thread"),
    ("rc_psm_search_samples", "label", "init"): (-1, "rc_psm_search_samples: label 6 of sample 2 at position 3 outside 1..n", "thread"),
    ("rc_psm_search_ctx", "null", None): (-1, "rc_psm_search_ctx: NULL ctx", "thread"),
    ("rc_psm_search_ctx", "null", "loss"): (-1, "rc_psm_search_ctx: NULL ctx", "thread"),
    ("rc_psm_search_ctx", "null", "maxsweeps"): (-1, "rc_psm_search_ctx: NULL ctx", "thread"),
    ("rc_psm_search_ctx", "null", "init"): (-1, "rc_psm_search_ctx: NULL ctx", "thread"),
    ("rc_psm_search_ctx", "empty", None): (-5, "rc_psm_search_ctx: no sample has been recorded", "both"),
    ("rc_psm_search_ctx", "empty", "loss"): (-1, "rc_psm_search_ctx: invalid loss specifier 7", "both"),
    ("rc_psm_search_ctx", "empty", "maxsweeps"): (-1, "rc_psm_search_ctx: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)", "both"),
    ("rc_psm_search_ctx", "empty", "init"): (-5, "rc_psm_search_ctx: no sample has been recorded", "both"),
    ("rc_psm_search_ctx", "two", None): (-1, "point search: the diagonal of the counts is not m = 2 everywhere", "both"),
    ("rc_psm_search_ctx", "two", "loss"): (-1, "rc_psm_search_ctx: invalid loss specifier 7", "both"),
    ("rc_psm_search_ctx", "two", "maxsweeps"): (-1, "rc_psm_search_ctx: need maxsweeps >= 1 and maxK >= 0 (got 0, 0)", "both"),
    ("rc_psm_search_ctx", "two", "init"): (-1, "point search: label 6 of run 2 outside 0..n", "both"),
    ("rc_hclust", "null", None): (-1, "rc_hclust: NULL argument", "thread"),
    ("rc_hclust", "null", "linkage"): (-1, "rc_hclust: NULL argument", "thread"),
    ("rc_hclust", "null", "maxcut"): (-1, "rc_hclust: NULL argument", "thread"),
    ("rc_hclust", "dev64", None): (-1, "rc_hclust: device 64 not available (", "thread"),
    ("rc_hclust", "dev64", "linkage"): (-1, "rc_hclust: invalid linkage specifier 9", "thread"),
    ("rc_hclust", "dev64", "maxcut"): (-1, "rc_hclust: need 0 <= maxcut <= n and vilb with maxcut > 0 (got 6)", "thread"),
    ("rc_hclust", "asym", None): (-1, "rc_hclust: the counts are not symmetric", "thread"),
    ("rc_hclust", "asym", "linkage"): (-1, "rc_hclust: invalid linkage specifier 9", "thread"),
    ("rc_hclust", "asym", "maxcut"): (-1, "rc_hclust: need 0 <= maxcut <= n and vilb with maxcut > 0 (got 6)", "thread"),
    ("rc_hclust", "asym6", None): (-1, "rc_hclust: the counts are not symmetric", "thread"),
    ("rc_hclust", "asym6", "linkage"): (-1, "rc_hclust: invalid linkage specifier 9", "thread"),
    ("rc_hclust", "asym6", "maxcut"): (-1, "rc_hclust: need 0 <= maxcut <= n and vilb with maxcut > 0 (got 7)", "thread"),
    ("rc_hclust_samples", "null", None): (-1, "rc_hclust_samples: NULL argument", "thread"),
    ("rc_hclust_samples", "null", "linkage"): (-1, "rc_hclust_samples: NULL argument", "thread"),
    ("rc_hclust_samples", "null", "maxcut"): (-1, "rc_hclust_samples: NULL argument", "thread"),
    ("rc_hclust_samples", "dev64", None): (-1, "rc_hclust_samples: device 64 not available (", "thread"),
    ("rc_hclust_samples", "dev64", "linkage"): (-1, "rc_hclust_samples: invalid linkage specifier 9", "thread"),
    ("rc_hclust_samples", "dev64", "maxcut"): (-1, "rc_hclust_samples: need 0 <= maxcut <= n and vilb with maxcut > 0 (got 6)", "thread"),
    ("rc_hclust_samples", "label", None): (-1, "rc_hclust_samples: label 6 of sample 2 at position 3 outside 1..n", "thread"),
    ("rc_hclust_samples", "label", "linkage"): (-1, "rc_hclust_samples: invalid linkage specifier 9", "thread"),
    ("rc_hclust_samples", "label", "maxcut"): (-1, "rc_hclust_samples: need 0 <= maxcut <= n and vilb with maxcut > 0 (got 6)", "thread"),
    ("rc_hclust_ctx", "null", None): (-1, "rc_hclust_ctx: NULL ctx", "thread"),
    ("rc_hclust_ctx", "null", "linkage"): (-1, "rc_hclust_ctx: NULL ctx", "thread"),
    ("rc_hclust_ctx", "null", "maxcut"): (-1, "rc_hclust_ctx: NULL ctx", "thread"),
    ("rc_hclust_ctx", "empty", None): (-5, "rc_hclust_ctx: no sample has been recorded", "both"),
    ("rc_hclust_ctx", "empty", "linkage"): (-1, "rc_hclust_ctx: invalid linkage specifier 9", "both"),
    ("rc_hclust_ctx", "empty", "maxcut"): (-1, "rc_hclust_ctx: need 0 <= maxcut <= n and vilb with maxcut > 0 (got 6)", "both"),
    ("rc_hclust_ctx", "two", None): (-1, "rc_hclust_ctx: the diagonal of the counts is not m = 2 everywhere", "both"),
    ("rc_hclust_ctx", "two", "linkage"): (-1, "rc_hclust_ctx: invalid linkage specifier 9", "both"),
    ("rc_hclust_ctx", "two", "maxcut"): (-1, "rc_hclust_ctx: need 0 <= maxcut <= n and vilb with maxcut > 0 (got 6)", "both"),
    ("rc_psm_expected_loss", "null", None): (-1, "rc_psm_expected_loss: NULL argument", "thread"),
    ("rc_psm_expected_loss", "null", "loss"): (-1, "rc_psm_expected_loss: NULL argument", "thread"),
    ("rc_psm_expected_loss", "null", "labelling"): (-1, "rc_psm_expected_loss: NULL argument", "thread"),
    ("rc_psm_expected_loss", "dev64", None): (-1, "rc_psm_expected_loss: device 64 not available (", "thread"),
    ("rc_psm_expected_loss", "dev64", "loss"): (-1, "rc_psm_expected_loss: invalid loss specifier 7", "thread"),
    ("rc_psm_expected_loss", "dev64", "labelling"): (-1, "rc_psm_expected_loss: device 64 not available (", "thread"),
    ("rc_psm_expected_loss", "asym", None): (-1, "rc_psm_expected_loss: the counts are not symmetric", "thread"),
    ("rc_psm_expected_loss", "asym", "loss"): (-1, "rc_psm_expected_loss: invalid loss specifier 7", "thread"),
    ("rc_psm_expected_loss", "asym", "labelling"): (-1, "rc_psm_expected_loss: label 6 of labelling 2 at position 3 outside 1..n", "thread"),
    ("rc_psm_expected_loss", "asym6", None): (-1, "rc_psm_expected_loss: the counts are not symmetric", "thread"),
    ("rc_psm_expected_loss", "asym6", "loss"): (-1, "rc_psm_expected_loss: invalid loss specifier 7", "thread"),
    ("rc_psm_expected_loss", "asym6", "labelling"): (-1, "rc_psm_expected_loss: label 7 of labelling 2 at position 3 outside 1..n", "thread"),
    ("rc_psm_expected_loss_ctx", "null", None): (-1, "rc_psm_expected_loss_ctx: NULL ctx", "thread"),
    ("rc_psm_expected_loss_ctx", "null", "loss"): (-1, "rc_psm_expected_loss_ctx: NULL ctx", "thread"),
    ("rc_psm_expected_loss_ctx", "null", "labelling"): (-1, "rc_psm_expected_loss_ctx: NULL ctx", "thread"),
    ("rc_psm_expected_loss_ctx", "empty", None): (-5, "rc_psm_expected_loss_ctx: no sample has been recorded", "both"),
    ("rc_psm_expected_loss_ctx", "empty", "loss"): (-1, "rc_psm_expected_loss_ctx: invalid loss specifier 7", "both"),
    ("rc_psm_expected_loss_ctx", "empty", "labelling"): (-5, "rc_psm_expected_loss_ctx: no sample has been recorded", "both"),
    ("rc_psm_expected_loss_ctx", "two", None): (-1, "rc_psm_expected_loss_ctx: the diagonal of the counts is not m = 2 everywhere", "both"),
    ("rc_psm_expected_loss_ctx", "two", "loss"): (-1, "rc_psm_expected_loss_ctx: invalid loss specifier 7", "both"),
    ("rc_psm_expected_loss_ctx", "two", "labelling"): (-1, "rc_psm_expected_loss_ctx: label 6 of labelling 2 at position 3 outside 1..n", "both"),
}


def counts_of(samples):
    return (samples[:, :, None] == samples[:, None, :]).sum(axis=0).astype(np.uint32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Rig:
    """two contexts on 5 points: `empty` has recorded nothing, `one` has recorded SAMPLES[0] once"""

    def __init__(self):
        D = np.abs(np.subtract.outer(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64)))
        self.empty, self.one = rc.Context(D), rc.Context(D)
        self.one.set_params(delta1=1.0, delta2=1.0, alpha=1.0, beta=1.0, zeta=1.0, gamma=1.0)
        self.one.set_state(SAMPLES[0])
        self.one.record_sample()

    def close(self):
        self.empty.close()
        self.one.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def observe(rig, fn, src, bad=None):
    """One direct call of fn.  Returns ((return code, text of the error, the buffer that holds it), the outputs)."""
    L = _lib.lib()
    consumer, form = FORMS[fn]
    n = 6 if src.endswith("6") else N
    samples = (SAMPLES6 if n == 6 else SAMPLES)[:1 if src == "ok1" else M]
    m = len(samples)
    ctx, keep = None, None
    if form == "ctx":
        ctx = {"null": None, "empty": rig.empty}.get(src, rig.one)
        m = 2 if src == "two" else 1
        head = (ctx.h if ctx is not None else None, m)
    else:
        keep = samples.copy() if form == "samples" else counts_of(samples)
        if src == "label":
            keep[1, 2] = n + 1
        if src.startswith("asym"):
            keep[1, 3] += 1
        head = (64 if src == "dev64" else 0, None if src == "null" else _ptr(keep), m, n)
    ms, cms = C.c_double(), C.c_double()
    tail = (C.byref(ms),) + ((C.byref(cms),) if form == "samples" else ())
    if consumer == "search":
        init, order = np.zeros((2, n), np.int64), np.tile(np.arange(1, n + 1, dtype=np.int32), (2, 1))
        if bad == "init":
            init[1, 3] = n + 1
        labels, runs, best = np.zeros((2, n), np.int64), (_lib.RcPsmRun * 2)(), C.c_int32(-1)
        args = (7 if bad == "loss" else 0, 2, _ptr(init), _ptr(order), 0, 0 if bad == "maxsweeps" else 100, _ptr(labels), runs,
                C.byref(best))
        out = lambda: dict(labels=labels.tolist(), best=best.value,
                           runs=[[getattr(r, k) for k, _ in _lib.RcPsmRun._fields_] for r in runs])
    elif consumer == "hclust":
        merges, bnum, vilb = np.zeros(n, _lib.HCLUST_MERGE), np.zeros(n, np.int64), np.zeros(n + 1)
        args = (9 if bad == "linkage" else 0, _ptr(merges), _ptr(bnum), n + 1 if bad == "maxcut" else 2, _ptr(vilb))
        out = lambda: dict(merges=merges.tolist(), binder_num=bnum.tolist(), vilb=vilb.tolist())
    else:
        labs = np.stack([np.arange(n) // 2 + 1, np.ones(n, np.int64)]).astype(np.int64)
        if bad == "labelling":
            labs[1, 2] = n + 1
        loss_out, num_out = np.zeros(2), np.zeros(2, np.int64)
        args = (7 if bad == "loss" else 0, 2, _ptr(labs), _ptr(loss_out), _ptr(num_out))
        out = lambda: dict(loss=loss_out.tolist(), num=num_out.tolist(), labs=labs, counts=counts_of(samples), m=m)
    # the markers: the context's buffer (mirrored into the thread's), then the thread's alone
    holder = ctx if ctx is not None else rig.one
    assert L.rc_set_option(holder.h, b"prune", 7) == ARG and L.rc_hclust_cut(None, 2, 1, None) == ARG
    assert (L.rc_last_error(holder.h).decode(), L.rc_last_error(None).decode()) == (MARK_CTX, MARK_THREAD)
    code = getattr(L, fn)(*head, *args, *tail)
    if code == 0:
        return (0, "", ""), out()
    text, held = L.rc_last_error(None).decode(), L.rc_last_error(holder.h).decode()
    where = "both" if held == text else "thread" if held == MARK_CTX else "context holds: " + held
    return (code, re.sub(r"\d+ visible\)$", "", text), where), None      # the number of visible devices is the machine's


def cases(fn):
    return [(src, bad) for (f, src, bad) in EXPECT if f == fn]


@pytest.mark.parametrize("fn", sorted(FORMS))
def test_a_bad_source_keeps_its_code_text_buffer_and_precedence(rig, fn):
    assert cases(fn)
    for src, bad in cases(fn):
        got, _ = observe(rig, fn, src, bad)
        print(fn, src, bad, got)
        assert got == EXPECT[fn, src, bad], (src, bad)
    # a valid call afterwards still succeeds, and equals the host form of the same counts
    consumer, form = FORMS[fn]
    for src in ("ok",) if form == "ctx" else ("ok", "ok6"):
        got, out = observe(rig, fn, src)
        assert got == (0, "", ""), src
        host, want = observe(rig, "rc_" + {"search": "psm_search", "hclust": "hclust", "eloss": "psm_expected_loss"}[consumer],
                             "ok1" if form == "ctx" else src)
        assert host == (0, "", "")
        if consumer == "eloss":
            # the exact Binder numerator: pairs together pay the samples that part them, pairs apart those that join them
            cnt, mm = out.pop("counts").astype(np.int64), out.pop("m")
            if form == "ctx":
                cnt, mm = want["counts"].astype(np.int64), want["m"]
            for lab, num in zip(out.pop("labs"), out["num"]):
                same = lab[:, None] == lab[None, :]
                assert num == int(np.triu(np.where(same, mm - cnt, cnt), 1).sum())
            want = dict(loss=want["loss"], num=want["num"])
        assert out == want, src


def test_every_entry_point_has_every_kind_of_case():
    """the table above covers, per entry point, its source alone being bad and the source and the consumer being bad together"""
    for fn, (consumer, form) in FORMS.items():
        srcs = {s for s, b in cases(fn) if b is None}
        assert srcs >= {"ctx": {"null", "empty", "two"}, "samples": {"null", "dev64", "label"},
                        "host": {"null", "dev64", "asym", "asym6"}}[form], fn
        assert {s for s, b in cases(fn) if b is not None} >= {"null", "empty" if form == "ctx" else "dev64"}, fn
