#!/usr/bin/env python3
"""How many of k_bulk_syml2's fast units span two clusters at the headline state (bench.py: N = 8192, K = 50, generating labels,
stationary), how many have a donor lane, and how many keep the per-lane class code — counted on the host.

The fast units of a 128-column block (columns c0 .. c0 + 127 of the internal order, rows 0 .. c0 - 1 above the diagonal block) all
see the same columns, so the classes are decided per column block and weighted by the block's 8-row groups (c0 / 8).  The internal
order is the one rc_set_state lays out (clusters of more than seven points by label, smaller ones first, stable); the labels are
those after the sweeps.  The choice of the two clusters and the lane predicates restate syml2_fast.
usage: python tools/two_cluster_premise.py [sweeps]   (one JSON line)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import redclust_amd as rc  # noqa: E402


def internal_order(labels, small_max=7):
    n = len(labels)
    size = np.bincount(labels, minlength=n + 1)
    large = size[labels] > small_max
    return np.lexsort((np.arange(n), labels, large))          # small clusters first, then by label, stable


def classify(cs):
    """cs: the 128 column clusters of a block -> (two_cluster, donors, straight, odd lanes)"""
    cs0, cs1 = cs[0::2], cs[1::2]
    k0 = cs0[0]
    if (cs == k0).all():
        return False, 0, True, 0
    not0, not1 = np.flatnonzero(cs0 != k0), np.flatnonzero(cs1 != k0)
    l0, l1 = (not0[0] if len(not0) else 64), (not1[0] if len(not1) else 64)
    k1 = cs0[l0] if l0 <= l1 else cs1[l1]
    cand = []
    for k in (k0, k1, cs0[32], cs1[63]):
        if k not in [c for c, _ in cand]:
            cand.append((k, int((cs == k).sum())))
    # the kernel's insertion order: (k0, k1) sorted by count, then k2, k3 displace by strictly larger counts
    (ka, na), (kb, nb) = cand[0], cand[1]
    if nb > na:
        (ka, na), (kb, nb) = (kb, nb), (ka, na)
    for k, c in cand[2:]:
        if c > na:
            (kb, nb), (ka, na) = (ka, na), (k, c)
        elif c > nb:
            kb, nb = k, c
    in0, in1 = (cs0 == ka) | (cs0 == kb), (cs1 == ka) | (cs1 == kb)
    whole0 = (cs0 == cs1) & in0
    nxt_whole, nxt_cs0 = np.append(whole0[1:], False), np.append(cs0[1:], -1)
    donor = ~whole0 & in0 & in1 & nxt_whole & (nxt_cs0 == cs1)
    whole = whole0 | donor
    isB = whole & (cs0 == kb)
    isA = whole & ~isB
    firstB = np.flatnonzero(isB)[0] if isB.any() else 64
    firstA = np.flatnonzero(isA)[0] if isA.any() else 64
    runB = firstB == 64 or not isA[firstB:].any()
    runA = firstA == 64 or not isB[firstA:].any()
    return True, int(donor.sum()), bool(runB or runA), int((~whole).sum())


def main():
    sweeps = int(sys.argv[1]) if len(sys.argv) > 1 else 220
    n, K = int(os.environ.get("RC_BENCH_N", 8192)), int(os.environ.get("RC_BENCH_K", 50))
    data = rc.generatemixture(n, K, seed=1)
    D, truth = data["distancematrix"], data["clusts"]
    ctx = rc.Context(D)
    ctx.set_params(**rc.likelihood_hyperparams(D, truth))
    ctx.set_state(truth)
    for t in range(sweeps):
        ctx.gibbs_sweep(1.0, 0.5, 1, t)
    labels = ctx.get_state()[0]
    name = ctx.bulk_kernel_name()
    ctx.close()
    order = internal_order(np.asarray(truth))
    lab = np.asarray(labels)[order]
    tot = dict(groups=0, two_cluster=0, one_donor=0, more_donors=0, per_lane_code=0, with_odd_lanes=0)
    blocks = dict(tot)
    for c0 in range(128, n - 127, 128):
        two, donors, straight, odd = classify(lab[c0:c0 + 128])
        for acc, w in ((tot, c0 // 8), (blocks, 1)):
            acc["groups"] += w
            acc["two_cluster"] += w * two
            acc["one_donor"] += w * (donors == 1)
            acc["more_donors"] += w * (donors > 1)
            acc["per_lane_code"] += w * (two and not straight)
            acc["with_odd_lanes"] += w * (odd > 0)
    share = {k: round(v / tot["groups"], 4) for k, v in tot.items() if k != "groups"}
    print(json.dumps(dict(n=n, K=K, sweeps=sweeps, kernel=name, labels_changed_from_truth=int((np.asarray(labels) != np.asarray(truth)).sum()),
                          cluster_size_mean=float(n / len(np.unique(labels))), column_blocks=blocks, groups_of_8_rows=tot, share_of_groups=share)))


if __name__ == "__main__":
    main()
