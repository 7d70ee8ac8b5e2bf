"""The run loop of the partition searches in NumPy, written once (DESIGN.md §8 "Point-estimate search", "One run";
csrc/greedy.inc.hip is its device counterpart): test infrastructure only.  psm_search_ref.py (Binder / the VI bound on the
counts), vi_search_ref.py (exact VI on the tables) and id_search_ref.py (exact ID on the tables) supply the score.

A criterion is an object with
  lab, sz                 the slots of the points (0 = unallocated) and the slot sizes, sz[1..len(sz) − 2] usable; the loop
                          updates both, the criterion keeps whatever else its score needs
  new_score               the score of a new cluster
  take_out(i, a)          point i has just left slot a (lab and sz already say so)
  scores(i, occ)          (scores, payloads or None) of putting i into each occupied slot of occ
  put_in(i, w, payload)   point i is about to enter slot w (lab and sz do not say so yet); payload is the winner's"""
import itertools

import numpy as np


def sortlabels(x):
    """utils.jl:69-74: relabel by order of first appearance"""
    out, seen = np.zeros(len(x), np.int64), {}
    for i, v in enumerate(x):
        out[i] = seen.setdefault(int(v), len(seen) + 1)
    return out


def greedy_search(crit, order, cap, maxsweeps):
    """One run.  order: a permutation of 1..n; cap: a new cluster is offered while fewer than cap are occupied.  Ties: the
    lower score, then the point's own slot, then the lowest slot; a new cluster takes the slot the point just emptied, else
    the lowest free one.  Returns a dict with the raw slots, the sortlabels'd labels, sweeps, converged, moves, K."""
    lab, sz = crit.lab, crit.sz
    usable = sz[1:len(sz) - 1]
    K = int(np.count_nonzero(sz))
    sweeps = moves = 0
    converged = False
    while sweeps < maxsweeps:
        moved = 0
        for i in (int(o) - 1 for o in order):
            a = int(lab[i])
            if a:
                lab[i] = 0
                sz[a] -= 1
                crit.take_out(i, a)
                if sz[a] == 0:
                    K -= 1
            emptied = a != 0 and sz[a] == 0
            occ = (np.flatnonzero(usable) + 1).tolist()
            best = None                                            # (score, priority, slot, payload, is_new)
            if occ:
                scores, payloads = crit.scores(i, np.asarray(occ))
                best = min(zip(scores, (0 if k == a else k for k in occ), occ, payloads or itertools.repeat(0)),
                           key=lambda cand: cand[:2]) + (False,)
            if K < cap:
                slot = a if emptied else int(np.flatnonzero(usable == 0)[0]) + 1
                cand = (crit.new_score, 0 if emptied else slot, slot, 0, True)
                if best is None or cand[:2] < best[:2]:
                    best = cand
            _, _, w, payload, isnew = best
            crit.put_in(i, w, payload)
            lab[i] = w
            sz[w] += 1
            K += int(isnew)
            moved += int(a == 0 or w != a)
        sweeps += 1
        moves += moved
        if moved == 0:
            converged = True
            break
    return dict(raw=lab.copy(), labels=sortlabels(lab), sweeps=sweeps, converged=converged, moves=moves, K=K)


def best_single_move_gain(c, value, may_open):
    """The largest decrease of value(labelling) any single-point move achieves, by brute force over every point and every
    target: the other clusters and, where may_open(number of clusters, the point is alone in its cluster) says so, a new
    one.  <= 0 means c is a local optimum."""
    c = np.asarray(c, np.int64)
    base, gain = value(c), 0
    labels = list(np.unique(c))
    fresh = int(c.max()) + 1
    for i in range(len(c)):
        targets = [l for l in labels if l != c[i]]
        if may_open(len(labels), int((c == c[i]).sum()) == 1):
            targets.append(fresh)
        for l in targets:
            x = c.copy()
            x[i] = l
            gain = max(gain, base - value(x))
    return gain
