"""The rule of `mash screen -w` (winner-take-all; Mash 2.3 CommandScreen restated, no recorded mash output) as a plain
statement on top of tests/screen_rule.py.  Shared by the winner tests; not a test module itself.

Per reference i: H_i its hashes, n_i = |H_i|, L_i its genome length; count(h) as in screen_rule.

    shared0_i  = number of h in H_i with count(h) >= 1                      (the plain screen's shared)
    score_i    = identity(shared0_i, n_i, k); its order is the order of the exact ratios shared0_i / n_i, which is what is
                 compared here (fractions.Fraction) -- and math.pow is asserted to order every pair met the same way
    winner(h)  = for every h with count(h) >= 1, among the references that hold h: the greatest score, then the greatest
                 L_i, then the LOWEST INDEX (Mash leaves this last choice open; it is ours).  A reference without hashes
                 holds none and never competes.
    shared_i   = number of h in H_i with winner(h) = i
    median_i   = element [shared_i / 2] of the ascending count(h) of those hashes (0: none)
    counts_i   = count(h) where i won h, 0 elsewhere
    identity_i, p_i follow from shared_i with n_i and the set size unchanged
    sum_i shared_i = number of distinct reference hashes with count >= 1
"""
import math
from fractions import Fraction

import numpy as np

from tests import screen_rule as rule


def _pow_agrees(a, b, k):
    """(shared0, n) of two references: math.pow orders the identities as the exact ratios are ordered"""
    (sa, na), (sb, nb) = a, b
    ra, rb = Fraction(sa, na), Fraction(sb, nb)
    ia, ib = rule.identity(sa, na, k), rule.identity(sb, nb, k)
    return (ra > rb) == (ia > ib) and (ra == rb) == (ia == ib)


def winner_tally(ref_hashes, hashes, k, lengths=None):
    """per reference: (counts per entry, shared, median) under winner-take-all, from the window hashes of the read set.
    lengths: genome lengths (None: all equal)."""
    refs = [np.asarray(H, dtype=np.uint64) for H in ref_hashes]
    nr = len(refs)
    lengths = [0] * nr if lengths is None else [int(x) for x in lengths]
    plain = rule.tally(refs, hashes)
    shared0 = [p[1] for p in plain]
    # the order of rule 3 as a sort key: greater is better; the index enters negated (lowest wins)
    key = [(Fraction(shared0[i], refs[i].size) if refs[i].size else Fraction(-1), lengths[i], -i) for i in range(nr)]
    checked = set()
    best = {}                                    # hash -> index of the winner so far
    for i in range(nr):
        for h, c in zip(refs[i].tolist(), plain[i][0].tolist()):
            if c == 0:
                continue
            j = best.get(h)
            if j is None:
                best[h] = i
                continue
            pair = (shared0[i], refs[i].size, shared0[j], refs[j].size)
            if pair not in checked:
                checked.add(pair)
                assert _pow_agrees(pair[:2], pair[2:], k), pair
            if key[i] > key[j]:
                best[h] = i
    out = []
    for i in range(nr):
        c = plain[i][0].copy()
        won = np.array([best.get(h) == i for h in refs[i].tolist()], dtype=bool) if refs[i].size else np.zeros(0, bool)
        c[~won] = 0
        nz = np.sort(c[c > 0])
        out.append((c, int(nz.size), int(nz[nz.size // 2]) if nz.size else 0))
    found = sum(1 for _ in best)
    assert sum(o[1] for o in out) == found       # every found hash has exactly one winner
    return out


def distinct_found(ref_hashes, hashes):
    """number of distinct reference hashes with count >= 1"""
    refs = [np.asarray(H, dtype=np.uint64) for H in ref_hashes]
    allh = np.unique(np.concatenate(refs + [np.zeros(0, np.uint64)]))
    return int(np.isin(allh, np.unique(np.asarray(hashes, dtype=np.uint64))).sum())
