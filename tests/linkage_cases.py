"""Sketch sets for complete and average linkage (mhx_dist_linkage), shared by the CPU tests and the GPU tests: the sets of
tests/mst_cases.py and one of its own, `short`, whose lists are of very different lengths.  What the oracle and the rule
(tests/linkage_rule.py) say about a set is computed once per process."""
import functools

import numpy as np

from tests import linkage_rule as lr
from tests import mst_cases as mc
from tests import triangle_cases as tc

K = mc.K
LINKAGES = (lr.COMPLETE, lr.AVERAGE)


@functools.lru_cache(maxsize=None)
def short():
    """ten lists at s = 1000: two empty ones (0/0), one of 1 hash, one of 5, six of 300 .. 1000 hashes that share a base, so
    that denom varies from pair to pair"""
    rng = np.random.default_rng(75)
    base = tc.sketch_like(rng, 1000)
    lists = [base[:0].copy(), base[:0].copy(), base[:1].copy(), base[3:8].copy()]
    for length in (300, 450, 620, 777, 913, 1000):
        lists.append(tc.mutate(rng, base, float(rng.uniform(0.02, 0.5)))[:length].copy())
    return tuple(lists), 1000


# n = 2 and 3: one pick and one update; 33 and 65 cross the slice and wave borders; identical and disjoint: every value ties;
# chains and set200 exercise the cached partners
CASES = [("set70", ()), ("set200", ()), ("chains", ()), ("crowded", (40,)), ("identical", (70,)), ("disjoint", (70,)), ("duplicate_pairs", (64,)),
         ("tiny", (2,)), ("tiny", (3,)), ("tiny", (33,)), ("tiny", (65,)), ("short", ())]
SMALL = [c for c in CASES if c[0] not in ("set200", "chains")]   # where a test traces every step


def lists_of(name, args=()):
    return short() if name == "short" else mc.lists_of(name, args)


@functools.lru_cache(maxsize=None)
def pairs(name, args=(), k=K):
    if name == "short":
        lists, s = short()
        return tc.oracle_pairs(lists, s, k)
    return mc.pairs(name, args, k)


@functools.lru_cache(maxsize=None)
def expected(name, args, linkage, k=K):
    """the rule's merges of a case set, [(a, b, size, num, den)] in merge order, and their heights"""
    lists, _ = lists_of(name, args)
    common, denom, _ = pairs(name, args, k)
    merges = lr.agglomerate(common, denom, len(lists), k, linkage)
    return merges, lr.heights(merges, k, linkage)


@functools.lru_cache(maxsize=None)
def traced(name, args, linkage, k=K):
    """the same with the best partner of every row after every step"""
    lists, _ = lists_of(name, args)
    common, denom, _ = pairs(name, args, k)
    return lr.agglomerate(common, denom, len(lists), k, linkage, trace=True)
