"""Sketch sets for neighbour joining (mhx_dist_nj), shared by the CPU tests and the GPU tests: the sets of
tests/linkage_cases.py and one of its own, `tiny257`, whose 257 nodes cross the border of a 256-thread workgroup in the
update.  What the oracle and the rule (tests/nj_rule.py) say about a set is computed once per process."""
import functools

import numpy as np

from tests import linkage_cases as lc
from tests import nj_rule as nr
from tests import triangle_cases as tc

K = lc.K


@functools.lru_cache(maxsize=None)
def tiny257():
    """257 lists built as mst_cases.tiny builds its 65: every list a mutated copy of an earlier one, so that neighbours share
    hashes at many levels"""
    rng = np.random.default_rng(76)
    lists = [tc.sketch_like(rng, 1000)]
    for i in range(1, 257):
        lists.append(tc.mutate(rng, lists[rng.integers(0, i)], float(rng.uniform(0.01, 0.6))))
    return tuple(lists), 1000


# n = 2: no scan; n = 3: one scan; 33 and 65 cross wave borders, 257 a workgroup border; identical and disjoint: every Q ties
CASES = list(lc.CASES) + [("tiny257", ())]


def lists_of(name, args=()):
    return tiny257() if name == "tiny257" else lc.lists_of(name, args)


@functools.lru_cache(maxsize=None)
def pairs(name, args=(), k=K):
    if name == "tiny257":
        lists, s = tiny257()
        return tc.oracle_pairs(lists, s, k)
    return lc.pairs(name, args, k)


@functools.lru_cache(maxsize=None)
def expected(name, args=(), k=K):
    """(records [(a, b, d, r_a, r_b)] in join order, updates the clamp changed, len_a, len_b) of a case set by the rule"""
    lists, _ = lists_of(name, args)
    common, denom, _ = pairs(name, args, k)
    records, clamps = nr.records_of(common, denom, len(lists), k)
    return (records, clamps) + nr.all_lengths(records)
