"""Sketch sets for the single-linkage tree (mhx_dist_mst), shared by the CPU tests and the GPU tests: the sets of
tests/cluster_cases.py (set70, set200, chains, long_set, crowded) and some of its own -- all lists identical, all disjoint,
duplicate pairs, and tiny sets that reach across a slice border.  What the oracle and the rule (tests/mst_rule.py) say about
a set is computed once per process."""
import functools

import numpy as np

from tests import cluster_cases as cc
from tests import mst_rule as mr
from tests import triangle_cases as tc
from tests.cluster_cases import chains, crowded, long_set, set70, set200   # noqa: F401  (the case sets, by name)

K = cc.K


@functools.lru_cache(maxsize=None)
def identical(n=70):
    """n copies of one list: every index is 1/1, the order is (lo, hi) alone and the tree is the star at list 0"""
    base = tc.sketch_like(np.random.default_rng(71), 1000)
    return tuple(base.copy() for _ in range(n)), 1000


@functools.lru_cache(maxsize=None)
def disjoint(n=70):
    """n lists that share no hash (list i holds the values = i mod n of one long list): every index is 0"""
    pool = tc.sketch_like(np.random.default_rng(72), 200 * n)
    return tuple(pool[i::n].copy() for i in range(n)), 1000


@functools.lru_cache(maxsize=None)
def duplicate_pairs(n=64):
    """n / 2 independent lists, each twice (i and i + n / 2): n / 2 edges at 1/1, the rest among independent lists"""
    rng = np.random.default_rng(73)
    half = [tc.sketch_like(rng, 1000) for _ in range(n // 2)]
    return tuple(half + [h.copy() for h in half]), 1000


@functools.lru_cache(maxsize=None)
def tiny(n):
    """the first n lists of a set of 65 in which neighbours share hashes at many levels: n = 2, 3, 33 (one pair across the
    border of the first slice) and 65 (three slices)"""
    rng = np.random.default_rng(74)
    lists = [tc.sketch_like(rng, 1000)]
    for i in range(1, 65):
        lists.append(tc.mutate(rng, lists[rng.integers(0, i)], float(rng.uniform(0.01, 0.6))))
    return tuple(lists[:n]), 1000


# (name, args) of every case of the issue; long_set(40, 20 000) is the GPU's windowed finish on top
CASES = [("set70", ()), ("set200", ()), ("chains", ()), ("long_set", (40, 12_000)), ("crowded", (40,)), ("identical", (70,)),
         ("disjoint", (70,)), ("duplicate_pairs", (64,)), ("tiny", (2,)), ("tiny", (3,)), ("tiny", (33,)), ("tiny", (65,))]


def lists_of(name, args=()):
    return globals()[name](*args)


@functools.lru_cache(maxsize=None)
def pairs(name, args=(), k=K):
    """tc.oracle_pairs of a case set, once per process (shared with the cluster and triangle tests where they have it)"""
    if name in ("set70", "set200", "chains", "long_set", "crowded"):
        return cc.pairs(name, k, *args)
    lists, s = lists_of(name, args)
    return tc.oracle_pairs(lists, s, k)


@functools.lru_cache(maxsize=None)
def expected(name, args=(), k=K):
    """the rule's tree of a case set: [(i, j, common, denom)] in edge order"""
    lists, _ = lists_of(name, args)
    common, denom, _ = pairs(name, args, k)
    return mr.kruskal(common, denom, len(lists))
