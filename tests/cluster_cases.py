"""Sketch sets for the single-linkage clustering (mhx_dist_cluster), shared by the CPU tests and the GPU tests: the sets of
tests/triangle_cases.py (set70, set200, long_set, crowded) and one of its own, chains(), in which every union is
indispensable.  What the rule (tests/cluster_rule.py) says about a set at a bound is computed once per process."""
import functools

import numpy as np

from tests import cluster_rule as cr
from tests import triangle_cases as tc
from tests.triangle_cases import crowded, long_set, set70, set200   # noqa: F401  (the case sets, by name)

K = 21
CHAINS_BOUND = 0.011


@functools.lru_cache(maxsize=None)
def chains():
    """150 lists at s = 1000: three chains of 50, 60 and 37 lists -- a fresh list, and every next one its predecessor with
    15 % of the hashes replaced --, three independent lists, and the whole set permuted.  At k = 21 consecutive lists of a
    chain lie 0.00615 .. 0.00917 apart, lists two steps apart at least 0.01268, everything else at least 0.0191: at the
    bound 0.011 the edges are exactly the 144 consecutive pairs -- each of them the only link between the two halves of its
    chain -- and after the permutation every chain runs through all five slices of 32 lists."""
    rng = np.random.default_rng(515)
    s = 1000
    lists = []
    for length in (50, 60, 37):
        lists.append(tc.sketch_like(rng, s))
        for _ in range(length - 1):
            lists.append(tc.mutate(rng, lists[-1], 0.15))
    lists += [tc.sketch_like(rng, s) for _ in range(3)]
    order = rng.permutation(len(lists))
    return tuple(lists[i] for i in order), s


@functools.lru_cache(maxsize=None)
def pairs(name, k=K, *args):
    """tc.oracle_pairs of a case set, once per process"""
    if name in ("set70", "set200"):
        return tc.expected(name, k, *args)   # shared with the triangle tests
    lists, s = globals()[name](*args)
    return tc.oracle_pairs(lists, s, k)


@functools.lru_cache(maxsize=None)
def expected(name, max_dist, k=K, *args):
    """(label, degree, n_clusters, n_edges) of the rule for a case set at a bound"""
    lists, s = globals()[name](*args)
    return cr.cluster(lists, s, k, max_dist, pairs(name, k, *args))


def middle_bound(name, *args):
    """a bound that splits the close pairs of a set: the middle one of the distinct oracle distances below 1"""
    dist = np.unique(pairs(name, K, *args)[2])
    dist = dist[dist < 1.0]
    return float(dist[dist.size // 2])
