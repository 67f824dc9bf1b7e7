"""CPU emulation of the single-linkage clustering (auriclass_amd/csrc/mhx_cluster.h, the very functions the kernels run):
tests/emul/cluster_emul.cpp builds the cmin table with the library's builder, picks the edges of a call cell by cell in
the kernels' order, and runs the union -- one pair after the other in several orders, and many pairs at once with the
accesses to `parent` interleaved by a seeded schedule -- and the flatten pass.  Everything against the rule of
tests/cluster_rule.py."""
import ctypes
import time

import numpy as np
import pytest

from tests import cluster_cases as cc
from tests import cluster_rule as cr
from tests import emul_build

BOUNDS = (-0.1, 0.0, 1e-4, 0.011, 0.05, 0.3, 0.999, 1.0)
CASES = [("set70", (), 0.02), ("set70", (), 0.0), ("set200", (), 0.05), ("set200", (), 0.02), ("chains", (), cc.CHAINS_BOUND),
         ("crowded", (40,), 0.02), ("long_set", (40, 12_000), 0.05)]


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("cluster_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_cluster_cmin.argtypes = [u32, ctypes.c_int, ctypes.c_double, vp]
    L.emul_cluster_cmin.restype = None
    L.emul_cluster_edges.argtypes = [vp, vp, u32, u32, vp, u32, vp, vp, u64]
    L.emul_cluster_edges.restype = u64
    L.emul_cluster_sequential.argtypes = [u32, vp, vp, u64, u64, vp]
    L.emul_cluster_sequential.restype = u32
    L.emul_cluster_interleaved.argtypes = [u32, vp, vp, u64, u32, u64, ctypes.c_int, vp, vp]
    L.emul_cluster_interleaved.restype = ctypes.c_int64
    return L


def built_cmin(L, s, k, max_dist):
    out = np.zeros(s + 1, np.uint32)
    L.emul_cluster_cmin(s, k, max_dist, out.ctypes.data)
    return out


def emulated_edges(L, name, args, max_dist, qbatch=1 << 16):
    """the edges tri_cluster_kernel keeps, in its order: the oracle's counts through the library's table and schedule"""
    lists, s = getattr(cc, name)(*args)
    common, denom, _ = cc.pairs(name, cc.K, *args)
    cmin = built_cmin(L, s, cc.K, max_dist)
    ei, ej = np.zeros(common.size, np.uint32), np.zeros(common.size, np.uint32)
    m = L.emul_cluster_edges(common.ctypes.data, denom.ctypes.data, len(lists), qbatch, cmin.ctypes.data, s, ei.ctypes.data, ej.ctypes.data, common.size)
    return len(lists), ei[:m].copy(), ej[:m].copy()


@pytest.mark.parametrize("k", [5, 21, 27, 32])
def test_built_table_equals_the_linear_definition(emul, k):
    for max_dist in BOUNDS:
        assert np.array_equal(built_cmin(emul, 1000, k, max_dist), cr.cmin_table(1000, k, max_dist)), (k, max_dist)


def test_table_of_a_million_entries(emul):
    """s = 10^6 at one bound, well under a second; against the linear definition where a test can afford it (whole rows at
    some denoms, the largest included) and against its two-sided form -- cmin[d] passes, cmin[d] - 1 does not -- on every
    13th denom"""
    s, k, max_dist = 1_000_000, 21, 0.05
    t0 = time.perf_counter()
    cmin = built_cmin(emul, s, k, max_dist)
    took = time.perf_counter() - t0
    print("cmin of %d entries: %.3f s" % (s + 1, took))
    assert took < 1.0
    assert np.array_equal(cmin[:1001], cr.cmin_table(1000, k, max_dist))
    for d in (1001, 31_337, 250_000, s):
        assert cmin[d] == cr.cmin_at(d, k, max_dist), d
    for d in range(1, s + 1, 13):
        c = int(cmin[d])
        assert 0 < c <= d and cr.distance(c, d, k) <= max_dist < cr.distance(c - 1, d, k), d
    assert (np.diff(cmin.astype(np.int64)) >= 0).all() and (np.diff(cmin.astype(np.int64)) <= 1).all()


@pytest.mark.parametrize("name,args,max_dist", CASES)
def test_sequential_unions_in_any_order(emul, name, args, max_dist):
    """the kept pairs in block order (whole batches, and batches of 48 queries) and in three shuffled orders, with and without
    flatten passes in between: the labels of the rule every time"""
    want_label, _, want_clusters, want_edges = cc.expected(name, max_dist, cc.K, *args)
    n, ei, ej = emulated_edges(emul, name, args, max_dist)
    assert ei.size == want_edges and (ej < ei).all()
    lists, s = getattr(cc, name)(*args)
    assert sorted(zip(ei.tolist(), ej.tolist())) == sorted(cr.edges(lists, s, cc.K, max_dist, cc.pairs(name, cc.K, *args)))   # the integer rule is the rule
    n48, ei48, ej48 = emulated_edges(emul, name, args, max_dist, qbatch=48)
    assert sorted(zip(ei48.tolist(), ej48.tolist())) == sorted(zip(ei.tolist(), ej.tolist()))
    orders = [(ei, ej), (ei48, ej48)]
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(ei.size)
        orders.append((ei[p].copy(), ej[p].copy()))
    for a, b in orders:
        for flatten_every in (0, 7):
            parent = np.full(n, 0xFFFFFFFF, np.uint32)
            roots = emul.emul_cluster_sequential(n, a.ctypes.data, b.ctypes.data, a.size, flatten_every, parent.ctypes.data)
            assert roots == want_clusters and np.array_equal(parent, want_label)


@pytest.mark.parametrize("name,args,max_dist", [("chains", (), cc.CHAINS_BOUND), ("set200", (), 0.05), ("set200", (), 1.0)])
def test_interleaved_unions(emul, name, args, max_dist):
    """64 virtual threads, a pending pair each, one access to `parent` per turn: twenty random schedules and twenty
    adversarial ones (every thread has found its roots before any compare-and-swap of the round happens) give the rule's
    labels, nothing is ever hooked under a larger index, and no union retries more than n times.  At the bound 1 all 19 900
    pairs of set200 are edges of one cluster: as many failed compare-and-swaps as a schedule can make."""
    want_label, _, want_clusters, _ = cc.expected(name, max_dist, cc.K, *args)
    n, ei, ej = emulated_edges(emul, name, args, max_dist)
    rng = np.random.default_rng(9)
    p = rng.permutation(ei.size)   # neighbours of one chain into different threads
    ei, ej = ei[p].copy(), ej[p].copy()
    most = 0
    for adversarial in (0, 1):
        for seed in range(20):
            parent = np.full(n, 0xFFFFFFFF, np.uint32)
            retries = ctypes.c_uint32(0)
            roots = emul.emul_cluster_interleaved(n, ei.ctypes.data, ej.ctypes.data, ei.size, 64, seed, adversarial, parent.ctypes.data,
                                                  ctypes.byref(retries))
            assert roots == want_clusters, (adversarial, seed)
            assert np.array_equal(parent, want_label), (adversarial, seed)
            assert retries.value <= n
            most = max(most, retries.value)
    print("most retries of one union:", most)
    if max_dist == 1.0:
        assert most > 0   # the schedules do make compare-and-swaps fail
