"""CPU emulation of the single-linkage tree (auriclass_amd/csrc/mhx_mst.h, the very functions the kernels run):
tests/emul/mst_emul.cpp runs whole calls -- the five steps of every Boruvka round, from either pair source, over the blocks in
the kernels' order and shuffled, every proposal, choice and union to its end or interleaved access by access from a seed and
under an adversarial schedule.  The edge set equals the rule's (tests/mst_rule.py), the rounds stay within ceil(log2 n), and
every round appends as many edges as it loses components."""
import ctypes
import math

import numpy as np
import pytest

from tests import emul_build
from tests import mst_cases as mc
from tests import mst_rule as mr


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("mst_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_mst_precedes.argtypes = [u32] * 8
    L.emul_mst_precedes.restype = ctypes.c_int
    L.emul_mst_labels.argtypes = [vp, vp, vp, vp, u32, ctypes.c_int, ctypes.c_double, vp]
    L.emul_mst_labels.restype = u32
    L.emul_mst_call.argtypes = [vp, vp, u32, ctypes.c_int, u32, u64, u32, u64, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.emul_mst_call.restype = ctypes.c_int64
    return L


def call(L, name, args, stored, qbatch=1 << 16, shuffle=0, V=0, seed=0, adversarial=0):
    """(sorted edges, rounds, most retries) of one emulated call; the per-round counters are checked here"""
    lists, _ = mc.lists_of(name, args)
    common, denom, _ = mc.pairs(name, args)
    n = len(lists)
    out = [np.zeros(n, np.uint32) for _ in range(4)]
    rounds, retries = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lost, appended = np.zeros(64, np.uint32), np.zeros(64, np.uint32)
    m = L.emul_mst_call(common.ctypes.data, denom.ctypes.data, n, stored, qbatch, shuffle, V, seed, adversarial, *(o.ctypes.data for o in out),
                        ctypes.byref(rounds), lost.ctypes.data, appended.ctypes.data, ctypes.byref(retries))
    assert m == n - 1, m
    r = rounds.value
    assert 1 <= r <= max(1, math.ceil(math.log2(n)))
    assert np.array_equal(lost[:r], appended[:r]) and int(lost[:r].sum()) == n - 1 and (lost[:r] > 0).all()
    assert (out[0][:m] > out[1][:m]).all()
    return sorted(zip(*(o[:m].tolist() for o in out))), r, retries.value


def test_order_is_the_rules(emul):
    """mst_precedes against the rule's order on every pair of a handful of edges with ties at each level, and at 2^20 - 1"""
    big = (1 << 20) - 1
    edges = [(1, 0, 0, 0), (2, 0, 5, 5), (2, 1, 1, 2), (3, 0, 2, 4), (3, 1, 2, 4), (4, 1, 1, 2), (5, 4, 3, 4), (6, 0, 2, 3), (7, 2, 0, 9), (8, 2, 0, 1),
             (9, 0, big, big), (9, 1, big - 1, big), (9, 2, big - 2, big - 1), (9, 3, 1, big), (9, 4, 0, big)]
    for a in edges:
        for b in edges:
            assert bool(emul.emul_mst_precedes(a[2], a[3], a[0], a[1], b[2], b[3], b[0], b[1])) == mr.precedes(a, b), (a, b)


@pytest.mark.parametrize("name,args", mc.CASES)
def test_whole_calls_in_both_pair_sources(emul, name, args):
    """stored and recomputed (whole batches, and batches of 48 queries), in the kernels' order and in three shuffled orders"""
    want = sorted(mc.expected(name, args))
    seen_rounds = set()
    for stored, qbatch in ((1, 0), (0, 1 << 16), (0, 48)):
        for shuffle in (0, 1, 2, 3):
            got, rounds, _ = call(emul, name, args, stored, qbatch=qbatch, shuffle=shuffle)
            assert got == want, (stored, qbatch, shuffle)
            seen_rounds.add(rounds)
    assert len(seen_rounds) == 1   # the picks of a round do not depend on the order of arrival
    print(name, args, "rounds", seen_rounds)


@pytest.mark.parametrize("name,args", mc.CASES)
def test_interleaved_steps(emul, name, args):
    """64 virtual threads, one access to best / winner / parent per turn: six random schedules and six adversarial ones
    (every thread has loaded before anyone swaps) per pair source give the rule's edge set"""
    want = sorted(mc.expected(name, args))
    most = 0
    for stored in (1, 0):
        for adversarial in (0, 1):
            for seed in range(6):
                got, _, retries = call(emul, name, args, stored, qbatch=48, shuffle=seed % 2, V=64, seed=seed, adversarial=adversarial)
                assert got == want, (stored, adversarial, seed)
                most = max(most, retries)
    print("most retries of one proposal, choice or union:", most)
    if name in ("identical", "set70"):
        assert most > 0   # the schedules do make compare-and-swaps fail


def test_cut_of_the_header_equals_the_rules(emul):
    lists, _ = mc.set70()
    tree = mc.expected("set70")
    n = len(lists)
    ei, ej, ec, ed = (np.array(col, np.uint32) for col in zip(*tree))
    for T in np.unique(mr.distances(tree, mc.K)).tolist():
        for bound in (T, float(np.nextafter(T, -np.inf))):
            label = np.zeros(n, np.uint32)
            roots = emul.emul_mst_labels(ei.ctypes.data, ej.ctypes.data, ec.ctypes.data, ed.ctypes.data, n, mc.K, bound, label.ctypes.data)
            want_label, want_roots = mr.mst_labels(tree, n, mc.K, bound)
            assert roots == want_roots and np.array_equal(label, want_label), bound
