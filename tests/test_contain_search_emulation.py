"""CPU emulation of the containment search's take-out (auriclass_amd/csrc/mhx_contain_search.h, the very functions the kernel
runs): tests/emul/contain_search_emul.cpp feeds the candidates of every block of the schedule through contain_keep and
contain_insert -- in the schedule's order, in reversed block order, and with flagged blocks delivered behind their group, as
the engine redoes them -- and all three must give the rule's lists (tests/contain_search_rule.py) on every case of
tests/contain_cases.py and on the tie case of tests/contain_search_cases.py.  The order on its own: strict, total, the rule's."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import contain_cases as cc
from tests import contain_search_cases as csc
from tests import contain_search_rule as rule
from tests import emul_build

K = cc.K
CASES = ("crafted",) + cc.NAMES + ("ties",)


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("contain_search_emul")
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    L.emul_contain_better.argtypes = [u32] * 6
    L.emul_contain_better.restype = ctypes.c_int
    L.emul_contain_insert_many.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp]
    L.emul_contain_insert_many.restype = u32
    L.emul_contain_search.argtypes = [vp, vp, vp, u32, u32, u32, ctypes.c_int, vp, u32, ctypes.c_int, ctypes.c_double, u32, u32, u32, vp, vp, vp, vp, vp]
    L.emul_contain_search.restype = ctypes.c_int64
    return L


def counts_of(name):
    return csc.expected() if name == "ties" else cc.expected(name)


def sweep():
    """(ref, shared, n_ref): equal shares with different counts (1/2, 2/4, 500/1000; 3/3, 200/200), products beyond 2^32"""
    big = 2 ** 32 - 1
    fr = [(1, 1), (7, 7), (big, big), (1, 2), (2, 4), (500, 1000), (1, big), (big - 1, big), (big - 2, big - 1), (2 ** 31, big),
          (2 ** 31 - 1, big - 2), (65536, 65537), (65535, 65536), (3, 1000), (999, 1000), (49_999, 50_000), (3, 3), (200, 200)]
    return [(r, c, d) for r, (c, d) in zip(itertools.cycle([5, 2, 9, 2 ** 32 - 1, 0]), fr)] + [(4, 1, 2), (6, 2, 4), (1, 7, 7)]


def test_better_is_a_strict_total_order(emul):
    items = sweep()
    b = lambda x, y: bool(emul.emul_contain_better(*x, *y))
    for x in items:
        assert not b(x, x)
        for y in items:
            assert b(x, y) == rule.better(x, y)                 # the library's order is the rule's
            if x != y:
                assert b(x, y) != b(y, x), (x, y)               # antisymmetric, and total: distinct references never tie
    for x, y, z in itertools.product(items, repeat=3):
        if b(x, y) and b(y, z):
            assert b(x, z), (x, y, z)                          # transitive


@pytest.mark.parametrize("top", [1, 5, 64])
def test_insertion_does_not_depend_on_the_order_of_arrival(emul, top):
    shared, n_qry, n_ref = csc.expected()
    rng = np.random.default_rng(top)
    ref = np.arange(70, dtype=np.uint32)
    for q in range(6):
        c, d = np.ascontiguousarray(shared[q]), np.ascontiguousarray(n_ref[q])
        live = np.flatnonzero(c > 0).astype(np.uint32)
        want = rule.select([(r, int(c[r]), int(d[r]), 0) for r in range(70)], K, top)
        want = [[h[a] for h in want] for a in range(3)]
        for order in (live, live[::-1], rng.permutation(live)):
            order = np.ascontiguousarray(order, np.uint32)
            out = [np.zeros(top, np.uint32) for _ in range(3)]
            m = emul.emul_contain_insert_many(ref.ctypes.data, c.ctypes.data, d.ctypes.data, order.ctypes.data, order.size, top, *[a.ctypes.data for a in out])
            assert [a[:m].tolist() for a in out] == want, q


def run_emul(L, counts, top, min_identity=0.0, min_shared=1, qbatch=0, reverse=0, flagged=None, group=0, k=K):
    shared, n_qry, n_ref = (np.ascontiguousarray(a, np.uint32) for a in counts)
    nq, nr = shared.shape
    out = [np.full((nq, top), 0xFFFFFFFF, np.uint32) for _ in range(4)] + [np.full(nq, 0xFFFFFFFF, np.uint32)]
    blocks = -(-nq // (qbatch or nq)) * -(-nr // 32)
    flags = None if flagged is None else np.ascontiguousarray(flagged(blocks), np.uint8)
    rc = L.emul_contain_search(shared.ctypes.data, n_qry.ctypes.data, n_ref.ctypes.data, nq, nr, qbatch, reverse, None if flags is None else flags.ctypes.data,
                               group, k, min_identity, min_shared, int(n_ref.max()), top, *[a.ctypes.data for a in out])
    assert rc == blocks
    return out


def same(got, want, what):
    for name, a, b in zip(("ref", "shared", "n_ref", "n_qry", "n_hits"), got, want):
        assert np.array_equal(a, b), (what, name)


@pytest.mark.parametrize("name", CASES)
def test_every_order_of_delivery_gives_the_rules_lists(emul, name):
    """the schedule's order, the blocks last to first, and flagged blocks (every third, or all) behind their group -- whole
    call or groups of four blocks; query batches of 1, 5 and all"""
    counts = counts_of(name)
    every_third = lambda n: np.arange(n) % 3 == 1
    everything = lambda n: np.ones(n, bool)
    for top, min_identity, min_shared in ((5, 0.0, 1), (64, 0.0, 1), (1, 0.0, 1), (5, 0.95, 3), (64, 1.0, 1)):
        want = rule.arrays(rule.search(*counts, K, top, min_identity, min_shared), top)
        if name in ("mixed", "plasmids", "ties") and (top, min_identity) == (5, 0.0):
            assert want[4].max() > 0
        for form in (dict(), dict(reverse=1), dict(flagged=every_third), dict(qbatch=5), dict(qbatch=5, reverse=1), dict(qbatch=1, flagged=every_third, group=4),
                     dict(qbatch=5, reverse=1, flagged=every_third), dict(flagged=everything, group=4)):
            same(run_emul(emul, counts, top, min_identity, min_shared, **form), want, (name, top, min_identity, form))


def test_the_tie_case_holds_its_ties(emul):
    """references 3, 35 and 67 are one list: they follow one another in index order, in every query that hits them; query 0
    holds the short reference 10 whole, 50/50 behind the 200/200 of the full ones.  Read off the lists the header's functions
    make when the three slices arrive last to first (the rule's lists, which the test above has compared them with)."""
    shared, n_qry, n_ref = csc.expected()
    got = run_emul(emul, csc.expected(), 64, reverse=1)
    res = [list(zip(*[a[q, :got[4][q]].tolist() for a in got[:4]])) for q in range(6)]
    assert res == rule.search(shared, n_qry, n_ref, K, 64)
    assert [h[0] for h in res[0][:5]] == [3, 11, 35, 67, 10]
    assert [(h[1], h[2]) for h in res[0][:5]] == [(200, 200)] * 4 + [(50, 50)]
    for q in (0, 1, 2):
        at = [h[0] for h in res[q]].index(3)
        trio = res[q][at:at + 3] if q else [res[q][0], res[q][2], res[q][3]]
        assert [h[0] for h in trio] == [3, 35, 67] and len({h[1:] for h in trio}) == 1
    assert 0 < res[2][0][1] < res[2][0][2]           # the mutant: a share below 1
    assert len(res[4]) == 0                          # the empty query
    assert [h[0] for h in res[5][:3]] == [20, 40, 66] and all(h[1] == h[2] == 200 for h in res[5][:3])
    assert rule.search(shared, n_qry, n_ref, K, 1)[1] == [res[1][0]] and res[1][0][0] == 3
