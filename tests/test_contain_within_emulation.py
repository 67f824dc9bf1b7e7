"""The host+device functions of auriclass_amd/csrc/mhx_contain_within.h run sequentially on the CPU
(tests/emul/contain_within_emul.cpp) over the pairs of the crowd case and of `mixed`: super-batches, the blocks of each in a
permuted order with every n-th taken out only after all others (the late fallback), the waves of every take-out drawing their
places in the arrival list in a shuffled order.  The resulting CSR equals the rule (tests/contain_within_rule.py) for every
permutation tried, with room to spare, with exactly enough, and -- row_off and the count -- with too little and with none."""
import ctypes

import numpy as np
import pytest

from tests import contain_cases as cc
from tests import contain_within_cases as cwc
from tests import contain_within_rule as rule
from tests import emul_build

K = cc.K


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("contain_within_emul")
    v, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emul_contain_within.argtypes = [v, v, v, u32, u32, u32, ctypes.c_int, ctypes.c_double, u32, u32, u64, u64, u32, v, v, v, v, v, u64, v]
    L.emul_contain_within.restype = u64
    return L


def counts_of(case):
    """(shared, n_qry, n_ref, limit of the need table)"""
    if case == "crowd":
        return cwc.matrix() + (cwc.S_R,)
    return cc.expected(case) + (cc.case(case)[3],)


def run(emul, case, bound, qbatch=0, cells=0, seed=0, late=0, cap=None, nq=None, nr=None):
    shared, n_qry, n_ref, limit = counts_of(case)
    nq, nr = shared.shape[0] if nq is None else nq, shared.shape[1] if nr is None else nr
    m = [np.ascontiguousarray(a[:nq, :nr]) for a in (shared, n_qry, n_ref)]
    row_off = np.full(nq + 1, 9, np.uint64)
    stats = np.zeros(5, np.uint64)
    if cap is None:   # the counting form
        n = emul.emul_contain_within(m[0].ctypes.data, m[1].ctypes.data, m[2].ctypes.data, nq, nr, limit, K, bound[0], bound[1], qbatch, cells, seed, late,
                                     row_off.ctypes.data, None, None, None, None, 0, stats.ctypes.data)
        return n, row_off, None, stats
    out = [np.full(max(cap, 1), 7, np.uint32) for _ in range(4)]
    n = emul.emul_contain_within(m[0].ctypes.data, m[1].ctypes.data, m[2].ctypes.data, nq, nr, limit, K, bound[0], bound[1], qbatch, cells, seed, late,
                                 row_off.ctypes.data, *[a.ctypes.data for a in out], cap, stats.ctypes.data)
    return n, row_off, out, stats


def want_of(case, bound, nq=None, nr=None):
    if case == "crowd":
        return cwc.expected(bound[0], bound[1], cwc.NQ if nq is None else nq, cwc.NR if nr is None else nr)
    return rule.csr(*cc.expected(case), K, bound[0], bound[1])


# (queries per block, cells of a super-batch, seed of the permutations, every late-th block taken out last)
FORMS = [(0, 0, 0, 0), (1, 0, 5, 0), (13, 0, 7, 3), (4, 100, 11, 2), (3, 45, 13, 4), (70, 11, 17, 1), (5, 770, 19, 5), (2, 0, 23, 2)]


@pytest.mark.parametrize("bound", cwc.bounds())
def test_crowd_equals_the_rule_for_every_permutation(emul, bound):
    want = want_of("crowd", bound)
    total = int(want[0][-1])
    seen = set()
    for qbatch, cells, seed, late in FORMS:
        n, row_off, out, stats = run(emul, "crowd", bound, qbatch, cells, seed, late, cap=total + 3)
        assert n == total and np.array_equal(row_off, want[0]), (qbatch, cells, seed, late)
        for a, w in zip(out, want[1:]):
            assert np.array_equal(a[:total], w) and (a[total:] == 7).all(), (qbatch, cells, seed, late)
        assert stats[3] == 0
        seen.add((int(stats[0]), int(stats[1]), int(stats[2]) > 0))
    assert {s[0] for s in seen} >= {1, 8, 18, 70} and any(s[2] for s in seen)   # one and many super-batches, blocks taken out late


@pytest.mark.parametrize("bound", [(0.0, 1), (0.9, 1), (0.95, 3)])
def test_mixed_equals_the_rule(emul, bound):
    """40 x 33 at s_r = 200: two slices, the second of one reference; n_ref runs over the whole need table"""
    want = want_of("mixed", bound)
    total = int(want[0][-1])
    assert total > 0
    for qbatch, cells, seed, late in FORMS:
        n, row_off, out, stats = run(emul, "mixed", bound, qbatch, cells, seed, late, cap=total)
        assert n == total and np.array_equal(row_off, want[0]) and all(np.array_equal(a, w) for a, w in zip(out, want[1:])), (qbatch, cells, seed, late)


def test_too_little_room_and_the_counting_form(emul):
    bound = cwc.MAIN[1]
    want = want_of("crowd", bound)
    total = int(want[0][-1])
    for qbatch, cells, seed, late in FORMS:
        n, row_off, out, _ = run(emul, "crowd", bound, qbatch, cells, seed, late, cap=total)
        assert n == total and all(np.array_equal(a, w) for a, w in zip(out, want[1:]))
        n, row_off, out, stats = run(emul, "crowd", bound, qbatch, cells, seed, late, cap=total - 1)
        assert n == total and np.array_equal(row_off, want[0])       # complete beside a list that did not fit
        n, row_off, out, stats = run(emul, "crowd", bound, qbatch, cells, seed, late, cap=10)   # less than one cell's run
        assert n == total and np.array_equal(row_off, want[0]) and (stats[3] > 0 or cells)
        n, row_off, _, stats = run(emul, "crowd", bound, qbatch, cells, seed, late)
        assert n == total and np.array_equal(row_off, want[0]) and stats[4] == 0   # no arrival list, no atomic


@pytest.mark.parametrize("nq,nr", [(1, 1), (3, 31), (4, 32), (5, 33), (70, 1), (1, 330)])
def test_shapes_around_a_slice(emul, nq, nr):
    for bound in ((0.0, 1), cwc.MAIN[0], (1.5, 1)):
        want = want_of("crowd", bound, nq, nr)
        total = int(want[0][-1])
        for qbatch, cells, seed, late in FORMS[:5]:
            n, row_off, out, _ = run(emul, "crowd", bound, qbatch, cells, seed, late, cap=total, nq=nq, nr=nr)
            assert n == total and np.array_equal(row_off, want[0]) and all(np.array_equal(a[:total], w) for a, w in zip(out, want[1:]))
