"""The host+device functions of auriclass_amd/csrc/mhx_within.h run sequentially on the CPU (tests/emul/within_emul.cpp) over
the pairs of the shared case set: super-batches, the blocks of each in a permuted order with some taken out only after all
others (the late fallback), the waves of every take-out drawing their places in the arrival list in a shuffled order.  The
resulting CSR equals the rule (tests/within_rule.py) for every permutation tried, with room to spare, with exactly enough,
and -- row_off and the count -- with too little and with none."""
import ctypes

import numpy as np
import pytest

from tests import emul_build
from tests import within_cases as wc


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("within_emul")
    v = ctypes.c_void_p
    L.emul_within.argtypes = [v, v, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint64,
                              ctypes.c_uint64, ctypes.c_uint32, v, v, v, v, ctypes.c_uint64, v]
    L.emul_within.restype = ctypes.c_uint64
    return L


def run(emul, max_dist, qbatch=0, cells=0, seed=0, late=0, cap=None, nq=wc.NQ, nr=wc.NR):
    common, denom, _ = wc.matrix()
    c, d = np.ascontiguousarray(common[:nq, :nr]), np.ascontiguousarray(denom[:nq, :nr])
    row_off = np.full(nq + 1, 9, np.uint64)
    stats = np.zeros(4, np.uint64)
    if cap is None:   # the counting form
        n = emul.emul_within(c.ctypes.data, d.ctypes.data, nq, nr, wc.S, wc.K, max_dist, qbatch, cells, seed, late, row_off.ctypes.data, None, None, None, 0,
                             stats.ctypes.data)
        return n, row_off, None, stats
    out = [np.full(max(cap, 1), 7, np.uint32) for _ in range(3)]
    n = emul.emul_within(c.ctypes.data, d.ctypes.data, nq, nr, wc.S, wc.K, max_dist, qbatch, cells, seed, late, row_off.ctypes.data, out[0].ctypes.data,
                         out[1].ctypes.data, out[2].ctypes.data, cap, stats.ctypes.data)
    return n, row_off, out, stats


# (queries per block, cells of a super-batch, seed of the permutations, every late-th block taken out last)
FORMS = [(0, 0, 0, 0), (1, 0, 5, 0), (13, 0, 7, 3), (4, 100, 11, 2), (3, 45, 13, 4), (70, 11, 17, 1), (5, 770, 19, 5), (2, 0, 23, 2)]


@pytest.mark.parametrize("max_dist", wc.bounds())
def test_csr_equals_the_rule_for_every_permutation(emul, max_dist):
    want = wc.expected(max_dist)
    total = int(want[0][-1])
    seen = set()
    for qbatch, cells, seed, late in FORMS:
        n, row_off, out, stats = run(emul, max_dist, qbatch, cells, seed, late, cap=total + 3)
        assert n == total and np.array_equal(row_off, want[0]), (qbatch, cells, seed, late)
        for a, w in zip(out, want[1:4]):
            assert np.array_equal(a[:total], w) and (a[total:] == 7).all(), (qbatch, cells, seed, late)
        assert stats[3] == 0
        seen.add((int(stats[0]), int(stats[1]), int(stats[2]) > 0))
    assert {s[0] for s in seen} >= {1, 8, 18, 70} and any(s[2] for s in seen)   # one and many super-batches, blocks taken out late


def test_capacity_and_the_counting_form(emul):
    want = wc.expected(0.02)
    total = int(want[0][-1])
    for qbatch, cells, seed, late in FORMS:
        n, row_off, out, _ = run(emul, 0.02, qbatch, cells, seed, late, cap=total)
        assert n == total and all(np.array_equal(a, w) for a, w in zip(out, want[1:4]))
        n, row_off, out, stats = run(emul, 0.02, qbatch, cells, seed, late, cap=total - 1)
        assert n == total and np.array_equal(row_off, want[0])       # complete beside a list that did not fit
        n, row_off, out, stats = run(emul, 0.02, qbatch, cells, seed, late, cap=10)
        assert n == total and np.array_equal(row_off, want[0]) and (stats[3] > 0 or cells)
        n, row_off, _, _ = run(emul, 0.02, qbatch, cells, seed, late)
        assert n == total and np.array_equal(row_off, want[0])


@pytest.mark.parametrize("nq,nr", [(1, 1), (3, 31), (4, 32), (5, 33), (70, 1), (1, 330)])
def test_shapes_around_a_slice(emul, nq, nr):
    for max_dist in (0.0, 0.02, 1.0):
        want = wc.expected(max_dist, nq, nr)
        total = int(want[0][-1])
        for qbatch, cells, seed, late in FORMS[:5]:
            n, row_off, out, _ = run(emul, max_dist, qbatch, cells, seed, late, cap=total, nq=nq, nr=nr)
            assert n == total and np.array_equal(row_off, want[0]) and all(np.array_equal(a[:total], w) for a, w in zip(out, want[1:4]))
