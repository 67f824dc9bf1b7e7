"""CPU emulation of neighbour joining (auriclass_amd/csrc/mhx_nj.h, the very functions the kernels run):
tests/emul/nj_emul.cpp runs whole calls -- init, then scan, join and update of every join, in the kernels' order and with every
launch shuffled.  The records, the branch lengths and the count of clamped updates equal the rule's (tests/nj_rule.py)."""
import ctypes
import struct

import numpy as np
import pytest

from tests import emul_build
from tests import nj_cases as nc
from tests import nj_rule as nr
from tests.test_nj_rule import balanced, caterpillar, tree_facts


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("nj_emul")
    u32, u64, i64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p
    L.emul_nj_q.argtypes = [u32, u64, u64, u64]
    L.emul_nj_q.restype = i64
    L.emul_nj_precedes.argtypes = [i64, u32, u32, i64, u32, u32]
    L.emul_nj_join_word.argtypes = [u64, u64, u64, ctypes.POINTER(ctypes.c_int)]
    L.emul_nj_join_word.restype = u64
    L.emul_nj_lengths.argtypes = [u64, u32, u64, u64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.emul_nj_lengths.restype = None
    L.emul_nj_scan_blocks.argtypes = [u32, u32]
    L.emul_nj_scan_blocks.restype = u32
    L.emul_nj_call.argtypes = [vp, vp, vp, u32, ctypes.c_int, u64, u32, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(u64)]
    L.emul_nj_call.restype = i64
    return L


def call(L, n, common=None, denom=None, raw=None, seed=0, blocks=0):
    """(records [(a, b, d, r_a, r_b)], len_a, len_b, clamps) of one emulated call"""
    m = max(n - 1, 0)
    ja, jb = (np.zeros(m, np.uint32) for _ in range(2))
    d, ra, rb = (np.zeros(m, np.uint64) for _ in range(3))
    la, lb = (np.zeros(m, np.float64) for _ in range(2))
    clamps = ctypes.c_uint64(0)
    p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    got = L.emul_nj_call(p(common), p(denom), p(raw), n, nc.K, seed, blocks, ja.ctypes.data, jb.ctypes.data, d.ctypes.data, ra.ctypes.data, rb.ctypes.data,
                         la.ctypes.data, lb.ctypes.data, ctypes.byref(clamps))
    assert got == m, got
    return list(zip(ja.tolist(), jb.tolist(), d.tolist(), ra.tolist(), rb.tolist())), la, lb, clamps.value


def bits(x):
    return struct.pack("<d", float(x))


def test_header_arithmetic_is_the_rules(emul):
    """Q at the extremes, the candidate order, the update's floor and clamp, and both length formulas bit for bit"""
    ONE = nr.ONE
    top = 65535 * ONE
    for m in (3, 4, 257, 65536):
        for d in (0, 1, ONE - 1, ONE):
            for ri, rj in ((0, 0), (top, top), (0, top), (d, d), (12345678901234, 987654321)):
                assert emul.emul_nj_q(m, d, ri, rj) == nr.q_value(m, d, ri, rj), (m, d, ri, rj)
    assert emul.emul_nj_q(65536, ONE, 0, 0) == 65534 * ONE and emul.emul_nj_q(65536, 0, top, top) == -2 * top
    cands = [(-5, 0, 1), (-5, 0, 2), (-5, 1, 2), (-4, 0, 1), (0, 0, 1), (3, 0, 3), (-2 * top, 7, 9), (65534 * ONE, 2, 3)]
    for a in cands:
        for b in cands:
            assert bool(emul.emul_nj_precedes(*a, *b)) == (a < b), (a, b)
    none = (0, 0xFFFFFFFF, 0xFFFFFFFF)
    assert not emul.emul_nj_precedes(*none, *cands[0]) and emul.emul_nj_precedes(*cands[0], *none) and not emul.emul_nj_precedes(*none, *none)
    clamped = ctypes.c_int(0)
    for dac, dbc, dab in ((1, 2, 8), (5, 2, 4), (3, 1, 4), (3, 0, 4), (0, 0, 0), (0, 0, ONE), (ONE, ONE, 0), (ONE, ONE, ONE), (ONE, 0, ONE), (ONE - 1, 0, ONE),
                          (7, 8, 0), (7, 7, 1)):
        w = emul.emul_nj_join_word(dac, dbc, dab, ctypes.byref(clamped))
        assert (w, bool(clamped.value)) == nr.join_word(dac, dbc, dab), (dac, dbc, dab)
    la, lb = ctypes.c_double(0), ctypes.c_double(0)
    rng = np.random.default_rng(78)
    cases = [(ONE, 65536, top, 0), (ONE, 65536, 0, top), (0, 3, 0, 0), (1, 3, 0, 1), (ONE, 2, 0, 0), (12345, 2, 0, 0), (3, 5, 1, 0), (1, 4, 0, 0)]
    cases += [(int(rng.integers(0, ONE + 1)), int(rng.integers(3, 65537)), int(rng.integers(0, top)), int(rng.integers(0, top))) for _ in range(200)]
    for d, m, r_a, r_b in cases:
        emul.emul_nj_lengths(d, m, r_a, r_b, ctypes.byref(la), ctypes.byref(lb))
        want = nr.lengths(d, m, r_a, r_b)
        assert (bits(la.value), bits(lb.value)) == (bits(want[0]), bits(want[1])), (d, m, r_a, r_b)
    # the grid of a scan: one workgroup per 2048 words of the m longest rows, 1 .. 1024
    assert emul.emul_nj_scan_blocks(3, 3) == 1 and emul.emul_nj_scan_blocks(257, 257) == 17 and emul.emul_nj_scan_blocks(65536, 65536) == 1024
    assert emul.emul_nj_scan_blocks(65536, 3) == 96


@pytest.mark.parametrize("name,args", nc.CASES)
def test_whole_calls_give_the_rules_records(emul, name, args):
    """in the kernels' order, in three shuffled orders and with the spans cut elsewhere: records, lengths and clamps are the rule's"""
    want, want_clamps, want_la, want_lb = nc.expected(name, args)
    n = len(nc.lists_of(name, args)[0])
    common, denom, _ = nc.pairs(name, args)
    for seed, blocks in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 7), (0, 1024)):
        got, la, lb, clamps = call(emul, n, common, denom, seed=seed, blocks=blocks)
        bad = [t for t in range(len(want)) if got[t] != want[t]]
        assert not bad, (seed, blocks, bad[:3], [got[t] for t in bad[:3]], [want[t] for t in bad[:3]])
        assert la.tobytes() == want_la.tobytes() and lb.tobytes() == want_lb.tobytes()
        assert clamps == want_clamps


@pytest.mark.parametrize("edges", [caterpillar(), balanced()], ids=["caterpillar", "balanced"])
def test_raw_words_of_an_additive_matrix(emul, edges):
    """a raw matrix of distance words in place of common / denom: the additive trees of tests/test_nj_rule.py"""
    M, _ = tree_facts(edges)
    want, want_clamps = nr.join(nr.matrix_words(M))
    raw = np.array([M[i][j] for i in range(8) for j in range(i)], np.uint64)
    for seed in (0, 1, 2):
        got, la, lb, clamps = call(emul, 8, raw=raw, seed=seed)
        assert got == want and clamps == want_clamps == 0
        assert (la.tobytes(), lb.tobytes()) == tuple(x.tobytes() for x in nr.all_lengths(want))


def test_random_words_with_ties_everywhere_and_with_none(emul):
    """raw triangles of n = 2 .. 60 nodes drawn at random -- from four distinct values, so that Q ties often and the clamp acts,
    and from the whole range --: records and clamps are the rule's"""
    rng = np.random.default_rng(79)
    acted = 0
    for n in list(range(2, 14)) + [21, 34, 47, 60]:
        for few in (True, False):
            raw = (rng.integers(0, 4, n * (n - 1) // 2).astype(np.uint64) << np.uint64(30)) if few else rng.integers(0, nr.ONE + 1, n * (n - 1) // 2).astype(np.uint64)
            at = iter(raw.tolist())
            want, want_clamps = nr.join([[next(at) for _ in range(i)] for i in range(n)])
            acted += want_clamps
            for seed in (0, 5):
                got, _, _, clamps = call(emul, n, raw=raw, seed=seed)
                assert got == want and clamps == want_clamps, (n, few, seed)
    assert acted > 0
