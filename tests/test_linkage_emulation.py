"""CPU emulation of complete and average linkage (auriclass_amd/csrc/mhx_linkage.h, the very functions the kernels run):
tests/emul/linkage_emul.cpp runs whole calls -- init, the first scan, then pick, update and rescan of every step, in the kernels'
order and with every launch shuffled.  The merges equal the rule's (tests/linkage_rule.py), and behind every step nn[i] is the
rule's best partner of every row."""
import ctypes

import numpy as np
import pytest

from tests import emul_build
from tests import linkage_cases as lc
from tests import linkage_rule as lr

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("linkage_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_linkage_fixed_distance.argtypes = [u32, u32, ctypes.c_int]
    L.emul_linkage_fixed_distance.restype = u64
    L.emul_linkage_cmp.argtypes = [ctypes.c_int, u64, u64, u64, u64]
    L.emul_linkage_cmp.restype = ctypes.c_int
    L.emul_linkage_combine.argtypes = [ctypes.c_int, u64, u64]
    L.emul_linkage_combine.restype = u64
    L.emul_linkage_labels.argtypes = [vp, vp, vp, u32, ctypes.c_double, vp]
    L.emul_linkage_labels.restype = u32
    L.emul_linkage_call.argtypes = [vp, vp, u32, ctypes.c_int, ctypes.c_int, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.emul_linkage_call.restype = ctypes.c_int64
    return L


def call(L, name, args, linkage, seed=0, trace=False):
    """(merges [(a, b, size, num, den)], dist, nn trace or None, rescans) of one emulated call on a case set"""
    common, denom, _ = lc.pairs(name, args)
    return call_pairs(L, common, denom, len(lc.lists_of(name, args)[0]), linkage, seed, trace)


def call_pairs(L, common, denom, n, linkage, seed=0, trace=False):
    m = max(n - 1, 0)
    ma, mb, size = (np.zeros(m, np.uint32) for _ in range(3))
    num, den = (np.zeros(m, np.uint64) for _ in range(2))
    dist = np.zeros(m, np.float64)
    nn = np.zeros((m, n), np.uint32) if trace else None
    rescans = ctypes.c_uint64(0)
    got = L.emul_linkage_call(common.ctypes.data, denom.ctypes.data, n, lc.K, linkage, seed, ma.ctypes.data, mb.ctypes.data, size.ctypes.data, num.ctypes.data,
                              den.ctypes.data, dist.ctypes.data, nn.ctypes.data if trace else None, ctypes.byref(rescans))
    assert got == m, got
    return list(zip(ma.tolist(), mb.tolist(), size.tolist(), num.tolist(), den.tolist())), dist, nn, rescans.value


def test_header_arithmetic_is_the_rules(emul):
    """fixed distance, the order of two values and the combine of the header against the Python restatement"""
    C, A = lr.COMPLETE, lr.AVERAGE
    big = (1 << 20) - 1
    for k in (1, 21, 32):
        for c, d in ((0, 0), (0, 9), (9, 9), (1, 2), (2, 4), (1, big), (big - 1, big), (500, 1000), (999, 1000), (1, 1000), (17, 50_000)):
            assert emul.emul_linkage_fixed_distance(c, d, k) == lr.fixed_distance(c, d, k), (c, d, k)
    fractions = [(0, 0), (5, 5), (1, 2), (2, 4), (3, 4), (0, 9), (0, 1), (big, big), (big - 1, big), (big - 2, big - 1), (1, big)]
    for a in fractions:
        for b in fractions:
            wa, wb = a[0] << 32 | a[1], b[0] << 32 | b[1]
            assert emul.emul_linkage_cmp(C, wa, 1, wb, 1) == lr.closer(C, a, b), (a, b)
            w = emul.emul_linkage_combine(C, wa, wb)
            assert (w >> 32, w & 0xFFFFFFFF) == lr.combine(C, a, b), (a, b)
    values = [(0, 1), (1, 1), (3, 2), (6, 4), (1 << 62, 1 << 30), ((1 << 62) - 1, 1 << 30), ((1 << 62) - 1, (1 << 30) - 1), (1 << 32, 1), (5 << 32, 5)]
    for a in values:
        for b in values:
            assert emul.emul_linkage_cmp(A, a[0], a[1], b[0], b[1]) == lr.closer(A, a, b), (a, b)
    assert emul.emul_linkage_combine(A, 3, 6) == 9


@pytest.mark.parametrize("linkage", lc.LINKAGES)
@pytest.mark.parametrize("name,args", lc.CASES)
def test_whole_calls_give_the_rules_merges(emul, name, args, linkage):
    """in the kernels' order and in two shuffled orders: merges, values and heights are the rule's"""
    want, want_dist = lc.expected(name, args, linkage)
    n = len(lc.lists_of(name, args)[0])
    for seed in (0, 1, 2):
        got, dist, _, rescans = call(emul, name, args, linkage, seed)
        bad = [t for t in range(len(want)) if got[t] != want[t]]
        assert not bad, (seed, bad[:3], [got[t] for t in bad[:3]], [want[t] for t in bad[:3]])
        assert np.array_equal(dist, want_dist)
        assert rescans >= n - 1   # the merged row at least, every step
    if name in ("identical", "disjoint"):
        assert rescans == n - 1   # every value ties: list 0's cluster stays every row's first partner, only its own row is scanned again
    print(name, args, "rescans per step", rescans / max(n - 1, 1))


@pytest.mark.parametrize("linkage", lc.LINKAGES)
@pytest.mark.parametrize("name,args", lc.SMALL)
def test_the_cached_partner_is_the_rules_after_every_step(emul, name, args, linkage):
    merges, partners = lc.traced(name, args, linkage)
    n = len(lc.lists_of(name, args)[0])
    for seed in (0, 3):
        got, _, nn, _ = call(emul, name, args, linkage, seed, trace=True)
        assert got == merges
        for t, want in enumerate(partners):
            row = nn[t].tolist()
            assert {i: j for i, j in enumerate(row) if j != NONE} == want, (seed, t)


@pytest.mark.parametrize("linkage", lc.LINKAGES)
def test_random_triangles_with_ties_everywhere_and_with_none(emul, linkage):
    """packed triangles of n = 2 .. 60 lists drawn at random -- from four distinct values, so that nearly every comparison ties,
    and from thousands --: merges and the cached partner behind every step are the rule's"""
    rng = np.random.default_rng(77)
    for n in list(range(2, 14)) + [21, 34, 47, 60]:
        pairs = n * (n - 1) // 2
        for few in (True, False):
            denom = np.full(pairs, 4 if few else 1000, np.uint32)
            common = rng.integers(0, 4 if few else 1001, pairs).astype(np.uint32)
            merges, partners = lr.agglomerate(common, denom, n, lc.K, linkage, trace=True)
            for seed in (0, 5):
                got, _, nn, _ = call_pairs(emul, common, denom, n, linkage, seed, trace=True)
                assert got == merges, (n, few, seed)
                for t, want in enumerate(partners):
                    assert {i: j for i, j in enumerate(nn[t].tolist()) if j != NONE} == want, (n, few, seed, t)


def test_cut_of_the_header_equals_the_rules(emul):
    n = len(lc.lists_of("set70")[0])
    for linkage in lc.LINKAGES:
        merges, dist = lc.expected("set70", (), linkage)
        ma, mb = (np.array([m[x] for m in merges], np.uint32) for x in (0, 1))
        for T in np.unique(dist).tolist():
            for bound in (T, float(np.nextafter(T, -np.inf))):
                label = np.zeros(n, np.uint32)
                roots = emul.emul_linkage_labels(ma.ctypes.data, mb.ctypes.data, dist.ctypes.data, n, bound, label.ctypes.data)
                want, want_roots, _ = lr.labels(merges, dist, n, bound)
                assert roots == want_roots and np.array_equal(label, want), bound
