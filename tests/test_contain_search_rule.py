"""The rule of the containment search (tests/contain_search_rule.py) on hand-made candidates -- every list also through the header's
own order, hit test and insertion (auriclass_amd/csrc/mhx_contain_search.h, through the emulator) --, and the need[] table that carries
the identity bound to the device -- the header's own builder (auriclass_amd/csrc/mhx_contain_search.h: contain_need_build,
through tests/emul/contain_search_emul.cpp) against the predicate it encodes, value by value.  No GPU; also that the entry
points are declared, exported and bound."""
import ctypes

import numpy as np
import pytest

from auriclass_amd import engine
from tests import contain_search_rule as rule
from tests import emul_build

K = 21


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("contain_search_emul")
    L.emul_contain_need.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p]
    L.emul_contain_need.restype = None
    L.emul_contain_keep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    L.emul_contain_keep.restype = ctypes.c_int
    L.emul_contain_better.argtypes = [ctypes.c_uint32] * 6
    L.emul_contain_better.restype = ctypes.c_int
    L.emul_contain_insert_many.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 3
    L.emul_contain_insert_many.restype = ctypes.c_uint32
    return L


def select(emul, cands, k, top, min_identity=0.0, min_shared=1):
    """rule.select of the candidates -- after the header's own functions have given the same list: the need table of
    contain_need_build, contain_keep on every candidate, and contain_insert one candidate after the other, in the order
    given and in the reverse one"""
    want = rule.select(cands, k, top, min_identity, min_shared)
    limit = max(c[2] for c in cands)
    need = np.zeros(limit + 1, np.uint32)
    emul.emul_contain_need(limit, k, min_identity, min_shared, need.ctypes.data)
    ref, shared, n_ref = (np.array([c[i] for c in cands], np.uint32) for i in range(3))
    kept = [i for i, c in enumerate(cands) if emul.emul_contain_keep(c[1], c[2], need.ctypes.data, limit)]
    assert kept == [i for i, c in enumerate(cands) if rule.is_hit(c[1], c[2], k, min_identity, min_shared)]
    for order in (kept, kept[::-1]):
        order = np.array(order, np.uint32)
        out = [np.zeros(top, np.uint32) for _ in range(3)]
        m = emul.emul_contain_insert_many(ref.ctypes.data, shared.ctypes.data, n_ref.ctypes.data, order.ctypes.data, order.size, top, *[a.ctypes.data for a in out])
        assert list(zip(*[a[:m].tolist() for a in out])) == [h[:3] for h in want]
    return want


def refs_of(result):
    return [h[0] for h in result]


def test_more_evidence_ranks_first_on_equal_shares(emul):
    """2/4 behind 100/200, 3/3 behind 200/200, and a larger share before both whatever its size"""
    cands = [(0, 2, 4, 9), (1, 100, 200, 9), (2, 3, 3, 9), (3, 200, 200, 9), (4, 3, 5, 9)]
    assert refs_of(select(emul, cands, K, 5)) == [3, 2, 4, 1, 0]
    assert rule.better((1, 100, 200), (0, 2, 4)) and not rule.better((0, 2, 4), (1, 100, 200))
    # the cross product is exact where doubles are not: (2^32 - 2) / (2^32 - 1) against (2^32 - 3) / (2^32 - 2)
    big = 2 ** 32 - 1
    assert rule.better((9, big - 1, big), (1, big - 2, big - 1)) and not rule.better((1, big - 2, big - 1), (9, big - 1, big))
    assert emul.emul_contain_better(9, big - 1, big, 1, big - 2, big - 1) == 1 and emul.emul_contain_better(1, big - 2, big - 1, 9, big - 1, big) == 0
    assert emul.emul_contain_better(1, 100, 200, 0, 2, 4) == 1 and emul.emul_contain_better(0, 2, 4, 1, 100, 200) == 0


def test_equal_share_and_equal_shared_go_by_the_lower_index(emul):
    cands = [(7, 50, 100, 1), (2, 50, 100, 2), (5, 50, 100, 3), (9, 25, 50, 4)]
    assert refs_of(select(emul, cands, K, 4)) == [2, 5, 7, 9]
    assert select(emul, cands, K, 4)[0] == (2, 50, 100, 2)   # the entry travels whole, n_qry with it


def test_nothing_shared_and_empty_references_are_never_hits(emul):
    cands = [(0, 0, 10, 10), (1, 0, 0, 0), (2, 0, 0, 7), (3, 1, 1000, 5)]
    assert refs_of(select(emul, cands, K, 64)) == [3]
    assert refs_of(select(emul, cands, K, 64, min_identity=-1.0)) == [3]   # not even below every bound
    assert not rule.is_hit(0, 0, K) and not rule.is_hit(0, 5, K, min_identity=-1.0)


def test_the_floor_on_shared(emul):
    """a one-hash reference inside a tiny window reaches 1/1: the floor keeps the top list from filling with such pairs"""
    cands = [(0, 1, 1, 3), (1, 2, 2, 3), (2, 180, 200, 900), (3, 19, 19, 40), (4, 20, 400, 700)]
    assert refs_of(select(emul, cands, K, 5)) == [3, 1, 0, 2, 4]
    assert refs_of(select(emul, cands, K, 5, min_shared=2)) == [3, 1, 2, 4]
    assert refs_of(select(emul, cands, K, 5, min_shared=20)) == [2, 4]
    assert refs_of(select(emul, cands, K, 5, min_shared=181)) == []


def test_identity_one_keeps_exactly_the_contained(emul):
    cands = [(0, 199, 200, 1), (1, 200, 200, 1), (2, 1, 1, 1), (3, 49_999, 50_000, 1), (4, 50_000, 50_000, 1)]
    assert refs_of(select(emul, cands, K, 64, min_identity=1.0)) == [4, 1, 2]
    assert refs_of(select(emul, cands, K, 64, min_identity=1.5)) == []
    assert refs_of(select(emul, cands, K, 64, min_identity=0.9999)) == [4, 1, 2, 3]      # (199/200)^(1/21) = 0.99976
    assert refs_of(select(emul, cands, K, 64, min_identity=0.999)) == [4, 1, 2, 3, 0]


def test_top_cuts_the_ranked_hits(emul):
    rng = np.random.default_rng(64)
    n_ref = rng.integers(1, 300, size=100)
    shared = (n_ref * rng.random(100)).astype(np.int64)
    cands = [(r, int(shared[r]), int(n_ref[r]), 0) for r in range(100)]
    full = rule.ranked([c for c in cands if c[1] >= 1])
    assert 64 < len(full) <= 100
    for a, b in zip(full, full[1:]):
        assert rule.better(a, b) and not rule.better(b, a)
    assert select(emul, cands, K, 1) == full[:1] and select(emul, cands, K, 64) == full[:64]       # more hits than top
    few = select(emul, cands, K, 64, min_identity=0.99)
    assert 0 < len(few) < 64 and few == [c for c in full if rule.is_hit(c[1], c[2], K, 0.99)]      # fewer
    with pytest.raises(AssertionError):
        rule.select(cands, K, 65)
    # the vectorised form of the rule is the rule
    S, N = np.array([shared, shared[::-1]], np.uint32), np.array([n_ref, n_ref], np.uint32)
    S = np.minimum(S, N)
    for top, mi, ms in ((1, 0.0, 1), (64, 0.0, 1), (5, 0.97, 3)):
        want = rule.arrays(rule.search(S, N + 1, N, K, top, mi, ms), top)
        got = rule.search_np(S, N + 1, N, rule.need_table(300, K, mi, ms), top)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("k", [16, 21, 32])
@pytest.mark.parametrize("min_identity", [0.0, 0.9, 0.99, 1.0, 1.5])
def test_need_table_is_the_predicate(emul, k, min_identity):
    """every (shared, n_ref) up to n_ref = 300 and the whole rows n_ref = 1000 and 50 000: shared >= need[n_ref] iff the pair is
    a hit -- which also says that the identity never falls when `shared` rises, what makes one threshold per n_ref the rule"""
    limit = 50_000
    for min_shared in (1, 7):
        need = np.zeros(limit + 1, np.uint32)
        emul.emul_contain_need(limit, k, min_identity, min_shared, need.ctypes.data)
        assert need[0] == 1
        assert need[:301].tolist() == rule.need_table(300, k, min_identity, min_shared)
        for n in list(range(301)) + [1000, 50_000]:
            assert need[n] == n + 1 or min_shared <= need[n] <= n
            hits = np.array([rule.is_hit(c, n, k, min_identity, min_shared) for c in range(n + 1)])
            assert np.array_equal(hits, np.arange(n + 1) >= need[n]), (n, int(need[n]))
        if min_identity > 1.0:
            assert np.array_equal(need, np.arange(1, limit + 2))
        if min_identity == 1.0:
            assert np.array_equal(need[min_shared:], np.arange(min_shared, limit + 1))
        # the device's test reads the table inside its bounds only
        assert emul.emul_contain_keep(5, limit + 1, need.ctypes.data, limit) == 0
        assert emul.emul_contain_keep(1000, 1000, need.ctypes.data, limit) == (1 if need[1000] <= 1000 else 0)   # (shared <= n_ref always)
        assert emul.emul_contain_keep(int(need[1000]) - 1, 1000, need.ctypes.data, limit) == 0


def test_entry_points_are_declared_exported_and_bound():
    declared = engine.declared_symbols()
    engine.build()
    lib = engine.load()
    for name in ("mhx_dist_contain_search", "mhx_contain_files_search"):
        assert name in declared, f"include/mhx.h does not declare {name}"
        assert getattr(lib, name).argtypes, name
    assert ctypes.sizeof(engine.ContainSearchOpts) == 32
    for fn in ("dist_contain_search", "dist_contain_search_device"):
        assert callable(getattr(engine, fn))
