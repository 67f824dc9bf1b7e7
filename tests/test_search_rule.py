"""CPU-side checks of the reference-set search: the restated rule (tests/search_rule.py) against a brute-force sort by exact
fractions, its corner cases (0/0, a small k where distinct indices print distance 1), the conditions the shared case set
(tests/search_cases.py) must satisfy, and the new entry points: declared, exported, and refusing to compute without a GPU
engine."""
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import search_cases as sc
from tests import search_rule as rule
from tests import triangle_cases as tc

NEW = ["mhx_dist_search", "mhx_search_files"]


@pytest.fixture(scope="module")
def lib():
    engine.build()
    return engine.load()


def brute(pairs, top, max_dist):
    """the same selection by another route: exact fractions as sort keys"""
    key = lambda p: (-(Fraction(1) if p[1] == p[2] else Fraction(p[1], p[2])), p[0])
    return sorted((p for p in pairs if p[3] <= max_dist), key=key)[:top]


def test_rule_equals_a_brute_force_sort():
    rng = np.random.default_rng(77)
    k = 21
    for trial in range(40):
        n = int(rng.integers(1, 120))
        denom = rng.choice([1, 2, 4, 7, 1000, 50_000, 2 ** 32 - 1], size=n)
        common = [int(rng.integers(0, d + 1)) for d in denom]
        if trial % 4 == 0:   # equal indices written differently, and the top of the order three ways
            common[:6], denom[:6] = [1, 2, 500, 7, 0, 1000][:n], [2, 4, 1000, 7, 0, 1000][:n]
        pairs = []
        for r in range(n):
            c, d = int(common[r]), int(denom[r])
            j = 1.0 if c == d else c / d
            dist = 0.0 if c == d else (1.0 if c == 0 else min(1.0, -np.log(2 * j / (1 + j)) / k))
            pairs.append((r, c, d, float(dist)))
        for top in (1, 5, 64):
            for max_dist in (0.0, 0.03, 0.3, 1.0):
                assert rule.select(pairs, top, max_dist) == brute(pairs, top, max_dist)
    a, b = (3, 1, 2), (9, 2, 4)
    assert rule.better(a, b) and not rule.better(b, a)   # equal index: the lower reference
    assert rule.better((9, 2 ** 32 - 1, 2 ** 32 - 1), (3, 2 ** 32 - 2, 2 ** 32 - 1))   # products beyond 2^32, compared exactly


def test_two_empty_lists_are_a_hit_at_distance_zero():
    empty, some = np.zeros(0, np.uint64), np.arange(1, 50, dtype=np.uint64)
    assert mo.compare(empty, empty, 1000, 21) == (0, 0, 0.0)
    got = rule.search([empty], [some, empty, some[:3], empty], 1000, 21, 5, 0.0)[0]
    assert got == [(1, 0, 0, 0.0), (3, 0, 0, 0.0)]   # 0/0 counts as 1/1; everything else is 0/n at distance 1
    got = rule.search([empty], [some, empty, some[:3], empty], 1000, 21, 3, 1.0)[0]
    assert [h[0] for h in got] == [1, 3, 0]
    assert rule.better((8, 0, 0), (2, 999, 1000)) and rule.better((2, 5, 5), (8, 0, 0))


def test_small_k_ranks_by_the_index_where_every_distance_prints_as_one():
    """k = 4, hashes below 2^32: sharing 1 .. 8 of 1000 hashes gives Jaccard indices below 0.0092, all at distance 1 after
    the clamp -- the order still follows the index"""
    rng = np.random.default_rng(44)
    k, s = 4, 1000
    query = tc.sketch_like(rng, s, hi=2 ** 32)
    refs, shared = [], [3, 8, 1, 5, 2, 7, 4, 6, 1, 0]
    for c in shared:
        own = tc.sketch_like(rng, s + 50, hi=2 ** 32)
        own = own[~np.isin(own, query)][:s - c]
        refs.append(np.unique(np.concatenate([query[:c], own])))   # the smallest hashes: inside the first s of the union
    got = rule.search([query], refs, s, k, 64, 1.0)[0]
    assert len(got) == len(refs) and all(h[3] == 1.0 for h in got)
    assert len({Fraction(h[1], h[2]) for h in got}) >= 8          # distinct indices ...
    fr = [Fraction(h[1], h[2]) for h in got]
    assert fr == sorted(fr, reverse=True)                         # ... in descending order
    assert [h[0] for h in got if h[1] == got[-2][1]] == sorted(h[0] for h in got if h[1] == got[-2][1])
    assert rule.search([query], refs, s, k, 3, 0.999)[0] == []   # and none of them is a hit below the clamp


def test_case_set_exercises_truncation_short_and_empty_lists():
    """the conditions the construction must satisfy (k = 21), whatever the exact figures"""
    common, denom, dist = sc.matrix()
    assert common.shape == (150, 200) and len(sc.queries()[:40]) == 40
    h = sc.hits_per_query(0.05)
    print("max_dist 0.05: more than 5 hits", int((h > 5).sum()), "1..5 hits", int(((h > 0) & (h <= 5)).sum()), "none", int((h == 0).sum()))
    assert (h > 5).any() and ((h > 0) & (h <= 5)).any() and (h == 0).any() and h.max() <= 64
    h40 = sc.hits_per_query(0.05, 40)
    assert (h40 > 5).any() and ((h40 > 0) & (h40 <= 5)).any() and (h40 == 0).any()
    h0 = sc.hits_per_query(0.0)
    assert h0.max() == 4 and (h0 == 0).any() and ((h0 > 1) & (h0 <= 5)).any()
    assert (sc.hits_per_query(1.0) == 200).all()
    ref, c, d, x, n = sc.expected(5, 0.0)
    assert ref[24, :4].tolist() == [5, 190, 191, 196] and n[24] == 4    # the four-way tie in index order
    assert ref[25, :2].tolist() == [77, 141] and n[25] == 2
    assert n[26] == 1 and (ref[26, 0], c[26, 0], d[26, 0], x[26, 0]) == (33, 0, 0, 0.0)   # 0/0 against the empty reference
    ties = 0
    for q in range(150):
        hit = np.flatnonzero(dist[q] <= 0.2)
        fr = [Fraction(int(common[q, r]), int(denom[q, r])) if denom[q, r] else Fraction(1) for r in hit]
        ties += len(fr) - len(set(fr))
    print("ties in the index among the hits at max_dist 0.2:", ties)
    assert ties > 0


def test_search_symbols_are_declared_and_exported(lib):
    declared = engine.declared_symbols()
    for name in NEW:
        assert name in declared, f"include/mhx.h does not declare {name}"
        assert hasattr(lib, name), f"libmhx.so does not export {name}"
    assert callable(engine.dist_search) and callable(engine.dist_search_device) and callable(engine.search_files)


NO_ENGINE = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
c = ctypes
L.mhx_last_error.restype = c.c_char_p
L.mhx_dist_search.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32,
                              c.c_double, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
rows = (c.c_uint64 * 16)(*range(1, 17))
lens = (c.c_uint32 * 1)(16)
out = (c.c_uint32 * 8)()
need = c.c_size_t(0)
paths = (c.c_char_p * 1)(b"query.msh")
got = {
    "dist_search": L.mhx_dist_search(rows, lens, 1, rows, lens, 1, 16, 21, 16, 1.0, 5, out, out, out, None, out, 0),
    "dist_search_empty": L.mhx_dist_search(None, None, 0, None, None, 0, 16, 21, 16, 1.0, 5, None, None, None, None, None, 0),
    "search_files": L.mhx_search_files(b"ref.msh", paths, 1, None, None, c.c_size_t(0), c.byref(need)),
}
bad = {k: v for k, v in got.items() if v != -1}
assert not bad, bad
assert b"no GPU engine" in L.mhx_last_error()
print("ok")
"""


def test_search_entry_points_answer_no_device_without_an_engine(lib):
    # a fresh process that never calls mhx_init: no engine, whatever the machine holds
    r = subprocess.run([sys.executable, "-c", NO_ENGINE, str(engine.LIB_PATH)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
