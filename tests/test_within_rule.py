"""CPU-side checks of the bounded neighbourhood call: the restated rule (tests/within_rule.py) against a brute-force filter of
the oracle matrix, the exact integer form of the bound (cluster_keep over cluster_cmin_build, through the emulator's small
entry) against the rule for every (common, denom) of the case set, a bound that IS the distance of an occurring pair, the
agreement with the search's rule where no list is truncated, the conditions the case set (tests/within_cases.py) must satisfy,
and the new entry points: declared, exported, and refusing to compute without a GPU engine."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

from auriclass_amd import engine
from tests import emul_build
from tests import search_cases as sc
from tests import search_rule
from tests import within_cases as wc
from tests import within_rule as rule

NEW = ["mhx_dist_within", "mhx_within_files"]


@pytest.fixture(scope="module")
def lib():
    engine.build()
    return engine.load()


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("within_emul")
    L.emul_within_keep.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    L.emul_within_keep.restype = None
    L.emul_within_cmin.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    L.emul_within_cmin.restype = None
    return L


def test_case_set_conditions():
    common, denom, dist = wc.matrix()
    assert common.shape == (70, 330) and wc.NQ % 4 != 0 and (wc.NR + 31) // 32 == 11 and wc.NR % 32 == 10
    for d in (0.02, 0.05):
        h = wc.hits_per_query(d)
        print("max_dist", d, "hits of queries 0 and 1:", int(h[0]), int(h[1]))
        assert h[0] > 64 and h[1] > 64            # beyond a search list, at bounds that are real thresholds:
    assert wc.hits_per_query(0.02)[0] < wc.hits_per_query(0.05)[0] < wc.NR   # 0.02 cuts the crowd in two, 0.05 still leaves references out
    assert not wc.hits_per_query(float(np.nextafter(1.0, 0.0)))[4:].any()
    assert wc.hits_per_query(0.0)[:4].tolist() == [3, 0, 1, 1]
    assert (wc.hits_per_query(1.0) == wc.NR).all() and not wc.hits_per_query(-1.0).any()
    crowd = np.flatnonzero(dist[0] <= 0.05)
    assert len(set(crowd // 32)) >= 10            # spread over ten slices
    want = wc.expected(0.0)
    assert want[1][:3].tolist() == [305, 307, 329] and want[1][3:].tolist() == [301, 303]
    assert (want[2][3], want[3][3], want[4][3]) == (0, 0, 0.0)   # 0/0 against the empty reference: distance 0


def test_rule_equals_a_brute_force_filter():
    common, denom, dist = wc.matrix()
    for max_dist in wc.bounds():
        row_off, ref, c, d, x = wc.expected(max_dist)
        keep = dist <= max_dist
        assert np.array_equal(np.diff(row_off.astype(np.int64)), keep.sum(axis=1))
        qi, ri = np.nonzero(keep)                  # row-major: by query, then ascending by reference
        assert np.array_equal(ref, ri.astype(np.uint32)) and np.array_equal(c, common[qi, ri]) and np.array_equal(d, denom[qi, ri])
        assert np.array_equal(x.view(np.uint64), dist[qi, ri].view(np.uint64))
        for q in (0, 1, 2, 69):
            assert np.all(np.diff(ref[int(row_off[q]):int(row_off[q + 1])].astype(np.int64)) > 0)


def test_the_integer_bound_equals_the_rule(emul):
    """cluster_keep over cluster_cmin_build -- what the kernels evaluate -- for every (common, denom) of the case set at each
    bound, a bound that is exactly the distance of an occurring pair (a hit) and the next double towards 0 (not a hit) included"""
    common, denom, dist = wc.matrix()
    c, d = np.ascontiguousarray(common.ravel()), np.ascontiguousarray(denom.ravel())
    x = wc.exact_bound()
    assert x in wc.bounds() and float(np.nextafter(x, 0.0)) in wc.bounds() and (dist == x).any()
    for max_dist in wc.bounds() + [0.3, float(np.nextafter(0.0, 1.0)), 5.0]:
        keep = np.zeros(c.size, np.uint8)
        emul.emul_within_keep(c.ctypes.data, d.ctypes.data, c.size, wc.S, wc.K, max_dist, keep.ctypes.data)
        assert np.array_equal(keep.astype(bool), dist.ravel() <= max_dist), max_dist
    at = np.zeros(c.size, np.uint8)
    below = np.zeros(c.size, np.uint8)
    emul.emul_within_keep(c.ctypes.data, d.ctypes.data, c.size, wc.S, wc.K, x, at.ctypes.data)
    emul.emul_within_keep(c.ctypes.data, d.ctypes.data, c.size, wc.S, wc.K, float(np.nextafter(x, 0.0)), below.ctypes.data)
    on = dist.ravel() == x
    assert at[on].all() and not below[on].any() and np.array_equal(at[~on], below[~on])
    cmin = np.zeros(wc.S + 1, np.uint32)
    emul.emul_within_cmin(wc.S, wc.K, 1.0, cmin.ctypes.data)
    assert not cmin.any()                                       # max_dist >= 1 keeps every pair
    emul.emul_within_cmin(wc.S, wc.K, -1e-300, cmin.ctypes.data)
    assert np.array_equal(cmin, np.arange(1, wc.S + 2))         # max_dist < 0 keeps none, 0/0 included
    emul.emul_within_cmin(wc.S, wc.K, 0.0, cmin.ctypes.data)
    assert np.array_equal(cmin, np.arange(wc.S + 1))            # 0: common == denom, 0/0 included


def test_order_one_equals_the_search_where_no_list_is_truncated():
    """tests/search_cases.py: no query has more than 11 hits below 1, so top = 64 cuts nothing off"""
    common, denom, dist = sc.matrix()
    for max_dist in (0.0, 0.02, 0.05, 0.2):
        assert sc.hits_per_query(max_dist).max() <= 11 if max_dist <= 0.05 else sc.hits_per_query(max_dist).max() <= 64
        row_off, ref, c, d, x = rule.csr_from_matrix(common, denom, dist, max_dist)
        for q in range(sc.NQ):
            lo, hi = int(row_off[q]), int(row_off[q + 1])
            mine = search_rule.ranked([(int(ref[t]), int(c[t]), int(d[t]), float(x[t])) for t in range(lo, hi)])
            pairs = [(r, int(common[q, r]), int(denom[q, r]), float(dist[q, r])) for r in range(common.shape[1])]
            assert mine == search_rule.select(pairs, 64, max_dist)


def test_within_symbols_are_declared_and_exported(lib):
    declared = engine.declared_symbols()
    for name in NEW:
        assert name in declared, f"include/mhx.h does not declare {name}"
        assert hasattr(lib, name), f"libmhx.so does not export {name}"
    assert all(callable(f) for f in (engine.dist_within, engine.dist_within_counts, engine.dist_within_device, engine.within_files))
    assert ctypes.sizeof(engine.WithinOpts) == 24


NO_ENGINE = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
c = ctypes
L.mhx_last_error.restype = c.c_char_p
L.mhx_dist_within.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32,
                              c.c_double, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_int]
rows = (c.c_uint64 * 16)(*range(1, 17))
lens = (c.c_uint32 * 1)(16)
out = (c.c_uint32 * 8)()
off = (c.c_uint64 * 2)()
n = c.c_uint64(0)
need = c.c_size_t(0)
paths = (c.c_char_p * 1)(b"query.msh")
got = {
    "dist_within": L.mhx_dist_within(rows, lens, 1, rows, lens, 1, 16, 21, 16, 1.0, off, out, out, out, None, 8, c.byref(n), 0),
    "dist_within_empty": L.mhx_dist_within(None, None, 0, None, None, 0, 16, 21, 16, 1.0, None, None, None, None, None, 0, None, 0),
    "within_files": L.mhx_within_files(b"ref.msh", paths, 1, None, None, c.c_size_t(0), c.byref(need)),
}
bad = {k: v for k, v in got.items() if v != -1}
assert not bad, bad
assert b"no GPU engine" in L.mhx_last_error()
print("ok")
"""


def test_within_entry_points_answer_no_device_without_an_engine(lib):
    # a fresh process that never calls mhx_init: no engine, whatever the machine holds
    r = subprocess.run([sys.executable, "-c", NO_ENGINE, str(engine.LIB_PATH)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
