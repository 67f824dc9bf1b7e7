"""The rule of the single-linkage tree (tests/mst_rule.py) on the CPU: the libm distance does not increase along the exact
edge order (what makes a cut of the tree the clustering), Kruskal against a brute-force Prim, the cut against the clustering's
rule at every distance that occurs, the library's own cut (engine.mst_labels) against the rule's, and the exports."""
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from auriclass_amd import engine
from tests import cluster_cases as cc
from tests import cluster_rule as cr
from tests import mst_cases as mc
from tests import mst_rule as mr
from tests import tree_rule as tl

NEW = ["mhx_dist_mst", "mhx_last_mst_rounds", "mhx_last_mst_stored", "mhx_mst_labels", "mhx_tree_files"]


@pytest.fixture(scope="module")
def lib():
    return engine.load()


@pytest.mark.parametrize("k", [5, 21, 27, 32])
def test_distance_does_not_increase_with_the_exact_index(k):
    """every c / d with d <= 400, c == d as 1/1 (0/0 included), sorted by exact value: the distances do not increase, and
    equal fractions (1/2, 2/4) give equal distances"""
    by_value = {}
    for d in range(401):
        for c in range(d + 1):
            by_value.setdefault(Fraction(*mr.index_key(c, d)), set()).add(cr.distance(c, d, k))
    assert len(by_value) == 48_679
    assert all(len(v) == 1 for v in by_value.values())   # one double per exact value
    assert cr.distance(1, 2, k) == cr.distance(2, 4, k) == cr.distance(200, 400, k)
    dist = np.array([next(iter(by_value[f])) for f in sorted(by_value)])
    assert (np.diff(dist) <= 0).all()
    assert dist[0] == 1.0 and dist[-1] == 0.0


def test_order_is_search_betters_with_lo_hi_ties():
    e = lambda i, j, c, d: (i, j, c, d)   # noqa: E731
    assert mr.precedes(e(5, 4, 3, 4), e(1, 0, 2, 3))          # 3/4 > 2/3
    assert mr.precedes(e(9, 8, 0, 0), e(1, 0, 999, 1000))     # 0/0 counts as 1/1
    assert mr.precedes(e(3, 1, 1, 2), e(3, 2, 2, 4)) and not mr.precedes(e(3, 2, 2, 4), e(3, 1, 1, 2))   # equal index: lower lo
    assert mr.precedes(e(3, 1, 2, 4), e(4, 1, 1, 2))          # equal index and lo: lower hi
    assert mr.precedes(e(2, 0, 5, 5), e(1, 0, 0, 0)) is False  # 1/1 both: (0, 1) before (0, 2)
    big = (1 << 20) - 1
    assert mr.precedes(e(1, 0, big, big), e(2, 0, big - 1, big))
    assert mr.precedes(e(1, 0, big - 1, big), e(2, 0, big - 2, big - 1))   # cross products of 2^40: exact in integers


def test_kruskal_equals_brute_force_prim_on_set70():
    lists, _ = mc.set70()
    common, denom, _ = mc.pairs("set70")
    tree = mc.expected("set70")
    assert len(tree) == 69 and all(i > j for i, j, _, _ in tree)
    assert tree == mr.prim(common, denom, len(lists))
    d = mr.distances(tree, mc.K)
    assert (np.diff(d) >= 0).all()   # merge order: the distance does not decrease


@pytest.mark.parametrize("name,args", [("identical", (70,)), ("disjoint", (70,)), ("duplicate_pairs", (64,))])
def test_trees_of_the_degenerate_sets(name, args):
    tree = mc.expected(name, args)
    n = len(mc.lists_of(name, args)[0])
    if name == "identical":
        assert tree == [(i, 0, 1000, 1000) for i in range(1, n)]   # the star at list 0
    if name == "disjoint":
        assert tree == [(i, 0, 0, c[3]) for i, c in zip(range(1, n), tree)]   # every index 0: (lo, hi) alone
    if name == "duplicate_pairs":
        assert tree[:n // 2] == [(i + n // 2, i, 1000, 1000) for i in range(n // 2)]


def test_cut_equals_the_clustering_at_every_distance_of_set70():
    """mst_labels of the rule's tree against cluster_rule.cluster at each distinct distance of set70 and at the double just
    below it; engine.mst_labels, the host function users call, gives the same"""
    lists, s = mc.set70()
    pairs = mc.pairs("set70")
    tree = mc.expected("set70")
    n = len(lists)
    ei, ej, ec, ed = (np.array(col, np.uint32) for col in zip(*tree))
    distinct = np.unique(pairs[2])
    assert distinct.size == 48
    for T in distinct.tolist():
        for bound in (T, float(np.nextafter(T, -np.inf))):
            want_label, _, want_clusters, _ = cr.cluster(lists, s, mc.K, bound, pairs)
            label, clusters = mr.mst_labels(tree, n, mc.K, bound)
            assert clusters == want_clusters and np.array_equal(label, want_label), (T, bound)
            label, clusters = engine.mst_labels(ei, ej, ec, ed, n, mc.K, bound)
            assert clusters == want_clusters and np.array_equal(label, want_label), (T, bound)


@pytest.mark.parametrize("bound", [-0.1, 0.0, 0.005, 0.02, 0.05, 1.0])
def test_cut_equals_the_clustering_on_set200(bound):
    lists, _ = mc.set200()
    tree = mc.expected("set200")
    want_label, _, want_clusters, _ = cc.expected("set200", bound)
    label, clusters = mr.mst_labels(tree, len(lists), mc.K, bound)
    assert clusters == want_clusters and np.array_equal(label, want_label)


def test_newick_rule_on_hand_written_cases():
    assert tl.newick([], [], []) == ""
    assert tl.newick(["a"], [], []) == "a;\n"
    assert tl.newick(["a b"], [], []) == "'a b';\n"
    assert tl.newick(["a", "b"], [(1, 0)], [0.25]) == "(a:0.25,b:0.25);\n"
    # the child with the lower lowest index first, whichever end of the merge names it
    assert tl.newick(["a", "b", "c"], [(2, 1), (2, 0)], [0.01, 0.5]) == "(a:0.5,(b:0.01,c:0.01):0.49);\n"
    assert tl.newick(["a", "b", "c"], [(1, 0), (2, 1)], [0.125, 0.25]) == "((a:0.125,b:0.125):0.125,c:0.25);\n"
    # ties: merges at one distance nest with branches of length 0, duplicates sit at height 0
    assert tl.newick(["a", "b", "c"], [(1, 0), (2, 0)], [0.0, 0.0]) == "((a:0,b:0):0,c:0);\n"
    assert tl.newick(["a", "b", "c", "d"], [(1, 0), (3, 2), (2, 0)], [0.1, 0.1, 0.1]) == "((a:0.1,b:0.1):0,(c:0.1,d:0.1):0);\n"
    # a height that falls (it cannot along the edge order, but the floor is part of the rule) gives a branch of 0
    assert tl.newick(["a", "b", "c"], [(1, 0), (2, 0)], [0.5, 0.25]) == "((a:0.5,b:0.5):0,c:0.25);\n"
    # quoting: any of ( ) [ ] ' : ; , or a blank; an inner quote doubled; other characters stay
    for name, want in (("x(y", "'x(y'"), ("x)y", "'x)y'"), ("x[y", "'x[y'"), ("x]y", "'x]y'"), ("x:y", "'x:y'"), ("x;y", "'x;y'"), ("x,y", "'x,y'"),
                       ("x y", "'x y'"), ("x\ty", "'x\ty'"), ("it's", "'it''s'"), ("x/y_z.fa|1", "x/y_z.fa|1"), ("", "")):
        assert tl.quoted(name) == want
    assert tl.newick(["it's", "b c"], [(1, 0)], [1.0]) == "('it''s':1,'b c':1);\n"
    assert tl.newick(["a", "b"], [(1, 0)], [1.23456789e-05]) == "(a:1.23457e-05,b:1.23457e-05);\n"   # %g


def test_mst_symbols_are_declared_and_exported(lib):
    declared = engine.declared_symbols()
    for name in NEW:
        assert name in declared, f"include/mhx.h does not declare {name}"
        assert hasattr(lib, name), f"libmhx.so does not export {name}"
    assert callable(engine.dist_mst) and callable(engine.dist_mst_device) and callable(engine.mst_labels) and callable(engine.tree_files)


NO_ENGINE = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
c = ctypes
L.mhx_last_error.restype = c.c_char_p
L.mhx_dist_mst.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                           c.c_void_p, c.c_int]
rows = (c.c_uint64 * 32)(*range(1, 33))
lens = (c.c_uint32 * 2)(16, 16)
out = (c.c_uint32 * 8)()
need = c.c_size_t(0)
paths = (c.c_char_p * 1)(b"set.msh")
got = {
    "tree_files": L.mhx_tree_files(paths, 1, None, None, c.c_size_t(0), c.byref(need)),
    "dist_mst": L.mhx_dist_mst(rows, lens, 2, 16, 21, 16, out, out, out, out, None, 0),
    "dist_mst_empty": L.mhx_dist_mst(None, None, 0, 16, 21, 16, None, None, None, None, None, 0),
}
bad = {k: v for k, v in got.items() if v != -1}
assert not bad, bad
assert b"no GPU engine" in L.mhx_last_error()
assert L.mhx_last_mst_rounds() == 0 and L.mhx_last_mst_stored() == -1
# the cut is host arithmetic: it answers without an engine
L.mhx_mst_labels.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32, c.c_int, c.c_double, c.c_void_p, c.POINTER(c.c_uint32)]
ei, ej, ec, ed = (c.c_uint32 * 2)(1, 2), (c.c_uint32 * 2)(0, 1), (c.c_uint32 * 2)(5, 1), (c.c_uint32 * 2)(5, 2)
label, clusters = (c.c_uint32 * 3)(9, 9, 9), c.c_uint32(9)
assert L.mhx_mst_labels(ei, ej, ec, ed, 3, 21, 0.0, label, c.byref(clusters)) == 0 and list(label) == [0, 0, 2] and clusters.value == 2
assert L.mhx_mst_labels(ei, ej, ec, ed, 3, 21, 1.0, label, c.byref(clusters)) == 0 and list(label) == [0, 0, 0] and clusters.value == 1
assert L.mhx_mst_labels(None, None, None, None, 0, 21, 1.0, None, c.byref(clusters)) == 0 and clusters.value == 0
for bad in ((ei, ej, ec, ed, 3, 0, 0.5, label, c.byref(clusters)), (ei, ej, ec, ed, 3, 21, float("nan"), label, c.byref(clusters)),
            (ei, ej, ec, ed, 3, 21, 0.5, None, c.byref(clusters)), (None, ej, ec, ed, 3, 21, 0.5, label, c.byref(clusters)),
            ((c.c_uint32 * 2)(1, 3), ej, ec, ed, 3, 21, 0.5, label, c.byref(clusters)), (ei, ej, ec, ed, 3, 21, 0.5, label, None)):
    assert L.mhx_mst_labels(*bad) == -2, bad[4:7]
print("ok")
"""


def test_mst_entry_point_answers_no_device_without_an_engine(lib):
    # a fresh process that never calls mhx_init: no engine, whatever the machine holds
    r = subprocess.run([sys.executable, "-c", NO_ENGINE, str(engine.LIB_PATH)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
