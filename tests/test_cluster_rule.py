"""The restated rule of the clustering (tests/cluster_rule.py) against itself and against the oracle: the distance arithmetic
that the cmin table rests on, the table against the predicate value by value, the breadth-first components against a
reference union-find on every case set, the guard figures of the case sets, and the text of a hand-made file."""
import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import cluster_cases as cc
from tests import cluster_rule as cr

BOUNDS = (-0.1, 0.0, 1e-4, 0.011, 0.05, 0.3, 0.999, 1.0)


def test_distance_is_the_oracles():
    """cr.distance restates compareSketches' arithmetic: bit for bit on pairs of lists that produce the counts"""
    for k in (5, 21, 27, 32):
        for denom in (1, 2, 7, 100, 1000):
            for common in sorted({0, 1, denom // 3, denom // 2, denom - 1, denom}):
                c, d, dist = mo.compare(np.arange(denom, dtype=np.uint64), np.arange(common, dtype=np.uint64), denom, k)
                assert (c, d) == (common, denom)
                assert cr.distance(common, denom, k) == dist, (k, common, denom)
    assert mo.compare(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 1000, 21) == (0, 0, 0.0)   # two empty lists
    assert cr.distance(0, 0, 21) == 0.0


@pytest.mark.parametrize("k", [5, 21, 27, 32])
def test_cmin_table_is_the_predicate(k):
    """for every (c, d), d <= 1000: distance(c, d) <= max_dist iff c >= cmin[d] -- which also says that the distance does not
    increase with c anywhere here, the one property the integer form of the rule needs"""
    s = 1000
    rows = [cr.distance_row(d, k) for d in range(s + 1)]
    for max_dist in BOUNDS:
        cmin = cr.cmin_table(s, k, max_dist)
        for d in (0, 1, 2, 999, 1000):
            assert cmin[d] == cr.cmin_at(d, k, max_dist)   # the definition, spelt out
        for d in range(s + 1):
            passes = rows[d] <= max_dist
            assert np.array_equal(passes, np.arange(d + 1) >= cmin[d]), (k, max_dist, d)
        if max_dist < 0:
            assert np.array_equal(cmin, np.arange(s + 1) + 1)   # no edges
        else:
            assert (cmin <= np.arange(s + 1)).all() and cmin[0] == 0   # common == denom, two empty lists included: distance 0
        if max_dist >= 1:
            assert not cmin.any()   # every pair


def union_find_labels(n, edge_list):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in edge_list:
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], np.uint32)


CASES = [("set70", (), (0.0, 0.005, 0.02, 0.05, 1.0)), ("set200", (), (0.0, 0.005, 0.02, 0.05, 1.0)), ("chains", (), (0.008, cc.CHAINS_BOUND, 0.013)),
         ("crowded", (40,), (0.0, 0.02)), ("long_set", (40, 12_000), (0.01, 0.1))]


@pytest.mark.parametrize("name,args,bounds", CASES)
def test_components_equal_a_union_find(name, args, bounds):
    lists, s = getattr(cc, name)(*args)
    n = len(lists)
    for max_dist in bounds:
        e = cr.edges(lists, s, cc.K, max_dist, cc.pairs(name, cc.K, *args))
        label = cr.components(n, e)
        assert np.array_equal(label, union_find_labels(n, e))
        assert (label <= np.arange(n)).all() and (label[label] == label).all()
        assert cr.degree(n, e).sum() == 2 * len(e)


def test_the_case_sets_are_what_they_claim():
    label, degree, clusters, n_edges = cc.expected("chains", cc.CHAINS_BOUND)
    assert (clusters, n_edges) == (6, 144)
    assert sorted(np.bincount(label)[np.bincount(label) > 0].tolist()) == [1, 1, 1, 37, 50, 60]
    assert degree.max() == 2   # paths: every edge is the only link between the two halves of its chain
    lists, _ = cc.chains()
    for root in np.flatnonzero(np.bincount(label) > 1):
        slices = {int(i) // 32 for i in np.flatnonzero(label == root)}
        assert len(slices) == 5   # a chain runs through every slice of 32 lists
    assert cc.expected("set200", 0.05)[2:] == (134, 289)
    label, _, clusters, n_edges = cc.expected("set200", 0.02)
    assert (clusters, n_edges) == (142, 221)
    same = sum(int(c) * (int(c) - 1) // 2 for c in np.bincount(label))
    assert same - n_edges == 6   # pairs of one cluster that are no edges: joined through a third list only
    assert cc.expected("set70", 0.0)[2:] == (69, 1)   # the exact duplicate


def test_cluster_text_of_a_hand_made_file():
    """five references: 0 ~ 2 ~ 4 by a chain (0 and 4 are no neighbours), 1 and 3 alone; the longest member of the chain is 2"""
    base = np.arange(1, 2001, 2, dtype=np.uint64)       # 1000 hashes
    near = base.copy()
    near[:10] += 1                                          # ten of the lowest hashes differ from base
    far = near.copy()
    far[10:30] += 1                                         # twenty more: thirty differ from base
    other = np.arange(10_000, 11_000, dtype=np.uint64)
    lone = np.arange(50_000, 50_400, dtype=np.uint64)
    refs = [mo.Reference("a.fa", "first", 500, base), mo.Reference("b.fa", "second", 900, other), mo.Reference("c.fa", "third", 700, near),
            mo.Reference("d.fa", "fourth", 100, lone), mo.Reference("e.fa", "fifth", 700, far)]
    F = mo.SketchFile(21, 1000, refs)
    d01, d12, d02 = (mo.compare(x, y, 1000, 21)[2] for x, y in ((base, near), (near, far), (base, far)))
    assert d01 < d12 < d02
    bound = (d12 + d02) / 2
    assert cr.cluster_text(F, bound) == ("1\t3\ta.fa\ta.fa\t1\n1\t3\ta.fa\tc.fa\t2\n1\t3\ta.fa\te.fa\t1\n"
                                         "2\t1\tb.fa\tb.fa\t0\n3\t1\td.fa\td.fa\t0\n")
    assert cr.cluster_text(F, bound, rep="longest") == ("1\t3\tc.fa\ta.fa\t1\n1\t3\tc.fa\tc.fa\t2\n1\t3\tc.fa\te.fa\t1\n"
                                                        "2\t1\tb.fa\tb.fa\t0\n3\t1\td.fa\td.fa\t0\n")   # 700 twice: the lower index
    assert cr.cluster_text(F, bound, comment=True).startswith("1\t3\tfirst\tfirst\t1\n1\t3\tfirst\tthird\t2\n")
    assert cr.representatives(F, bound) == [0, 1, 3] and cr.representatives(F, bound, "longest") == [2, 1, 3]
    assert [r.name for r in cr.representatives_file(F, bound, "longest").references] == ["c.fa", "b.fa", "d.fa"]
    assert cr.cluster_text(F, -1.0).count("\n") == 5 and cr.representatives(F, -1.0) == [0, 1, 2, 3, 4]
    assert cr.cluster_text(F, 1.0) == "".join("1\t5\ta.fa\t%s\t4\n" % r.name for r in refs)
