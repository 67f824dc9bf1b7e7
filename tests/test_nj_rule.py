"""The rule of neighbour joining (tests/nj_rule.py) checked against what neighbour joining guarantees: an additive matrix
gives back the tree that generated it, branch for branch; where every Q ties the (lo, hi) order alone decides; the smallest
sets; and the unrooted Newick text with its quoting and its trifurcation."""
import numpy as np
import pytest

from tests import nj_cases as nc
from tests import nj_rule as nr

U = 1 << 20   # a branch of length x below is 2 x U words: every leaf distance is an even integer


def caterpillar():
    """leaves 0 .. 7, inner nodes 8 .. 13 in a chain: 0 and 1 hang on 8, 2 .. 5 on 9 .. 12, 6 and 7 on 13"""
    leaf = [(0, 8, 3), (1, 8, 11), (2, 9, 5), (3, 10, 1), (4, 11, 9), (5, 12, 2), (6, 13, 7), (7, 13, 13)]
    chain = [(8, 9, 4), (9, 10, 6), (10, 11, 1), (11, 12, 8), (12, 13, 3)]
    return leaf + chain


def balanced():
    """((0,1),(2,3)) -- ((4,5),(6,7)): cherries on 8 .. 11, 8 and 9 on 12, 10 and 11 on 13, 12 -- 13"""
    leaf = [(0, 8, 2), (1, 8, 9), (2, 9, 14), (3, 9, 1), (4, 10, 6), (5, 10, 3), (6, 11, 12), (7, 11, 5)]
    inner = [(8, 12, 7), (9, 12, 2), (10, 13, 4), (11, 13, 10), (12, 13, 8)]
    return leaf + inner


def relabelled(edges, perm):
    return [(perm[u] if u < 8 else u, perm[v] if v < 8 else v, x) for u, v, x in edges]


def tree_facts(edges, n=8):
    """(full matrix of leaf distances in words, {split: branch in words}) of an unrooted tree; a split is the side without leaf 0"""
    nodes = sorted({u for e in edges for u in e[:2]})
    near = {u: [] for u in nodes}
    for u, v, x in edges:
        near[u].append((v, 2 * x * U))
        near[v].append((u, 2 * x * U))

    def walk(start, banned=None):
        seen, todo = {start: 0}, [start]
        while todo:
            u = todo.pop()
            for v, x in near[u]:
                if v not in seen and (u, v) != banned and (v, u) != banned:
                    seen[v] = seen[u] + x
                    todo.append(v)
        return seen
    M = [[walk(i)[j] for j in range(n)] for i in range(n)]
    splits = {}
    for u, v, x in edges:
        side = frozenset(w for w in walk(u, (u, v)) if w < n)
        if 0 in side:
            side = frozenset(range(n)) - side
        splits[side] = 2 * x * U
    return M, splits


def splits_of(records, n):
    """{split: branch length as a double} of the records' tree"""
    la, lb = nr.all_lengths(records)
    below = {i: frozenset([i]) for i in range(n)}
    out = {}

    def put(side, length):
        if 0 in side:
            side = frozenset(range(n)) - side
        assert side not in out
        out[side] = length
    for t, (a, b, d, _, _) in enumerate(records[:-1]):
        put(below[a], la[t])
        put(below[b], lb[t])
        below[b] = below[b] | below.pop(a)
    a, b, d = records[-1][:3]
    put(below[a], d * nr.SCALE)
    assert lb[-1] == 0.0 and la[-1] == d * nr.SCALE
    return out


@pytest.mark.parametrize("edges", [caterpillar(), balanced(), relabelled(caterpillar(), [5, 2, 7, 0, 3, 6, 1, 4]), relabelled(balanced(), [6, 3, 0, 5, 7, 1, 4, 2])],
                         ids=["caterpillar", "balanced", "caterpillar relabelled", "balanced relabelled"])
def test_an_additive_matrix_gives_back_its_tree(edges):
    """the classical guarantee: every split of the generating tree with its exact branch length, and the clamp never acts"""
    M, want = tree_facts(edges)
    assert all(M[i][j] % 2 == 0 and M[i][j] == M[j][i] and M[i][j] <= nr.ONE for i in range(8) for j in range(8))
    records, clamps = nr.join(nr.matrix_words(M))
    assert clamps == 0 and len(records) == 7
    got = splits_of(records, 8)
    assert len(want) == 13 and set(got) == set(want)
    for side, words in want.items():
        assert got[side] == words * nr.SCALE, (sorted(side), got[side], words * nr.SCALE)
    # every r is the row sum of the matrix while the nodes are leaves
    a, b, d, r_a, r_b = records[0]
    assert (d, r_a, r_b) == (M[a][b], sum(M[a]), sum(M[b]))


@pytest.mark.parametrize("name", ["identical", "disjoint"])
def test_where_every_q_ties_the_ids_decide(name):
    """all lists equal (every d = 0) or all disjoint (every d = 2^32): every comparison of every join ties, and node 0 takes the
    lowest other node, join after join"""
    lists, _ = nc.lists_of(name, (70,))
    common, denom, _ = nc.pairs(name, (70,))
    n = len(lists)
    count = {}
    records, clamps = nr.records_of(common, denom, n, nc.K, count)
    assert [(a, b) for a, b, *_ in records] == [(t + 1, 0) for t in range(n - 1)]
    assert count["ties"] == sum(m * (m - 1) // 2 - 1 for m in range(3, n + 1))
    assert clamps == 0
    if name == "identical":
        assert all(rec[2:] == (0, 0, 0) for rec in records)
    else:
        assert records[0] == (1, 0, nr.ONE, (n - 1) * nr.ONE, (n - 1) * nr.ONE)


def test_the_smallest_sets():
    assert nr.join([]) == ([], 0)
    assert nr.join([[]]) == ([], 0)
    assert nr.join([[], [12345]]) == ([(1, 0, 12345, 0, 0)], 0)
    assert nr.lengths(12345, 2, 0, 0) == (12345 * nr.SCALE, 0.0)
    # a star of three leaves with branches 2, 4, 6: all three Q tie, (0, 1) joins, the new node is 6 from leaf 2
    records, clamps = nr.join([[], [6 * U], [8 * U, 10 * U]])
    assert records == [(1, 0, 6 * U, 16 * U, 14 * U), (2, 0, 6 * U, 0, 0)] and clamps == 0
    la, lb = nr.all_lengths(records)
    assert la.tolist() == [4 * U * nr.SCALE, 6 * U * nr.SCALE] and lb.tolist() == [2 * U * nr.SCALE, 0.0]
    # the floor and the clamp: (1 + 2 - 8) >> 1 = -3 -> 0, (5 + 2 - 4) >> 1 = 1
    assert nr.join_word(1, 2, 8) == (0, True) and nr.join_word(5, 2, 4) == (1, False) and nr.join_word(3, 1, 4) == (0, False)
    assert nr.join_word(3, 0, 4) == (0, True)   # -1 >> 1 = -1: a floor, not a truncation
    assert nr.newick([], []) == "" and nr.newick(["a b"], []) == "'a b';\n"
    assert nr.newick(["x", "y"], [(1, 0, 1 << 31, 0, 0)]) == "(x:0,y:0.5);\n"


def test_newick_quoting_and_the_trifurcation():
    """((0:2,1:4):6,2:8,3:10) in units of 2^-5: (0, 1) joins first (it ties with (2, 3): the lower lo), then all three Q tie and
    (0, 2) joins; the root holds the two children of that join and leaf 3 with the distance of the last record"""
    W = 1 << 27
    d = {(1, 0): 6, (2, 0): 16, (3, 0): 18, (2, 1): 18, (3, 1): 20, (3, 2): 18}
    D = [[d[(i, j)] * W for j in range(i)] for i in range(4)]
    records, clamps = nr.join([row[:] for row in D])
    assert clamps == 0
    assert records == [(1, 0, 6 * W, 44 * W, 40 * W), (2, 0, 14 * W, 32 * W, 30 * W), (3, 0, 10 * W, 0, 0)]
    assert nr.newick(["n0", "n1", "n2", "n3"], records) == "((n0:0.0625,n1:0.125):0.1875,n2:0.25,n3:0.3125);\n"
    assert nr.newick(["n0", "it's (a) name", "a,b:c;[d]", "n3"], records) == "((n0:0.0625,'it''s (a) name':0.125):0.1875,'a,b:c;[d]':0.25,n3:0.3125);\n"
    # three leaves: the trifurcation alone, children by their lowest leaf
    records, _ = nr.join([[], [6 * W], [8 * W, 10 * W]])
    assert nr.newick(["n0", "n1", "n2"], records) == "(n0:0.0625,n1:0.125,n2:0.1875);\n"
    # a negative length prints as 0 in the tree: leaf 1 lies "behind" leaf 0 as seen from leaf 2
    records, _ = nr.join([[], [2 * W], [10 * W, 4 * W]])
    la, lb = nr.all_lengths(records)
    assert min(la.min(), lb.min()) < 0
    text = nr.newick(["n0", "n1", "n2"], records)
    assert ":0," in text and "-" not in text


def test_the_case_sets_cover_clamps_negative_lengths_and_ties():
    """what the sets exercise, by the rule: a clamped update in tiny(33), tiny(65) and short, negative branch lengths in tiny and
    chains, hundreds of thousands of tied comparisons in set200"""
    for name, args, clamps, negative in (("tiny", (33,), 1, 8), ("tiny", (65,), 1, 17), ("short", (), 1, None), ("chains", (), 0, 20)):
        records, got, la, lb = nc.expected(name, args)
        assert got == clamps, (name, args, got)
        if negative is not None:
            assert int((la < 0).sum() + (lb < 0).sum()) == negative, (name, args)
    lists, _ = nc.lists_of("set200")
    common, denom, _ = nc.pairs("set200")
    count = {}
    nr.records_of(common, denom, len(lists), nc.K, count)
    print("set200: tied comparisons", count["ties"])
    assert count["ties"] > 100_000
    # Q stays far inside 64 bits: |Q| < 2^50 at the limits of the call
    assert abs(nr.q_value(65536, nr.ONE, 0, 0)) < 1 << 50 and abs(nr.q_value(65536, 0, 65535 * nr.ONE, 65535 * nr.ONE)) < 1 << 50
