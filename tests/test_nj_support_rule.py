"""The rule of the jackknife support (tests/nj_support_rule.py) on hand-made trees, the host-only count of the library
(mhx_nj_split_support) against it on the replicate trees of two case sets, and the rule's table and Newick text."""
import re

import numpy as np
import pytest

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import nj_cases as nc
from tests import nj_rule as nr
from tests import nj_support_rule as ns

NEW = ("mhx_resample_rows", "mhx_dist_nj_support", "mhx_nj_split_support", "mhx_nj_files_opts")
R, KEEP, SEED = 4, 0.5, 42

# six leaves: ((0,1),(2,3),(4,5)) -- join 3 = n - 3 closes {0,1,2,3}, the complement of the third child {4,5} of join 2
MAIN6 = [(1, 0), (3, 2), (5, 4), (2, 0), (4, 0)]
REPS6 = [
    MAIN6,                                              # the same tree: every split
    [(2, 1), (3, 0), (5, 4), (1, 0), (4, 0)],           # {1,2}, {0,3} -> {1,2,4,5}, {4,5}, {0,1,2,3} -> {4,5}
    [(1, 0), (4, 3), (5, 2), (3, 0), (2, 0)],           # {0,1} -> {2,3,4,5}, {3,4}, {2,5}, {0,1,3,4} -> {2,5}
]


def test_split_rule_on_a_hand_made_tree():
    n = 6
    sets = ns.leaf_sets(MAIN6, n)
    assert [sorted(x) for x in sets] == [[0, 1], [2, 3], [4, 5], [0, 1, 2, 3], [0, 1, 2, 3, 4, 5]]
    # through leaf 0: a set that holds it is replaced by its complement
    assert [sorted(ns.canon(x, n)) for x in sets] == [[2, 3, 4, 5], [2, 3], [4, 5], [4, 5], []]
    assert [ns.trivial(x, n) for x in sets] == [False, False, False, False, True]
    assert ns.splits(REPS6[1], n) == {frozenset([1, 2]), frozenset([1, 2, 4, 5]), frozenset([4, 5]), frozenset()}
    assert ns.splits(REPS6[2], n) == {frozenset([2, 3, 4, 5]), frozenset([3, 4]), frozenset([2, 5]), frozenset()}
    sup = ns.support(MAIN6, REPS6, n)
    assert sup == [2, 1, 2, 2, 3]
    assert sup[n - 3] == sup[2]          # join n - 3 and the third child, the node of join 2: one split, one count
    assert ns.support(MAIN6, [], n) == [0, 0, 0, 0, 0]
    # a caterpillar of four leaves: {0,1,2} has n - 1 leaves, {0,1,2,3} n -- in every tree whatever the replicates say
    main4 = [(1, 0), (2, 0), (3, 0)]
    reps4 = [[(3, 2), (1, 0), (2, 0)], [(2, 1), (3, 0), (1, 0)]]
    assert ns.support(main4, reps4, 4) == [1, 2, 2]
    assert ns.support([(1, 0)], reps=[[(1, 0)]] * 5, n=2) == [5]


def test_library_symbols_are_declared_and_exported():
    lib = engine.load()
    declared = engine.declared_symbols()
    for name in NEW:
        assert name in declared, f"include/mhx.h does not declare {name}"
        assert hasattr(lib, name), f"libmhx.so does not export {name}"
    for fn in ("resample_rows", "dist_nj_support", "dist_nj_support_device", "nj_split_support", "nj_files"):
        assert callable(getattr(engine, fn))
    assert engine.ctypes.sizeof(engine.NjOpts) == 32


def test_host_count_on_the_hand_made_trees():
    got = engine.nj_split_support([a for a, _ in MAIN6], [b for _, b in MAIN6], [[a for a, _ in t] for t in REPS6], [[b for _, b in t] for t in REPS6], 6)
    assert got.tolist() == [2, 1, 2, 2, 3]
    assert engine.nj_split_support([1], [0], [[1]] * 5, [[0]] * 5, 2).tolist() == [5]
    assert engine.nj_split_support([], [], [], [], 1).size == 0
    lib = engine.load()
    # joins that are no tree: an id that is gone, b >= a, an id outside
    for bad in ([(1, 0), (1, 0), (5, 4), (2, 0), (4, 0)], [(0, 1), (3, 2), (5, 4), (2, 0), (4, 0)], [(6, 0), (3, 2), (5, 4), (2, 0), (4, 0)]):
        with pytest.raises(engine.EngineError) as exc:
            engine.nj_split_support([a for a, _ in bad], [b for _, b in bad], np.zeros((0, 5)), np.zeros((0, 5)), 6)
        assert exc.value.code == engine.MHX_E_ARG and "no tree" in exc.value.message
        with pytest.raises(engine.EngineError) as exc:
            engine.nj_split_support([a for a, _ in MAIN6], [b for _, b in MAIN6], [[a for a, _ in bad]], [[b for _, b in bad]], 6)
        assert exc.value.code == engine.MHX_E_ARG and "replicate 0" in exc.value.message
    v = engine.ctypes.c_void_p
    assert lib.mhx_nj_split_support(v(None), v(None), v(None), v(None), engine.ctypes.c_uint32(6), engine.ctypes.c_uint32(0), v(None)) == engine.MHX_E_ARG


@pytest.mark.parametrize("name,args", [("set70", ()), ("tiny", (33,))])
def test_host_count_equals_the_rule_on_replicate_trees(name, args):
    """host only, like mst_labels: the replicate trees come from the rule"""
    n = len(nc.lists_of(name, args)[0])
    want, rep_a, rep_b, _ = ns.expected(name, args, R, KEEP, SEED)
    main = nc.expected(name, args)[0]
    got = engine.nj_split_support([r[0] for r in main], [r[1] for r in main], rep_a, rep_b, n)
    assert got.tolist() == want.tolist()
    assert got[-1] == R and got.max() <= R
    if name == "set70":   # otherwise the count could not be told from a constant
        assert any(0 < c < R for c in want.tolist()), want.tolist()
    # a tree against itself: every split, every time
    same = engine.nj_split_support([r[0] for r in main], [r[1] for r in main], [[r[0] for r in main]] * 3, [[r[1] for r in main]] * 3, n)
    assert (same == 3).all()


def small_file():
    """nine references off one base, so that the tree has inner nodes worth a label; names that need quoting among them"""
    rng = np.random.default_rng(83)
    from tests import triangle_cases as tc
    base = tc.sketch_like(rng, 400)[:300]
    lists = [base] + [tc.mutate(rng, base, 0.05 * (i + 1))[:300] for i in range(8)]
    names = ["ref%d.fa" % i for i in range(9)]
    names[2] = "it's (a) name.fa"
    return mo.SketchFile(nc.K, 300, [mo.Reference(names[i], "genome %d" % i, 1_000_000 + i, h) for i, h in enumerate(lists)])


def test_table_and_newick_text_of_the_rule():
    F = small_file()
    n = len(F.references)
    records, sup = ns.file_support(F, 5, 0.5, 42)
    assert len(sup) == n - 1 and sup[-1] == 5 and all(0 <= c <= 5 for c in sup)
    table = ns.table_text(F, 5, 0.5, 42)
    rows = [r.split("\t") for r in table.splitlines()]
    assert len(rows) == n - 1 and all(len(r) == 7 for r in rows)
    assert [r[6] for r in rows] == ["%d/5" % c for c in sup]
    assert "".join("\t".join(r[:6]) + "\n" for r in rows) == nr.table_text(F)
    assert ns.table_text(F, 5, 0.5, 42, comment=True).startswith("genome ")
    text = ns.newick_text(F, 5, 0.5, 42)
    labels = re.findall(r"\)(\d+):", text)
    assert len(labels) == n - 3 and sorted(map(int, labels)) == sorted(100 * c // 5 for c in sup[:n - 3])
    assert re.sub(r"\)\d+:", "):", text) == nr.newick_text(F) and text.endswith(");\n")   # the trifurcation carries no label
    # the label is floored: 2 of 3 replicates print 66
    assert ns.newick(["a", "b", "c", "d"], [(1, 0, 5, 0, 0), (3, 2, 5, 0, 0), (2, 0, 5, 0, 0)], [2, 2, 3], 3).count(")66:") == 1
    # up to three leaves there is no inner node but the root
    G = mo.SketchFile(F.kmer_size, F.sketch_size, F.references[:3])
    assert ns.newick_text(G, 5, 0.5, 42) == nr.newick_text(G)
