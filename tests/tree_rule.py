"""The rule of the file-level single-linkage tree (mhx_tree_files, python -m auriclass_amd.tree) as a plain statement, on top
of the tree of tests/mst_rule.py.  Shared by the tree tests; not a test module itself.

    set         = the references of all sketch files, in argument order and then file order (triangle_rule.combine)
    merges      = the tree of mst_rule.kruskal over the oracle's pairs, in edge order; the distance of a merge is the oracle's
    table       = per merge e = 0 .. n - 2: "name_i\\tname_j\\tdist\\tp\\tcommon/denom\\tclusters\\n" -- the triangle's edge-list
                  row of the pair (names; comments under -C) and clusters = n - 1 - e, the clusters left after the merge
    newick      = the dendrogram: the height of a node is its merge distance, leaves are at 0; a branch is
                  max(0, parent height - child height), printed "%g"; of the two children of a merge the one whose lowest
                  index is lower comes first; a name is single-quoted when it holds any of ( ) [ ] ' : ; , or a blank, an
                  inner quote doubled; n = 1 prints "name;"; the output ends ";\\n"
"""
import numpy as np

from oracle import mash_oracle as mo
from tests import mst_rule as mr
from tests import triangle_rule as tr

SPECIAL = set("()[]':;,")


def quoted(name):
    if any(ch in SPECIAL or ch.isspace() for ch in name):
        return "'" + name.replace("'", "''") + "'"
    return name


def newick(names, merges, dists):
    """merges: [(i, j, ...)] in merge order, dists: their distances; names: one per leaf"""
    n = len(names)
    if n == 0:
        return ""
    # a cluster: (text, height, lowest index), found by any of its members
    cluster = {i: (quoted(names[i]), 0.0, i) for i in range(n)}
    members = {i: [i] for i in range(n)}
    for (i, j, *_), d in zip(merges, dists):
        a, b = cluster[i], cluster[j]
        assert a is not b
        if b[2] < a[2]:
            a, b = b, a
        text = "(%s:%s,%s:%s)" % (a[0], "%g" % max(0.0, d - a[1]), b[0], "%g" % max(0.0, d - b[1]))
        joined = (text, float(d), a[2])
        both = members[a[2]] + members[b[2]]
        members[a[2]] = both
        for x in both:
            cluster[x] = joined
    assert len(members[0]) == n
    return cluster[0][0] + ";\n"


def merges_of(F):
    """([(i, j, common, denom)] in merge order, their distances, their p-values) of a SketchFile"""
    n = len(F.references)
    rows = tr.pairs(F)
    common = np.array([r[2] for r in rows], np.uint32)
    denom = np.array([r[3] for r in rows], np.uint32)
    by_pair = {(r[0], r[1]): r for r in rows}
    tree = mr.kruskal(common, denom, n)
    return tree, [by_pair[(i, j)][4] for i, j, _, _ in tree], [by_pair[(i, j)][5] for i, j, _, _ in tree]


def table_text(F, comment=False):
    tree, dists, ps = merges_of(F)
    shown = [(r.comment if comment else r.name) for r in F.references]
    n = len(shown)
    return "".join("%s\t%s\t%s\t%s\t%d/%d\t%d\n" % (shown[i], shown[j], mo.fmt_g(d), mo.fmt_g(p), c, dn, n - 1 - e)
                   for e, ((i, j, c, dn), d, p) in enumerate(zip(tree, dists, ps)))


def newick_text(F, comment=False):
    tree, dists, _ = merges_of(F)
    return newick([(r.comment if comment else r.name) for r in F.references], tree, dists)
