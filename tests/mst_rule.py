"""The rule of the single-linkage tree (mhx_dist_mst) as a plain statement over a set of sketches, built from the piece of the
CPU oracle that mash's own output pins for `mash dist`: compare (compareSketches).  Shared by the tree tests; not a test
module itself.

    pair(i, j)  = compare(list i, list j) for j < i: common, denom.  Every pair is an edge: the tree spans the set and no
                  distance bound applies.
    edge order  = edge a precedes edge b iff its Jaccard index common / denom is greater, compared exactly (Python integers:
                  a.common * b.denom > b.common * a.denom); common == denom counts as 1/1, 0/0 included; equal indices go by
                  the lower lo = min(i, j), then by the lower hi.  Total and strict.
    tree        = Kruskal over the edges in this order (deliberately not Boruvka, which is what the library runs): the n - 1
                  edges (i, j, common, denom), i > j, in edge order -- the merge order of the dendrogram.  The distance of
                  an edge is the oracle's double (cluster_rule.distance: host libm).
    cut         = mst_labels(edges, n, k, max_dist): a union-find over the tree edges with distance <= max_dist, label[i] =
                  the lowest index of i's component.  Equal to the clustering's labels at max_dist wherever the distance
                  does not increase along the edge order (tests/test_mst_rule.py checks that fraction by fraction).
"""
import functools

import numpy as np

from tests import cluster_rule as cr


def index_key(common, denom):
    """(numerator, denominator) of the Jaccard index with common == denom as 1/1"""
    return (1, 1) if common == denom else (int(common), int(denom))


def precedes(a, b):
    """a, b: (i, j, common, denom) with i > j"""
    (an, ad), (bn, bd) = index_key(a[2], a[3]), index_key(b[2], b[3])
    if an * bd != bn * ad:
        return an * bd > bn * ad
    return (a[1], a[0]) < (b[1], b[0])   # (lo, hi)


def _cmp(a, b):
    return -1 if precedes(a, b) else (1 if precedes(b, a) else 0)


def sort_edges(edge_list):
    return sorted(edge_list, key=functools.cmp_to_key(_cmp))


def all_edges(common, denom, n):
    """(i, j, common, denom) of every pair j < i from the packed triangle (tc.oracle_pairs)"""
    ii, jj = cr.packed_indices(n)
    return list(zip(ii.tolist(), jj.tolist(), np.asarray(common).tolist(), np.asarray(denom).tolist()))


def kruskal(common, denom, n):
    """the tree: [(i, j, common, denom)] in edge order"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    tree = []
    for e in sort_edges(all_edges(common, denom, n)):
        a, b = find(e[0]), find(e[1])
        if a != b:
            parent[a] = b
            tree.append(e)
    assert len(tree) == max(n - 1, 0)
    return tree


def prim(common, denom, n):
    """the same tree by brute force from vertex 0: each step the first edge, in edge order, that leaves the grown part"""
    at = lambda i, j: i * (i - 1) // 2 + j   # noqa: E731
    inside = {0}
    tree = []
    while len(inside) < n:
        best = None
        for u in inside:
            for v in range(n):
                if v in inside:
                    continue
                i, j = max(u, v), min(u, v)
                e = (i, j, int(common[at(i, j)]), int(denom[at(i, j)]))
                if best is None or precedes(e, best):
                    best = e
        tree.append(best)
        inside.add(best[0])
        inside.add(best[1])
    return sort_edges(tree)


def distances(tree, k):
    return np.array([cr.distance(c, d, k) for _, _, c, d in tree], np.float64)


def mst_labels(tree, n, k, max_dist):
    """(label, n_clusters) of the cut at max_dist: connected components (breadth-first search) of the kept tree edges"""
    kept = [(i, j) for i, j, c, d in tree if cr.distance(c, d, k) <= max_dist]
    label = cr.components(n, kept)
    return label, int((label == np.arange(n)).sum())
