"""The rule of the single-linkage clustering (mhx_dist_cluster, mhx_cluster_files) as a plain statement over a set of
sketches, built from the piece of the CPU oracle that mash's own output pins for `mash dist`: compare (compareSketches).
Shared by the cluster tests; not a test module itself.

    pair(i, j) = compare(list i, list j) for j < i: common, denom, distance
    edge       = a pair with distance <= max_dist
    cluster    = a connected component of the graph of the edges (breadth-first search -- deliberately not a union-find,
                 which is what the library runs); label[i] = the lowest index in i's component
    degree[i]  = the edges that i is an end of
    cmin[d]    = the smallest c in 0 .. d with distance(c, d) <= max_dist, d + 1 when there is none (the linear definition)
    text       = clusters numbered from 1 by their lowest member, members in index order, per reference
                 "cluster\\tsize\\trepresentative\\tmember\\tdegree\\n" with names (comments under -C); the representative
                 is the lowest member ("first") or the member of greatest length, ties to the lower index ("longest")
"""
import functools
import math
from collections import deque

import numpy as np

from oracle import mash_oracle as mo
from tests import triangle_cases as tc
from tests import triangle_rule as tr


def packed_indices(n):
    """(i, j) of every packed pair, in the order of tc.oracle_pairs: i ascending, j < i ascending"""
    ii = np.array([i for i in range(n) for j in range(i)], np.int64)
    jj = np.array([j for i in range(n) for j in range(i)], np.int64)
    return ii, jj


def edges(lists, s, k, max_dist, pairs=None):
    """[(i, j)], j < i, of the pairs whose oracle distance is <= max_dist; pairs: tc.oracle_pairs of the set, if at hand"""
    _, _, dist = pairs if pairs is not None else tc.oracle_pairs(lists, s, k)
    ii, jj = packed_indices(len(lists))
    keep = np.flatnonzero(dist <= max_dist)
    return list(zip(ii[keep].tolist(), jj[keep].tolist()))


def components(n, edge_list):
    """label[i] = the lowest index of i's connected component, by breadth-first search from every index in ascending order"""
    near = [[] for _ in range(n)]
    for i, j in edge_list:
        near[i].append(j)
        near[j].append(i)
    label = np.full(n, -1, np.int64)
    for start in range(n):
        if label[start] >= 0:
            continue
        label[start] = start
        todo = deque([start])
        while todo:
            x = todo.popleft()
            for y in near[x]:
                if label[y] < 0:
                    label[y] = start
                    todo.append(y)
    return label.astype(np.uint32)


def degree(n, edge_list):
    out = np.zeros(n, np.uint32)
    for i, j in edge_list:
        out[i] += 1
        out[j] += 1
    return out


def cluster(lists, s, k, max_dist, pairs=None):
    """(label, degree, n_clusters, n_edges) of the rule"""
    n = len(lists)
    e = edges(lists, s, k, max_dist, pairs)
    label = components(n, e)
    return label, degree(n, e), int((label == np.arange(n)).sum()), len(e)


# ---- the bound as integers --------------------------------------------------------------------------------------------------
def distance(common, denom, k):
    """the distance of a pair with these counts, the arithmetic of compareSketches in the same doubles and libm's log
    (tests/test_cluster_rule.py holds it against mo.compare)"""
    if common == denom:
        return 0.0
    if common == 0:
        return 1.0
    jac = common / denom
    d = -math.log(2.0 * jac / (1.0 + jac)) / k
    return 1.0 if d > 1.0 else d


@functools.lru_cache(maxsize=None)
def distance_row(denom, k):
    """distance(c, denom) for c = 0 .. denom"""
    return np.array([distance(c, denom, k) for c in range(denom + 1)], np.float64)


def cmin_at(d, k, max_dist, row=None):
    """the linear definition for one denom: the first c of 0 .. d that passes, d + 1 when none does"""
    if row is not None:
        hit = np.flatnonzero(row <= max_dist)
        return int(hit[0]) if hit.size else d + 1
    for c in range(d + 1):
        if distance(c, d, k) <= max_dist:
            return c
    return d + 1


def cmin_table(s, k, max_dist):
    """cmin[0 .. s] by the linear definition (the distances of a denom are computed once per k and kept)"""
    return np.array([cmin_at(d, k, max_dist, distance_row(d, k)) for d in range(s + 1)], np.uint32)


# ---- file level ---------------------------------------------------------------------------------------------------------------
def _file_clusters(F, max_dist):
    lists = [r.hashes for r in F.references]
    n = len(lists)
    rows = tr.pairs(F)
    e = [(i, j) for i, j, _, _, d, _ in rows if d <= max_dist]
    label = components(n, e)
    return label, degree(n, e)


def _representative(F, members, rep):
    if rep == "first":
        return members[0]
    assert rep == "longest"
    best = members[0]
    for i in members[1:]:
        if F.references[i].length > F.references[best].length:
            best = i
    return best


def representatives(F, max_dist, rep="first"):
    """index of the representative of every cluster, in cluster order"""
    label, _ = _file_clusters(F, max_dist)
    roots = [i for i in range(len(label)) if label[i] == i]
    return [_representative(F, [i for i in range(len(label)) if label[i] == root], rep) for root in roots]


def representatives_file(F, max_dist, rep="first"):
    """the SketchFile that -o writes: the representatives in cluster order, unchanged"""
    return mo.SketchFile(F.kmer_size, F.sketch_size, [F.references[i] for i in representatives(F, max_dist, rep)])


def cluster_text(F, max_dist, comment=False, rep="first"):
    label, deg = _file_clusters(F, max_dist)
    shown = [(r.comment if comment else r.name) for r in F.references]
    roots = [i for i in range(len(label)) if label[i] == i]
    text = []
    for number, root in enumerate(roots, 1):
        members = [i for i in range(len(label)) if label[i] == root]
        r = _representative(F, members, rep)
        for i in members:
            text.append("%d\t%d\t%s\t%s\t%d\n" % (number, len(members), shown[r], shown[i], deg[i]))
    return "".join(text)
