"""The rule of complete and average linkage (mhx_dist_linkage) as a plain statement over the oracle's pairs, plain and slow:
brute force over all active pairs every step, in Python integers.  Shared by the linkage tests; not a test module itself.

    clusters    = a cluster's id is its lowest member; n clusters {i} at the start; every step the pair of active clusters
                  with the smallest linkage value merges, among equal values the lower lo id, then the lower hi id; the merged
                  cluster keeps id lo; n - 1 steps
    complete    = the value of a cluster pair is the (common, denom) of its worst leaf pair: the smallest index common / denom,
                  compared exactly, common == denom counting as 1/1; V(A u B, C) is the worse of V(A, C) and V(B, C), of two
                  equal indices the one with the greater denom
    average     = the value is num / den, num the sum over all leaf pairs of fixed_distance (units of 2^-32), den = |A| |B|;
                  V(A u B, C) = (num_AC + num_BC, den_AC + den_BC); compared as num1 den2 against num2 den1
    heights     = complete: the oracle's distance (cluster_rule.distance, host libm) of the decisive pair; average:
                  (float(num) / float(den)) * 2^-32
    cut         = the merges from the first one on while dist[t] <= max_dist, none behind the first that is not; label[i] = the
                  lowest index of i's cluster
"""
import numpy as np

from tests import cluster_rule as cr

COMPLETE, AVERAGE = 1, 2
ONE = 1 << 32
LN2 = 2977044471   # floor(ln 2 * 2^32)
MASK = (1 << 64) - 1


def fixed_distance(common, denom, k):
    """q(common, denom, k): the distance in units of 2^-32 by integers alone"""
    common, denom = int(common), int(denom)
    if common == denom:
        return 0
    if common == 0:
        return ONE
    y = ((common + denom) << 42) // (2 * common)
    e = y.bit_length() - 1
    z = (y << (63 - e)) & MASK
    G = e - 42
    for _ in range(40):
        z = (z * z) >> 64
        if z >= 1 << 63:
            G = 2 * G + 1
        else:
            G = 2 * G
            z = (z << 1) & MASK
    return min(ONE, ((G * LN2) >> 40) // k)


def _index(v):
    return (1, 1) if v[0] == v[1] else v


def closer(linkage, a, b):
    """-1: value a is the smaller linkage value, 0: equal, 1: b is.  complete: (common, denom); average: (num, den)"""
    if linkage == COMPLETE:
        (an, ad), (bn, bd) = _index(a), _index(b)
        l, r = bn * ad, an * bd     # the greater index is the smaller distance
    else:
        l, r = a[0] * b[1], b[0] * a[1]
    return -1 if l < r else (1 if l > r else 0)


def combine(linkage, a, b):
    if linkage == AVERAGE:
        return (a[0] + b[0], a[1] + b[1])
    c = closer(COMPLETE, a, b)
    if c != 0:
        return b if c < 0 else a    # the worse one
    return a if a[1] >= b[1] else b


def leaf_values(common, denom, n, k, linkage):
    """V[hi][lo] of the n single lists from the packed triangle (tc.oracle_pairs)"""
    V = [[None] * i for i in range(n)]
    p = 0
    for i in range(n):
        for j in range(i):
            c, d = int(common[p]), int(denom[p])
            V[i][j] = (c, d) if linkage == COMPLETE else (fixed_distance(c, d, k), 1)
            p += 1
    return V


def best_partners(V, active, linkage):
    """{i: the best active j < i of row i, ties to the lower j} for every active i that has one"""
    out = {}
    for x, i in enumerate(active):
        best = None
        for j in active[:x]:
            if best is None or closer(linkage, V[i][j], V[i][best]) < 0:
                best = j
        if best is not None:
            out[i] = best
    return out


def agglomerate(common, denom, n, k, linkage, trace=False):
    """[(a, b, size, num, den)] of the n - 1 merges in merge order, a > b; with trace also best_partners after every step"""
    V = leaf_values(common, denom, n, k, linkage)
    active = list(range(n))
    size = [1] * n
    merges, partners = [], []
    for _ in range(max(n - 1, 0)):
        best = None
        for x, lo in enumerate(active):            # (lo, hi) ascending: the first of equal values stays
            for hi in active[x + 1:]:
                v = V[hi][lo]
                if best is None or closer(linkage, v, best[0]) < 0:
                    best = (v, lo, hi)
        v, b, a = best
        size[b] += size[a]
        merges.append((a, b, size[b], v[0], v[1]))
        active.remove(a)
        for c in active:
            if c == b:
                continue
            va = V[max(a, c)][min(a, c)]
            vb = V[max(b, c)][min(b, c)]
            V[max(b, c)][min(b, c)] = combine(linkage, va, vb)
        if trace:
            partners.append(best_partners(V, active, linkage))
    return (merges, partners) if trace else merges


def heights(merges, k, linkage):
    if linkage == COMPLETE:
        return np.array([cr.distance(num, den, k) for _, _, _, num, den in merges], np.float64)
    return np.array([(float(num) / float(den)) * 2.0 ** -32 for _, _, _, num, den in merges], np.float64)


def labels(merges, dists, n, max_dist):
    """(label, n_clusters, merges applied) of the cut at max_dist"""
    label = list(range(n))
    applied = 0
    for (a, b, *_), d in zip(merges, dists):
        if not d <= max_dist:
            break
        label = [b if l == a else l for l in label]
        applied += 1
    return np.array(label, np.uint32), n - applied, applied


# ---- file level ---------------------------------------------------------------------------------------------------------------
def merges_of(F, linkage):
    """(merges, heights) of a SketchFile (oracle.mash_oracle), its pairs by triangle_rule.pairs"""
    from tests import triangle_rule as tr

    rows = tr.pairs(F)
    common = np.array([r[2] for r in rows], np.uint32)
    denom = np.array([r[3] for r in rows], np.uint32)
    merges = agglomerate(common, denom, len(F.references), F.kmer_size, linkage)
    return merges, heights(merges, F.kmer_size, linkage)


def table_text(F, linkage, comment=False):
    """per merge "name_a\\tname_b\\tdist\\tsize\\tclusters\\n": the names of the two ids, the height as the triangle prints a
    distance, the members of the merged cluster, the clusters left"""
    from oracle import mash_oracle as mo

    merges, dist = merges_of(F, linkage)
    shown = [(r.comment if comment else r.name) for r in F.references]
    n = len(shown)
    return "".join("%s\t%s\t%s\t%d\t%d\n" % (shown[a], shown[b], mo.fmt_g(d), size, n - 1 - t) for t, ((a, b, size, _, _), d) in enumerate(zip(merges, dist)))


def newick_text(F, linkage, comment=False):
    from tests import tree_rule as tl

    merges, dist = merges_of(F, linkage)
    return tl.newick([(r.comment if comment else r.name) for r in F.references], merges, dist)


def cut_clusters(F, linkage, max_dist, rep="first"):
    """[(members, representative)] of the cut at max_dist, clusters by their lowest member, members in index order"""
    merges, dist = merges_of(F, linkage)
    n = len(F.references)
    label, _, _ = labels(merges, dist, n, max_dist)
    out = []
    for root in [i for i in range(n) if label[i] == i]:
        members = [i for i in range(n) if label[i] == root]
        out.append((members, cr._representative(F, members, rep)))
    return out


def cut_text(F, linkage, max_dist, comment=False, rep="first"):
    """per reference "cluster\\tsize\\trepresentative\\tmember\\n" (cluster_rule.cluster_text without the degree column)"""
    shown = [(r.comment if comment else r.name) for r in F.references]
    return "".join("%d\t%d\t%s\t%s\n" % (number, len(members), shown[r], shown[i])
                   for number, (members, r) in enumerate(cut_clusters(F, linkage, max_dist, rep), 1) for i in members)
