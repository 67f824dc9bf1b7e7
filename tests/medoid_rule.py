"""The rule of the medoids of a partition (mhx_dist_medoids), of the pair "a list against its target" (mhx_dist_to) and of
the table with the distance-to-representative columns (mhx_cluster_reps_files) as a plain statement over the oracle's
pairs, in Python integers, with no float anywhere but in the printed columns.  Shared by the medoid tests; not a test
module itself.

    input      = n lists (n <= 65 536, s < 2^20) and label[n], label[i] the lowest index of i's cluster
    valid      = label[i] <= i and label[label[i]] == label[i] for all i; the rule holds for ANY valid partition
    sum[i]     = the sum of linkage_rule.fixed_distance(common, denom, k) (units of 2^-32) over all j != i with
                 label[j] == label[i]; (common, denom) = compare(list i, list j), the pair rule of the distance path
    medoid     = the member of a cluster with the smallest (sum, index); medoid[i] that of i's cluster; a singleton is
                 its own medoid with sum 0
    dist_to    = (common, denom) of compare(list i, list target[i]); the pair (i, i) goes through the rule like any other
    key        = sum << 16 | index (what the device takes the minimum of)
    text       = clusters numbered from 1 by their lowest member, members in index order, per reference
                 "cluster\\tsize\\trepresentative\\tmember\\tdist\\tp\\tcommon/denom\\n": the last three fields as the triangle's
                 edge row prints them for the pair (member, representative)
"""
import numpy as np

from oracle import mash_oracle as mo
from tests import cluster_rule as cr
from tests import linkage_rule as lr

MAX_N = 1 << 16
MAX_SUM = (MAX_N - 1) << 32
LINKAGES = {"single": 0, "complete": 1, "average": 2}


def valid(label):
    label = [int(l) for l in label]
    return all(0 <= l <= i and label[l] == l for i, l in enumerate(label))


def key(total, index):
    assert 0 <= total <= MAX_SUM and 0 <= index < MAX_N
    return total << 16 | index


def unkey(word):
    return word >> 16, word & 0xFFFF


def pair_table(common, denom, n, k):
    """D[i][j] = fixed_distance of the pair (i, j) from the packed triangle (tc.oracle_pairs), both ways round; D[i][i] = 0"""
    D = [[0] * n for _ in range(n)]
    p = 0
    for i in range(n):
        for j in range(i):
            D[i][j] = D[j][i] = lr.fixed_distance(int(common[p]), int(denom[p]), k)
            p += 1
    return D


def sums(D, label):
    """sum[i] as a list of Python integers"""
    label = [int(l) for l in label]
    assert valid(label)
    n = len(label)
    return [sum(D[i][j] for j in range(n) if j != i and label[j] == label[i]) for i in range(n)]


def medoids(total, label):
    """medoid[i]: the member of i's cluster with the smallest (sum, index)"""
    label = [int(l) for l in label]
    best = {}
    for i, l in enumerate(label):
        if l not in best or (total[i], i) < best[l]:
            best[l] = (total[i], i)
    return [best[l][1] for l in label]


def dist_to(lists, s, k, target):
    """(common, denom) of compare(list i, list target[i]) as two lists of integers"""
    out = [mo.compare(lists[i], lists[int(t)], s, k)[:2] for i, t in enumerate(target)]
    return [int(c) for c, _ in out], [int(d) for _, d in out]


def medoids_of(lists, s, k, label, pairs):
    """(medoid, sum, common, denom) of the rule; pairs: tc.oracle_pairs of the set"""
    n = len(lists)
    total = sums(pair_table(pairs[0], pairs[1], n, k), label)
    med = medoids(total, label)
    common, denom = dist_to(lists, s, k, med)
    return med, total, common, denom


# ---- file level ---------------------------------------------------------------------------------------------------------------
def file_labels(F, max_dist, linkage="single"):
    """the labels mhx_cluster_reps_files starts from"""
    if linkage == "single":
        return [int(l) for l in cr._file_clusters(F, max_dist)[0]]
    merges, dist = lr.merges_of(F, LINKAGES[linkage])
    return [int(l) for l in lr.labels(merges, dist, len(F.references), max_dist)[0]]


def representatives(F, max_dist, linkage="single", rep="medoid"):
    """(label, rep_of) with rep_of[l] the representative of the cluster with label l"""
    from tests import triangle_rule as tr

    label = file_labels(F, max_dist, linkage)
    n = len(label)
    roots = [i for i in range(n) if label[i] == i]
    if rep == "medoid":
        rows = tr.pairs(F)
        D = pair_table([r[2] for r in rows], [r[3] for r in rows], n, F.kmer_size)
        med = medoids(sums(D, label), label)
        return label, {l: med[l] for l in roots}
    return label, {l: cr._representative(F, [i for i in range(n) if label[i] == l], rep) for l in roots}


def reps_text(F, max_dist, linkage="single", rep="medoid", comment=False):
    label, rep_of = representatives(F, max_dist, linkage, rep)
    refs = F.references
    shown = [(r.comment if comment else r.name) for r in refs]
    n = len(label)
    text = []
    for number, root in enumerate(sorted(rep_of), 1):
        members = [i for i in range(n) if label[i] == root]
        r = rep_of[root]
        for i in members:
            common, denom, d = mo.compare(refs[i].hashes, refs[r].hashes, F.sketch_size, F.kmer_size)
            p = mo.p_value(common, refs[i].length, refs[r].length, 4.0 ** F.kmer_size, denom)
            text.append("%d\t%d\t%s\t%s\t%s\t%s\t%d/%d\n" % (number, len(members), shown[r], shown[i], mo.fmt_g(d), mo.fmt_g(p), common, denom))
    return "".join(text)


def reps_file(F, max_dist, linkage="single", rep="medoid"):
    """the SketchFile that -o writes: the representatives in cluster order, unchanged"""
    _, rep_of = representatives(F, max_dist, linkage, rep)
    return mo.SketchFile(F.kmer_size, F.sketch_size, [F.references[rep_of[l]] for l in sorted(rep_of)])
