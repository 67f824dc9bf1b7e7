"""The rule of neighbour joining over a sketch set (mhx_dist_nj) as a plain statement, plain and slow: brute force over all
active pairs every join, in Python integers.  Shared by the neighbour-joining tests; not a test module itself.

    leaves      = d(i, j) = linkage_rule.fixed_distance(common, denom, k) of the triangle's pair, in units of 2^-32, 0 .. 2^32
    nodes       = a node's id is its lowest leaf; m = n active nodes at the start; r_i = the sum of d(i, c) over active c != i
    join        = while m > 2: Q(i, j) = (m - 2) d(i, j) - r_i - r_j; the pair with the smallest Q joins, among equal Q the
                  lower lo id, then the lower hi id; with b < a, b becomes the new node u and a dies
    update      = for every other active c: d(u, c) = max(0, (d(a, c) + d(b, c) - d(a, b)) >> 1), a floor.  The clamp at 0 is
                  a deliberate deviation from textbook neighbour joining (which lets negative distances stand): every
                  distance stays in 0 .. 2^32.  r_c += d(u, c) - d(a, c) - d(b, c), r_u = the sum of the d(u, c)
    records     = n - 1 of them, (a, b, d_ab, r_a, r_b) as the values were before the join, record t made with m = n - t; the
                  last one (m = 2) joins the two nodes that are left and has r_a = r_b = 0
    lengths     = m > 2: len_a = float(d (m - 2) + r_a - r_b) / float(2 (m - 2)) * 2^-32, len_b with r_a and r_b swapped; the
                  last record: len_a = d 2^-32, len_b = 0.  They may be negative and are reported as computed
    table       = per record "name_a\\tname_b\\tlen_a\\tlen_b\\tdist\\tnodes\\n": the names of the two ids (comments under -C),
                  the lengths and dist = d 2^-32 as the triangle prints a distance, nodes = m - 1 left after the join
    newick      = unrooted: every join but the last is a node "(X:len,Y:len)"; for n >= 3 the root is the trifurcation of the
                  two children of record n - 3 and the node that is left, the latter with the dist of record n - 2 as its length;
                  n = 2: "(name0:0,name1:d);", n = 1: "name;", n = 0: ""; children in the order of their lowest leaf; lengths
                  "%g" of max(0, len); names quoted as tree_rule.quoted quotes them; the text ends ";\\n"
"""
import numpy as np

from tests import linkage_rule as lr

ONE = 1 << 32
SCALE = 2.0 ** -32


def q_value(m, d, ri, rj):
    return (m - 2) * d - ri - rj


def join_word(dac, dbc, dab):
    """(d(u, c), whether the clamp changed it)"""
    v = (dac + dbc - dab) >> 1      # Python's >> floors
    return (0, True) if v < 0 else (v, False)


def lengths(d, m, r_a, r_b):
    if m <= 2:
        return float(d) * SCALE, 0.0
    return (float(d * (m - 2) + r_a - r_b) / float(2 * (m - 2)) * SCALE, float(d * (m - 2) + r_b - r_a) / float(2 * (m - 2)) * SCALE)


def leaf_words(common, denom, n, k):
    """D[hi][lo] of the n single lists from the packed triangle (tc.oracle_pairs)"""
    memo = {}
    D = [[0] * i for i in range(n)]
    p = 0
    for i in range(n):
        for j in range(i):
            key = (int(common[p]), int(denom[p]))
            if key not in memo:
                memo[key] = lr.fixed_distance(key[0], key[1], k)
            D[i][j] = memo[key]
            p += 1
    return D


def matrix_words(M):
    """D[hi][lo] from a full symmetric matrix of distance words"""
    return [[int(M[i][j]) for j in range(i)] for i in range(len(M))]


def join(D, count=None):
    """([(a, b, d, r_a, r_b)] of the n - 1 records in join order, updates the clamp changed) of D[hi][lo], which is used up.
    count (a dict) receives "ties": the comparisons of two candidates with equal Q"""
    n = len(D)
    active = list(range(n))
    r = [0] * n
    for i in range(n):
        for j in range(i):
            r[i] += D[i][j]
            r[j] += D[i][j]
    records, clamps, ties = [], 0, 0
    m = n
    while m > 2:
        best = None
        for x, hi in enumerate(active):        # (q, lo, hi) ascending
            row, rh = D[hi], r[hi]
            cands = [((m - 2) * row[lo] - rh - r[lo], lo, hi) for lo in active[:x]]
            if count is not None:
                for cand in cands:
                    if best is not None and cand[0] == best[0]:
                        ties += 1
                    if best is None or cand < best:
                        best = cand
            elif cands:
                first = min(cands)
                if best is None or first < best:
                    best = first
        _, b, a = best
        dab = D[a][b]
        records.append((a, b, dab, r[a], r[b]))
        active.remove(a)
        ru = 0
        for c in active:
            if c == b:
                continue
            dac = D[max(a, c)][min(a, c)]
            dbc = D[max(b, c)][min(b, c)]
            new, clamped = join_word(dac, dbc, dab)
            clamps += clamped
            D[max(b, c)][min(b, c)] = new
            r[c] += new - dac - dbc
            ru += new
        r[b] = ru
        m -= 1
    if n >= 2:
        b, a = active
        records.append((a, b, D[a][b], 0, 0))
    if count is not None:
        count["ties"] = ties
    return records, clamps


def records_of(common, denom, n, k, count=None):
    return join(leaf_words(common, denom, n, k), count)


def all_lengths(records):
    """(len_a, len_b) of every record as float64 arrays"""
    n = len(records) + 1
    both = [lengths(d, n - t, ra, rb) for t, (_, _, d, ra, rb) in enumerate(records)]
    return np.array([x[0] for x in both], np.float64), np.array([x[1] for x in both], np.float64)


def newick(names, records):
    from tests import tree_rule as tl

    n = len(names)
    if n == 0:
        return ""
    if n == 1:
        return tl.quoted(names[0]) + ";\n"
    la, lb = all_lengths(records)
    branch = lambda x: "%g" % max(0.0, float(x))   # noqa: E731
    text = {i: tl.quoted(names[i]) for i in range(n)}   # by the id of an active node
    if n == 2:
        a, b = records[0][:2]
        return "(%s:%s,%s:%s);\n" % (text[b], branch(lb[0]), text[a], branch(la[0]))
    for t in range(n - 3):
        a, b = records[t][:2]
        text[b] = "(%s:%s,%s:%s)" % (text[b], branch(lb[t]), text.pop(a), branch(la[t]))
    a, b = records[n - 3][:2]
    other = [i for i in records[n - 2][:2] if i != b]
    assert len(other) == 1 and sorted(text) == sorted([a, b, other[0]])
    kids = sorted([(b, lb[n - 3]), (a, la[n - 3]), (other[0], records[n - 2][2] * SCALE)])
    return "(" + ",".join("%s:%s" % (text[i], branch(x)) for i, x in kids) + ");\n"


# ---- file level ---------------------------------------------------------------------------------------------------------------
def records_of_file(F):
    """the records of a SketchFile (oracle.mash_oracle), its pairs by triangle_rule.pairs"""
    from tests import triangle_rule as tr

    rows = tr.pairs(F)
    common = np.array([r[2] for r in rows], np.uint32)
    denom = np.array([r[3] for r in rows], np.uint32)
    return records_of(common, denom, len(F.references), F.kmer_size)[0]


def table_text(F, comment=False):
    from oracle import mash_oracle as mo

    records = records_of_file(F)
    shown = [(r.comment if comment else r.name) for r in F.references]
    n = len(shown)
    la, lb = all_lengths(records)
    return "".join("%s\t%s\t%s\t%s\t%s\t%d\n" % (shown[a], shown[b], mo.fmt_g(la[t]), mo.fmt_g(lb[t]), mo.fmt_g(d * SCALE), n - 1 - t)
                   for t, (a, b, d, _, _) in enumerate(records))


def newick_text(F, comment=False):
    return newick([(r.comment if comment else r.name) for r in F.references], records_of_file(F))
