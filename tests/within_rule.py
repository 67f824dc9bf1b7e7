"""The rule of the bounded neighbourhood call (mhx_dist_within, mhx_within_files: `mash dist -d D -v P`) as a plain statement
over sketches, built from the pieces of the CPU oracle that are pinned by mash's own output for `mash dist`: compare
(compareSketches), p_value and fmt_g.  No mash output is recorded for `dist -d`: mash's CommandDistance prints a pair iff
distance <= -d && p <= -v, and that rule is restated here.  Shared by the within tests; not a test module itself.

    pair(q, r) = compare(reference r, query q): common, denom, distance
    hit        = a pair whose distance is <= max_dist (max_dist >= 1 keeps every pair, max_dist < 0 none: no distance is
                 negative; 0/0 -- two empty lists -- has distance 0)
    result     = per query ALL its hits, ascending by reference index; as CSR: row_off[q] = hits of the queries before q
    text       = for every query sketch, in argument order and then file order, its result as `mash dist` rows
                 "ref\\tquery\\tdistance\\tp\\tcommon/denom\\n" -- order 0: in reference order, what `mash dist -d` prints;
                 order 1: best first by the search's order (tests/search_rule.py: better) --; rows with p > max_p_value are dropped
"""
import numpy as np

from oracle import mash_oracle as mo
from tests import search_rule


def hits(pairs, max_dist):
    """pairs = [(ref, common, denom, distance)] of one query, by reference -> its result"""
    return [p for p in pairs if p[3] <= max_dist]


def within(queries, refs, s, k, max_dist):
    """hash lists in, per query [(ref, common, denom, distance)]"""
    return [hits([(r,) + tuple(mo.compare(refs[r], q, s, k)) for r in range(len(refs))], max_dist) for q in queries]


def csr(per_query):
    """the results of the queries as (row_off uint64 [nq + 1], ref, common, denom uint32, dist float64)"""
    row_off = np.zeros(len(per_query) + 1, np.uint64)
    row_off[1:] = np.cumsum([len(h) for h in per_query], dtype=np.uint64)
    flat = [p for h in per_query for p in h]
    cols = [np.array([p[a] for p in flat], np.uint32) for a in range(3)]
    return (row_off, *cols, np.array([p[3] for p in flat], np.float64))


def csr_from_matrix(common, denom, dist, max_dist):
    """the rule over a matrix of pairs [nq, nr]"""
    nq, nr = common.shape
    return csr([hits([(r, int(common[q, r]), int(denom[q, r]), float(dist[q, r])) for r in range(nr)], max_dist) for q in range(nq)])


def within_text(R, query_files, max_dist, max_p_value=1.0, order=0):
    """R and query_files are mo.SketchFile"""
    k = R.kmer_size
    rows = []
    for Q in query_files:
        s = min(R.sketch_size, Q.sketch_size)
        for q in Q.references:
            got = within([q.hashes], [x.hashes for x in R.references], s, k, max_dist)[0]
            if order == 1:
                got = search_rule.ranked(got)
            for r, common, denom, d in got:
                ref = R.references[r]
                p = mo.p_value(common, ref.length, q.length, 4.0 ** k, denom)
                if p <= max_p_value:
                    rows.append("%s\t%s\t%s\t%s\t%d/%d\n" % (ref.name, q.name, mo.fmt_g(d), mo.fmt_g(p), common, denom))
    return "".join(rows)
