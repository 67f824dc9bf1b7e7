"""The rule of the reference-set search (mhx_dist_search, mhx_search_files) as a plain statement over sketches, built from
the pieces of the CPU oracle that are pinned by mash's own output for `mash dist`: compare (compareSketches), p_value and
fmt_g.  No mash output is recorded for it (mash has no such command).  Shared by the search tests; not a test module itself.

    pair(q, r) = compare(reference r, query q): common, denom, distance
    rank       = by the Jaccard index common / denom, compared exactly: a is better than b iff
                 a.common * b.denom > b.common * a.denom in integers; common == denom counts as 1/1 (that includes 0/0, two
                 empty lists, whose distance is 0); pairs of equal index go by the lower reference index.  A total order.
                 Not by the distance: it is clamped to 1, so for small k many indices print as 1.
    hit        = a pair whose distance is <= max_dist (max_dist >= 1 keeps everything; max_dist < 0 keeps nothing: no
                 distance is negative).  The device-pointer form of mhx_dist_search only prefilters, and its prefilter
                 takes a negative bound for 0: there its lists are the rule's at max_dist = 0, the pairs of distance 0
    result     = per query the first min(top, hits) hits in rank order
    text       = for every query sketch, in argument order and then file order, its result as `mash dist` rows
                 "ref\\tquery\\tdistance\\tp\\tcommon/denom\\n"; rows with p > max_p_value are dropped from the result
                 already chosen -- nothing moves up into their place
"""
import functools

from oracle import mash_oracle as mo


def index(common, denom):
    """the Jaccard index of a pair as an exact fraction (numerator, denominator)"""
    return (1, 1) if common == denom else (common, denom)


def better(a, b):
    """a, b = (ref, common, denom)"""
    (an, ad), (bn, bd) = index(a[1], a[2]), index(b[1], b[2])
    if an * bd != bn * ad:
        return an * bd > bn * ad
    return a[0] < b[0]


def ranked(pairs):
    """(ref, common, denom, ...) tuples, best first"""
    return sorted(pairs, key=functools.cmp_to_key(lambda a, b: -1 if better(a, b) else (1 if better(b, a) else 0)))


def select(pairs, top, max_dist=1.0):
    """pairs = [(ref, common, denom, distance)] of one query -> its result"""
    return ranked([p for p in pairs if p[3] <= max_dist])[:top]


def search(queries, refs, s, k, top, max_dist=1.0):
    """hash lists in, per query [(ref, common, denom, distance)]"""
    return [select([(r,) + tuple(mo.compare(refs[r], q, s, k)) for r in range(len(refs))], top, max_dist) for q in queries]


def search_text(R, query_files, top=5, max_dist=1.0, max_p_value=1.0):
    """R and query_files are mo.SketchFile"""
    k = R.kmer_size
    rows = []
    for Q in query_files:
        s = min(R.sketch_size, Q.sketch_size)
        for q in Q.references:
            for r, common, denom, d in search([q.hashes], [x.hashes for x in R.references], s, k, top, max_dist)[0]:
                ref = R.references[r]
                p = mo.p_value(common, ref.length, q.length, 4.0 ** k, denom)
                if p <= max_p_value:
                    rows.append("%s\t%s\t%s\t%s\t%d/%d\n" % (ref.name, q.name, mo.fmt_g(d), mo.fmt_g(p), common, denom))
    return "".join(rows)
